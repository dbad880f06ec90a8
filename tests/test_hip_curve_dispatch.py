"""GPU: ``expo_filter_dispatch_curves_fwd / _bwd`` and ``expo_heads_regress_curves_fwd / _bwd`` through their bindings,
image by image against the float64 oracle (tests/_curve_dispatch_ref.py): every step count the kernels branch on, ids that
put -1, Tone, Color and the light filters side by side in one launch, the vector path, the element-wise tail path and
more curve blocks per image than the product shape has; exact zeros, bit reproducibility, the bits of the 8-step
dispatch on the rows whose bodies are shared; the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from tests import _agent_glue_ref as R
from tests import _curve_dispatch_ref as C
from tests._tol import assert_image_close, assert_param_grad_close

pytestmark = pytest.mark.gpu
NP_DT = {torch.float16: np.float16, torch.float32: np.float32}
STEPS = (1, 5, 8, 12, 16)
# (name, shape, ids): the product shape (two curve blocks per image), the element-wise tail path, four curve blocks, and
# at 64x64 one batch with nothing for the light launch and one with nothing for the curve launch
cycle = lambda n: (np.arange(n) % 10 - 1).astype(np.int32)  # -1, 0 .. 8, -1, ...
CASES = {
    'product': ((11, 64, 64, 3), cycle(11)),
    'tail': ((11, 7, 5, 3), cycle(11)),
    'four_blocks': ((10, 96, 80, 3), cycle(10)),
    'all_curves': ((4, 64, 64, 3), np.array([4, 7, 7, 4], dtype=np.int32)),
    'all_light': ((8, 64, 64, 3), np.array([0, 1, 2, 3, 5, 6, 8, 0], dtype=np.int32)),
}


def run(dev, dtype, x, dy, ids, rows, steps, dpen, need_dx=True, with_pen=True):
  """One forward and one backward; every output starts from a pattern the kernels must overwrite."""
  tx, tdy = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
  tid, tp = torch.from_numpy(ids).to(dev), torch.from_numpy(rows).to(dev)
  n = x.shape[0]
  y = torch.full_like(tx, 3.0)
  pen = torch.full((n,), -3.0, device=dev) if with_pen else None
  _cabi.dispatch_curves_fwd(tid, tx, y, tp, steps, pen)
  dx = torch.full_like(tx, 3.0) if need_dx else None
  dp = torch.full((n, C.WIDE), float('nan'), device=dev)
  tdpen = torch.from_numpy(dpen).to(dev) if dpen is not None else None
  _cabi.dispatch_curves_bwd(tid, tx, tdy, dx, tp, dp, steps, tdpen)
  torch.cuda.synchronize()
  return dict(y=y.cpu().numpy(), pen=None if pen is None else pen.cpu().numpy(), dx=None if dx is None else dx.cpu().numpy(),
              dp=dp.cpu().numpy())


def bits(a):
  return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('steps', STEPS)
def test_dispatch_for_any_step_count_against_the_oracle(steps, case, dtype, gpu_device):
  dev = gpu_device
  npdt = NP_DT[dtype]
  shape, ids = CASES[case]
  n = shape[0]
  seed = 1000 * steps + 10 * list(CASES).index(case) + (dtype == torch.float32)
  x, dy = C.make_inputs(seed, shape, npdt, steps)
  rows = C.make_rows(seed + 1, ids, steps, hump_rows=(0, 1) if case == 'all_curves' else ())
  dpen = (np.random.default_rng(seed + 2).standard_normal(n) * 50.0).astype(np.float32)
  got = run(dev, dtype, x, dy, ids, rows, steps, dpen)
  ry, rpen, rdx, rdp, adp = C.dispatch_oracle(x, dy, ids, rows, steps, dpen)
  what = 'L = %d %s %s' % (steps, case, npdt.__name__)
  # (a one-step curve is clip(x, 0, 1) whatever its parameter: the all-curve batch has no over-exposed image at L = 1)
  live = not (case == 'all_curves' and steps == 1)
  assert (rpen > 1e-4).any() == live, 'the case must exercise the penalty'
  if case == 'all_curves' and live:
    assert rpen[0] > 1e-3 and rpen[1] > 1e-3, 'a curve image must exercise the live penalty'
  assert_image_close(got['y'], ry, npdt, what + ' y')
  on_knot = C.on_knot_mask(x.astype(np.float64), steps) & np.isin(ids, (4, 7))[:, None, None, None]
  assert C.on_knot_mask(x.astype(np.float64), steps).mean() < 0.01
  assert_image_close(np.where(on_knot, 0, got['dx']), np.where(on_knot, 0, rdx), npdt, what + ' dx')
  assert_param_grad_close(got['dp'], rdp, adp, what + ' dparams')
  np.testing.assert_allclose(got['pen'], rpen, rtol=2e-4, atol=1e-7)
  # exactly 0 behind a filter's parameters and in the rows that selected nothing; y and dx of id -1 are all-zero bits
  counts = np.array([C.num_params(int(f), steps) if f >= 0 else 0 for f in ids])
  behind = np.arange(C.WIDE)[None, :] >= counts[:, None]
  assert (bits(got['dp'])[behind] == 0).all(), what
  none = ids < 0
  if none.any():
    assert (bits(got['y'][none]) == 0).all() and (bits(got['dx'][none]) == 0).all() and got['pen'][none].max() == 0
  # dx is optional and does not change dparams; a second run gives the same bits of everything
  no_dx = run(dev, dtype, x, dy, ids, rows, steps, dpen, need_dx=False)
  assert no_dx['dx'] is None and np.array_equal(bits(no_dx['dp']), bits(got['dp'])), what
  again = run(dev, dtype, x, dy, ids, rows, steps, dpen)
  for key in ('y', 'pen', 'dx', 'dp'):
    assert np.array_equal(bits(again[key]), bits(got[key])), (what, key)
  # a dpenalty of zeros is no dpenalty, bit for bit; a live one moves the parameter gradient of an over-exposed row
  zero = run(dev, dtype, x, dy, ids, rows, steps, np.zeros(n, dtype=np.float32))
  off = run(dev, dtype, x, dy, ids, rows, steps, None)
  for key in ('y', 'dx', 'dp'):
    assert np.array_equal(bits(zero[key]), bits(off[key])), (what, key)
  if live:
    hot = int(np.argmax(rpen))
    assert rpen[hot] > 1e-4 and dpen[hot] != 0 and not np.array_equal(got['dp'][hot], off['dp'][hot]), what


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('case', ['product', 'tail', 'four_blocks'])
@pytest.mark.parametrize('steps', [5, 16])
def test_light_rows_have_the_bits_of_the_eight_step_dispatch(steps, case, dtype, gpu_device):
  """Every id but 4 and 7 runs the body of expo_filter_dispatch_fwd / _bwd: y, dx and (the finish keeps the summation
  order) dparams of those images are the same bits as that entry's on the same image and the first 24 slots."""
  dev = gpu_device
  npdt = NP_DT[dtype]
  shape, ids = CASES[case]
  n = shape[0]
  x, dy = C.make_inputs(7 + steps, shape, npdt, steps)
  rows = C.make_rows(8 + steps, ids, steps)
  dpen = (np.random.default_rng(9).standard_normal(n) * 50.0).astype(np.float32)
  got = run(dev, dtype, x, dy, ids, rows, steps, dpen)
  light = ~np.isin(ids, (4, 7))
  ids8 = np.where(light, ids, -1).astype(np.int32)  # (the curve images: nothing for the narrow entry to do)
  tx, tdy = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
  tid, tp = torch.from_numpy(ids8).to(dev), torch.from_numpy(np.ascontiguousarray(rows[:, :24])).to(dev)
  y, dx = torch.empty_like(tx), torch.empty_like(tx)
  pen, dp = torch.empty(n, device=dev), torch.empty((n, 24), device=dev)
  _cabi.dispatch_fwd(tid, tx, y, tp, pen)
  _cabi.dispatch_bwd(tid, tx, tdy, dx, tp, dp, torch.from_numpy(dpen).to(dev))
  torch.cuda.synchronize()
  assert light.sum() >= 7
  assert np.array_equal(bits(got['y'][light]), bits(y.cpu().numpy()[light]))
  assert np.array_equal(bits(got['dx'][light]), bits(dx.cpu().numpy()[light]))
  assert np.array_equal(bits(got['dp'][light, :24]), bits(dp.cpu().numpy()[light]))


# ---- heads --------------------------------------------------------------------------------------------------------------
def heads_run(dev, raws, ids, ranges, selected, dparams, steps):
  n = raws[0].shape[0]
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  traws = [t(r) for r in raws]
  params = torch.full((n, C.WIDE), float('nan'), device=dev)
  _cabi.heads_regress_curves_fwd(traws, ids, ranges, t(selected), params, steps)
  draws = [torch.full(tuple(r.shape), float('nan'), device=dev) for r in raws]
  _cabi.heads_regress_curves_bwd(traws, draws, ids, ranges, t(selected), t(dparams), steps)
  return params.cpu().numpy(), [d.cpu().numpy() for d in draws]


HEADS_WITH_CURVES = [name for name, ids in R.HEAD_LISTS.items() if 4 in ids or 7 in ids]


@pytest.mark.parametrize('ranges', [R.shipped_ranges(), R.biased_ranges()], ids=['shipped', 'biased'])
@pytest.mark.parametrize('heads', HEADS_WITH_CURVES)
@pytest.mark.parametrize('steps', [1, 5, 16])
def test_heads_for_any_step_count_against_the_float64_reference(steps, heads, ranges, gpu_device):
  """The grid of tests/test_hip_agent_glue.py::test_heads_against_the_float64_reference on the head lists with a curve."""
  ids = R.HEAD_LISTS[heads]
  for n in R.HEAD_NS:
    for mask_features in (6, 0):
      raws, selected, dparams = C.heads_inputs(ids, n, mask_features, 100 + n + mask_features, steps)
      what = 'L = %d %s n %d mask features %d' % (steps, heads, n, mask_features)
      params, draws = heads_run(gpu_device, raws, ids, ranges, selected, dparams, steps)
      assert np.isfinite(params).all() and all(np.isfinite(d).all() for d in draws), what
      R.assert_close(params, C.heads_fwd(raws, ids, ranges, selected, steps), R.C_PARAMS, R.C_PARAMS, 1, what + ' params')
      counts = np.array([C.num_params(ids[j], steps) if j >= 0 else 0 for j in selected])
      assert (params[np.arange(C.WIDE)[None, :] >= counts[:, None]] == 0).all(), what
      d_ref, scale = C.heads_bwd(raws, ids, ranges, selected, dparams, steps)
      for j, fid in enumerate(ids):
        p = C.num_params(fid, steps)
        R.assert_close(draws[j], d_ref[j], 0, R.C_DRAW, scale[j], what + ' d raw of head %d (filter %d)' % (j, fid))
        assert (draws[j][selected != j] == 0).all() and (draws[j][:, p:] == 0).all(), (what, j)


def test_wide_heads_at_eight_steps_equal_the_narrow_entry(gpu_device):
  dev = gpu_device
  ids = R.HEAD_LISTS['nine_with_level']
  ranges = R.biased_ranges()
  raws, selected, dparams = C.heads_inputs(ids, 257, 6, 5, 8)
  params, _ = heads_run(dev, raws, ids, ranges, selected, dparams, 8)
  t = lambda a: torch.from_numpy(a).to(dev)
  narrow = torch.empty((257, 24), device=dev)
  _cabi.heads_regress_fwd([t(r) for r in raws], ids, ranges, t(selected), narrow)
  R.assert_close(params[:, :24], narrow.cpu().numpy().astype(np.float64), R.C_PARAMS, R.C_PARAMS, 1, 'wide vs narrow')
  assert (params[:, 24:] == 0).all()


# ---- argument checks ----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_enqueued(gpu_device):
  lib = _cabi.load()
  dev = gpu_device
  bad, ok = -1, 0
  n, h, w = 3, 8, 8
  x = torch.zeros((n, h, w, 3), dtype=torch.float16, device=dev)
  y, dy, dx = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
  prm, dprm = torch.zeros((n, C.WIDE), device=dev), torch.zeros((n, C.WIDE), device=dev)
  pen = torch.zeros(n, device=dev)
  ids = torch.zeros(n, dtype=torch.int32, device=dev)
  need = lib.expo_filter_dispatch_curves_workspace_bytes(n, h, w, 0, 16)
  ws = torch.zeros(need, dtype=torch.uint8, device=dev)
  torch.cuda.synchronize()
  ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

  def fwd(steps=16, n=n, wsp=ws, wsb=need, penalty=pen, dtype=0):
    return lib.expo_filter_dispatch_curves_fwd(ptr(ids), ptr(x), ptr(y), ptr(prm), steps, ptr(penalty), n, h, w, dtype, ptr(wsp),
                                               wsb, None)

  def bwd(steps=16, n=n, wsp=ws, wsb=need, mode=0, dtype=0):
    return lib.expo_filter_dispatch_curves_bwd(ptr(ids), ptr(x), ptr(dy), ptr(dx), ptr(prm), ptr(dprm), ptr(pen), steps, n, h, w,
                                               dtype, mode, ptr(wsp), wsb, None)

  for call in (fwd, bwd):
    for steps in (0, 17, -1):
      assert call(steps=steps) == bad and b'curve_steps' in lib.expo_last_error()
    assert call(wsp=None, wsb=0) == bad and b'workspace' in lib.expo_last_error()
    assert call(wsb=need - 4) == bad and b'workspace' in lib.expo_last_error()
    assert call(dtype=7) == -2
    assert call(n=-1) == bad
    assert call(n=0) == ok and call(n=0, wsp=None, wsb=0) == ok
  assert bwd(mode=2) == bad
  assert lib.expo_filter_dispatch_curves_fwd(None, ptr(x), ptr(y), ptr(prm), 16, None, n, h, w, 0, None, 0, None) == bad
  with pytest.raises(_cabi.ExposureHipError, match='curve_steps'):
    _cabi.dispatch_curves_fwd(ids, x, y, prm, 17)
  with pytest.raises(_cabi.ExposureHipError, match='shape'):
    _cabi.dispatch_curves_fwd(ids, x, y, prm[:, :24].contiguous(), 16)

  # the heads: the filter ids live on the host and are checked there ([0, 8]), like the widths and the step count
  raws = [torch.zeros((n, 64), device=dev) for _ in range(17)]
  draws = [torch.zeros((n, 64), device=dev) for _ in range(17)]
  rng = (ctypes.c_float * 9)(*[float(v) for v in R.shipped_ranges()])

  def heads(count, abi=None, widths=None, n=n, back=False, steps=16):
    m = max(count, 1)
    abi = abi or [0] * m
    widths = widths or [64] * m
    r = (ctypes.c_void_p * m)(*[ptr(t) for t in raws[:m]])
    d = (ctypes.c_void_p * m)(*[ptr(t) for t in draws[:m]])
    wd, a = (ctypes.c_int * m)(*widths), (ctypes.c_int * m)(*abi)
    if back:
      return lib.expo_heads_regress_curves_bwd(r, d, wd, a, count, rng, ptr(ids), ptr(prm), steps, n, None)
    return lib.expo_heads_regress_curves_fwd(r, wd, a, count, rng, ptr(ids), ptr(prm), steps, n, None)

  for back in (False, True):
    assert heads(0, back=back) == bad and heads(17, back=back) == bad
    assert heads(2, abi=[0, 9], back=back) == bad and b'filter_id' in lib.expo_last_error()
    assert heads(2, abi=[-1, 0], back=back) == bad and heads(2, abi=[-2, 0], back=back) == bad
    assert heads(2, steps=0, back=back) == bad and heads(2, steps=17, back=back) == bad
    assert heads(2, abi=[0, 7], widths=[1, 47], back=back) == bad  # the colour curve has 48 parameters at 16 steps
    assert heads(2, abi=[4, 2], widths=[15, 3], back=back) == bad
    assert heads(2, abi=[0, 7], widths=[1, 15], steps=5, back=back) == ok
    assert heads(2, n=-1, back=back) == bad
    assert heads(2, abi=[0, 7], widths=[1, 48], n=0, back=back) == ok
  torch.cuda.synchronize()
  for t in (y, dx, dprm, pen, prm) + tuple(draws):
    assert float(t.float().abs().sum()) == 0  # nothing ran
  # the per-image ids live on the device and are not read on the host: an id outside [-1, 8] selects nothing, like -1
  wild = torch.tensor([9, -2, 1000], dtype=torch.int32, device=dev)
  xs = torch.full_like(x, 0.5)
  out, dxo = torch.full_like(x, 3.0), torch.full_like(x, 3.0)
  dpo = torch.full((n, C.WIDE), float('nan'), device=dev)
  po = torch.full((n,), 3.0, device=dev)
  _cabi.dispatch_curves_fwd(wild, xs, out, prm, 16, po)
  _cabi.dispatch_curves_bwd(wild, xs, xs, dxo, prm, dpo, 16, po)
  torch.cuda.synchronize()
  assert float(out.float().abs().sum()) == 0 and float(dxo.float().abs().sum()) == 0
  assert float(dpo.abs().sum()) == 0 and float(po.abs().sum()) == 0
