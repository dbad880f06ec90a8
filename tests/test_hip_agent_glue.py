"""GPU: ``expo_agent_select_fwd / _bwd`` and ``expo_heads_regress_fwd / _bwd`` called through their bindings, against the
float64 reference of tests/_agent_glue_ref.py (the tolerances: four times the float32 restatement's own error, see there and
DESIGN.md section 7).  Every output buffer is filled with NaN before a call and must come back written in every element."""
import ctypes

import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from oracle import agent_np
from oracle import filters_np as fnp
from tests import _agent_glue_ref as R

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
UNWRITTEN = -12345  # no id


def _dev(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(shape, dev):
  return torch.full(shape, float('nan'), dtype=torch.float32, device=dev)


def _noise_tensor(noise, two_d, dev, seed=0):
  """(n, 131) with the draws in column 0, or the 1-D tensor (noise_stride 1)."""
  if not two_d:
    return _dev(noise.astype(f32), dev)
  z = np.random.default_rng(seed).random((len(noise), 131)).astype(f32)
  z[:, 0] = noise
  return _dev(z, dev)


def select_fwd(dev, logits, noise, states, progress, consts, is_train, two_d):
  n, k = logits.shape
  out = dict(pdf=_nan((n, k), dev), entropy=_nan((n,), dev),
             selected=torch.full((n,), UNWRITTEN, dtype=torch.int32, device=dev), onehot=_nan((n, k), dev),
             surrogate=_nan((n,), dev), new_states=_nan(tuple(states.shape), dev), penalty_base=_nan((n,), dev))
  _cabi.agent_select_fwd(_dev(logits, dev), _noise_tensor(noise, two_d, dev), _dev(states, dev),
                         torch.tensor([progress], dtype=torch.float32, device=dev), consts, is_train, out['pdf'], out['entropy'],
                         out['selected'], out['onehot'], out['surrogate'], out['new_states'], out['penalty_base'])
  return {name: v.cpu().numpy() for name, v in out.items()}


def select_bwd(dev, logits, selected, progress, consts, state_dim, d_surrogate, d_penalty_base):
  d_logits = _nan(tuple(logits.shape), dev)
  _cabi.agent_select_bwd(_dev(logits, dev), _dev(selected.astype(np.int32), dev),
                         torch.tensor([progress], dtype=torch.float32, device=dev), consts, state_dim, _dev(d_surrogate, dev),
                         _dev(d_penalty_base, dev), d_logits)
  return d_logits.cpu().numpy()


@pytest.mark.parametrize('k', R.SELECT_KS)
def test_selection_against_the_float64_reference(k, gpu_device):
  """Every (n, exploration, is_train) of ``select_cases``: pdf, entropy, surrogate, penalty_base and d_logits inside their
  error models, ids / onehot / new_states (trailing columns included) exactly, on every row."""
  worst = {}
  for c in R.select_cases(k):
    x = R.select_inputs(k, c['n'], c['eps'], c['seed'], c['trailing'])
    what = 'K %d n %d exploration %g is_train %d' % (k, c['n'], c['eps'], c['is_train'])
    ref = R.select_fwd(x['logits'], x['noise'], x['states'], c['progress'], c['consts'], c['is_train'])
    got = select_fwd(gpu_device, x['logits'], x['noise'], x['states'], c['progress'], c['consts'], c['is_train'], c['noise_2d'])
    assert (got['selected'] != UNWRITTEN).all(), what
    assert np.array_equal(got['selected'], ref['selected']), (what, np.flatnonzero(got['selected'] != ref['selected']))
    if c['is_train']:
      assert np.array_equal(got['selected'], x['target']) and got['selected'][0] == -1, what
      assert got['surrogate'][0] == 0 and (got['onehot'][0] == 0).all(), what
    elif c['n'] > 1:
      assert got['selected'][1] == 0, 'argmax of an all-equal row must be the first maximum'
    assert np.array_equal(got['onehot'], ref['onehot']), what
    assert np.array_equal(got['new_states'], ref['new_states']), what  # (NaN anywhere fails this)
    assert np.array_equal(got['new_states'][:, 3 + k:], x['states'][:, 3 + k:]), what
    checks = (('pdf', R.C_PDF, 0, 0), ('entropy', R.C_ENTROPY, R.C_ENTROPY, 1), ('surrogate', R.C_SURROGATE, R.C_SURROGATE, 1),
              ('penalty_base', 0, R.C_PENALTY, ref['penalty_scale']))
    for name, c_rel, c_abs, scale in checks:
      r = R.assert_close(got[name], ref[name], c_rel, c_abs, scale, what + ' ' + name)
      worst[name] = max(worst.get(name, 0.0), r)
    if c['eps'] == 1:
      assert np.abs(got['pdf'] - 1.0 / k).max() <= 1e-6 / k
    d_ref, scale = R.select_bwd(x['logits'], ref['selected'], c['progress'], c['consts'], x['d_surrogate'], x['d_penalty_base'])
    d_got = select_bwd(gpu_device, x['logits'], got['selected'], c['progress'], c['consts'], x['states'].shape[1],
                       x['d_surrogate'], x['d_penalty_base'])
    r = R.assert_close(d_got, d_ref, R.C_DLOGITS, R.C_DLOGITS, scale, what + ' d_logits')
    worst['d_logits'] = max(worst.get('d_logits', 0.0), r)
    if c['eps'] == 1 or k == 1:
      assert (d_got == 0).all(), what  # nothing reaches the logits through a uniform pdf
  print('K = %d: kernel, worst err / tol: %s' % (k, {name: '%.3f' % v for name, v in worst.items()}))


@pytest.mark.parametrize('k', R.SELECT_KS)
def test_sampled_ids_at_the_cdf_edges(k, gpu_device):
  """Noise exactly on an edge of the kernel's own cdf, one ulp above and one ulp below, for every edge 1 .. K-1: the ids are
  those of ``agent_np.pdf_sample`` in float32 on the kernel's pdf, bit for bit (strict comparison, correctly rounded division,
  the written association orders of the row sum and the scan); 1.0 and 1.5 give K - 1, 0 and NaN give -1."""
  n = 130
  consts = np.array([0.05, 0.05, 1.0, 1.0, 5], dtype=f32)
  clean_rows = 0
  for index, eps in enumerate(R.SELECT_EPS):
    consts[0] = eps
    x = R.select_inputs(k, n, eps, 77 * k + index, 0)
    two_d = index % 2 == 0
    run = lambda noise: select_fwd(gpu_device, x['logits'], noise.astype(f32), x['states'], 0.0, consts, 1, two_d)
    first = run(x['noise'])
    pdf = first['pdf']
    assert pdf.dtype == f32 and np.isfinite(pdf).all()
    cdf = agent_np.exclusive_cumsum(pdf / (agent_np.row_sum(pdf) + f32(1e-36)))
    assert cdf.dtype == f32
    rows = np.arange(n)
    if k > 1:
      j = 1 + rows % (k - 1)
      edge = cdf[rows, j]
      above, below = np.nextafter(edge, f32(np.inf)), np.nextafter(edge, f32(0))
      assert (above > edge).all() and (below < edge).all() and (edge > 0).all()
      before = cdf[rows, j - 1]
      after = np.where(j + 1 < k, cdf[rows, np.minimum(j + 1, k - 1)], f32(np.inf))
      for noise, clean, want in ((edge, before < edge, j - 1), (above, after > edge, j), (below, before < below, j - 1)):
        got = run(noise)
        assert np.array_equal(got['pdf'], pdf)
        assert np.array_equal(got['selected'], agent_np.pdf_sample(pdf, noise[:, None])), (eps, np.flatnonzero(
            got['selected'] != agent_np.pdf_sample(pdf, noise[:, None])))
        assert np.array_equal(got['selected'][clean], want[clean]), eps
        if eps > 0:  # every probability is at least exploration / K: no two edges coincide, every edge 1 .. K-1 is met
          assert clean.all() and set(j.tolist()) == set(range(1, k))
        clean_rows += int(clean.sum())
    special = np.array([1.0, 1.5, np.nan, 0.0], dtype=f32)[rows % 4]
    with np.errstate(invalid='ignore'):
      want = agent_np.pdf_sample(pdf, special[:, None])
    got = run(special)['selected']
    assert np.array_equal(got, want), eps
    assert (got[rows % 4 == 1] == k - 1).all() and (got[rows % 4 >= 2] == -1).all()
    if eps > 0 or k == 1:
      assert (got[rows % 4 == 0] == k - 1).all()
  assert k == 1 or clean_rows >= 3 * 3 * n


def _heads_run(dev, raws, ids, ranges, selected, dparams):
  n = raws[0].shape[0]
  traws = [_dev(r, dev) for r in raws]
  sel = _dev(selected, dev)
  params = _nan((n, R.MAX_PARAMS), dev)
  _cabi.heads_regress_fwd(traws, ids, ranges, sel, params)
  draws = [_nan(tuple(r.shape), dev) for r in raws]
  _cabi.heads_regress_bwd(traws, draws, ids, ranges, sel, _dev(dparams, dev))
  return params.cpu().numpy(), [d.cpu().numpy() for d in draws]


@pytest.mark.parametrize('ranges', [R.shipped_ranges(), R.biased_ranges()], ids=['shipped', 'biased'])
@pytest.mark.parametrize('heads', list(R.HEAD_LISTS))
def test_heads_against_the_float64_reference(heads, ranges, gpu_device):
  """params inside C_PARAMS (|ref| + 1), exactly 0 behind a filter's parameters and in the rows that selected nothing; d raw
  of every head inside C_DRAW x the sum of its absolute terms (the rounding count: ``heads_bwd``'s docstring), exactly 0
  outside the selected head's parameter slice and in the mask columns; everything finite at features of +-20, +-100, 0."""
  ids = R.HEAD_LISTS[heads]
  worst = dict(params=0.0, draw=0.0)
  for n in R.HEAD_NS:
    for mask_features in (6, 0):
      raws, selected, dparams = R.heads_inputs(ids, n, mask_features, 100 + n + mask_features)
      what = '%s n %d mask features %d' % (heads, n, mask_features)
      params, draws = _heads_run(gpu_device, raws, ids, ranges, selected, dparams)
      ref = R.heads_fwd(raws, ids, ranges, selected)
      worst['params'] = max(worst['params'], R.assert_close(params, ref, R.C_PARAMS, R.C_PARAMS, 1, what + ' params'))
      counts = np.array([fnp.NUM_PARAMS[ids[j]] if j >= 0 else 0 for j in selected])
      behind = np.arange(R.MAX_PARAMS)[None, :] >= counts[:, None]
      assert (params[behind] == 0).all(), what
      d_ref, scale = R.heads_bwd(raws, ids, ranges, selected, dparams)
      for j, fid in enumerate(ids):
        p = fnp.NUM_PARAMS[fid]
        r = R.assert_close(draws[j], d_ref[j], 0, R.C_DRAW, scale[j], what + ' d raw of head %d (filter %d)' % (j, fid))
        worst['draw'] = max(worst['draw'], r)
        assert (draws[j][selected != j] == 0).all() and (draws[j][:, p:] == 0).all(), (what, j)
        if fid == 2 and (selected == j).any():
          assert (dparams[selected == j, 0] != 0).all() and (draws[j][selected == j, 0] == 0).all()
  print('%s: kernel, worst err / tol: %s' % (heads, {name: '%.3f' % v for name, v in worst.items()}))


def test_bad_arguments_are_refused_before_anything_is_enqueued(gpu_device):
  lib = _cabi.load()
  dev = gpu_device
  bad, ok = -1, 0  # EXPO_E_BADARG, EXPO_OK
  n, k = 4, 8
  z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())
  logits, noise, states, progress = z(n, 16), z(n), z(n, 24), z(1)
  pdf, ent, onehot, sur, new_states, pen = z(n, 16), z(n), z(n, 16), z(n), z(n, 24), z(n)
  sel = torch.zeros(n, dtype=torch.int32, device=dev)
  consts = (ctypes.c_float * 5)(0.05, 0.05, 1.0, 1.0, 5.0)
  torch.cuda.synchronize()

  def fwd(k=k, state_dim=3 + k, stride=1, n=n):
    return lib.expo_agent_select_fwd(ptr(logits), ptr(noise), stride, ptr(states), ptr(progress), consts, k, state_dim, 1, ptr(pdf),
                                     ptr(ent), ptr(sel), ptr(onehot), ptr(sur), ptr(new_states), ptr(pen), n, None)

  def bwd(k=k, state_dim=3 + k, n=n):
    return lib.expo_agent_select_bwd(ptr(logits), ptr(sel), ptr(progress), consts, k, state_dim, ptr(sur), ptr(pen), ptr(pdf), n, None)

  assert fwd(k=0, state_dim=24) == bad and fwd(k=17, state_dim=24) == bad and bwd(k=0, state_dim=24) == bad and bwd(k=17, state_dim=24) == bad
  assert fwd(state_dim=2 + k) == bad and bwd(state_dim=2 + k) == bad
  assert fwd(stride=0) == bad and fwd(stride=-1) == bad
  assert fwd(n=-1) == bad and bwd(n=-1) == bad
  assert fwd(n=0) == ok and bwd(n=0) == ok

  raws = [z(n, 32) for _ in range(17)]
  draws = [z(n, 32) for _ in range(17)]
  params = z(n, R.MAX_PARAMS)
  rng = (ctypes.c_float * 9)(*[float(v) for v in R.shipped_ranges()])

  def heads(count, abi=None, widths=None, n=n, back=False):
    m = max(count, 1)
    abi = abi or [0] * m
    widths = widths or [32] * m
    r = (ctypes.c_void_p * m)(*[ptr(t) for t in raws[:m]])
    d = (ctypes.c_void_p * m)(*[ptr(t) for t in draws[:m]])
    w, a = (ctypes.c_int * m)(*widths), (ctypes.c_int * m)(*abi)
    if back:
      return lib.expo_heads_regress_bwd(r, d, w, a, count, rng, ptr(sel), ptr(params), n, None)
    return lib.expo_heads_regress_fwd(r, w, a, count, rng, ptr(sel), ptr(params), n, None)

  for back in (False, True):
    assert heads(0, back=back) == bad and heads(17, back=back) == bad
    assert heads(2, abi=[0, 9], back=back) == bad and heads(2, abi=[-1, 0], back=back) == bad
    assert heads(2, abi=[0, 7], widths=[1, 23], back=back) == bad  # the colour curve has 24 parameters
    assert heads(2, abi=[4, 2], widths=[8, 2], back=back) == bad
    assert heads(2, n=-1, back=back) == bad
    assert heads(2, abi=[0, 7], widths=[1, 24], n=0, back=back) == ok
  torch.cuda.synchronize()
  for t in (pdf, ent, onehot, sur, new_states, pen, params) + tuple(draws):
    assert float(t.abs().sum()) == 0  # nothing ran
  assert b'' != lib.expo_last_error()
