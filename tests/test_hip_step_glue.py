"""GPU: the training step's loss-glue kernels -- ``expo_gp_inputs / _rows``, ``expo_grad_penalty_fwd / _bwd``,
``expo_planes_concat``, ``expo_generator_losses``, ``expo_critic_head_fwd / _bwd``, ``expo_critic_report``,
``expo_plane_sums``, ``expo_gp_direct`` -- called through their bindings against the float64 reference of
tests/_step_glue_ref.py (the tolerances: four times the float32 restatement's own error, see there and DESIGN.md section
7.3).  Every output buffer is NaN before a call and has 64 guard elements behind it that must come back untouched."""
import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from tests import _step_glue_ref as R

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
GUARD_VALUE = -777.0


def _dev(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Outputs:
  """NaN-filled float32 output tensors, each a view of a buffer with ``R.GUARD`` more elements behind it."""

  def __init__(self, dev):
    self.dev, self.buffers = dev, []

  def new(self, *shape):
    count = int(np.prod(shape))
    buf = torch.full((count + R.GUARD,), float('nan'), dtype=torch.float32, device=self.dev)
    buf[count:] = GUARD_VALUE
    self.buffers.append((buf, count))
    return buf[:count].view(shape)

  def guards_untouched(self, what):
    for buf, count in self.buffers:
      assert bool((buf[count:] == GUARD_VALUE).all()), what + ': wrote behind an output'


def _merge(worst, new):
  for k, v in new.items():
    worst[k] = max(worst.get(k, 0.0), v)


def _show(what, worst):
  print('%s: kernel, worst err / tol: %s' % (what, {k: '%.3f' % v for k, v in worst.items()}))


# ---- expo_gp_inputs / expo_gp_inputs_rows -----------------------------------------------------------------------------
def _gp_inputs(dev, real, fake, alpha, real_rows=None, fake_rows=None, what=''):
  out = Outputs(dev)
  n = len(real) if real_rows is None else len(real_rows)
  cat = out.new(*((2 * n,) + real.shape[1:]))
  interp = out.new(*((n,) + real.shape[1:])) if alpha is not None else None
  rows = lambda r: None if r is None else _dev(r, dev)
  _cabi.gp_inputs(_dev(real, dev), _dev(fake, dev), None if alpha is None else _dev(alpha, dev), cat, interp,
                  real_rows=rows(real_rows), fake_rows=rows(fake_rows))
  torch.cuda.synchronize()
  out.guards_untouched(what)
  return cat.cpu().numpy(), None if interp is None else interp.cpu().numpy()


@pytest.mark.parametrize('np_dtype', [np.float16, f32], ids=['fp16', 'fp32'])
def test_gp_inputs_against_the_float64_reference(np_dtype, gpu_device):
  """Five image sizes, two of them past the 64-block cap (the grid-stride loop), with and without interp; the row variants
  on 7 x 5 images.  cat_out bit-equal to the float conversion, interp inside C_INTERP x its absolute terms."""
  worst = 0.0
  for shape in R.GP_SHAPES:
    real, fake, alpha = R.gp_case(shape, np_dtype, len(shape) + shape[1])
    what = 'gp_inputs %s' % (shape,)
    ref_cat, ref, scale = R.gp_inputs(real, fake, alpha)
    cat, interp = _gp_inputs(gpu_device, real, fake, alpha, what=what)
    assert np.array_equal(cat, ref_cat), what
    worst = max(worst, R.check_interp(interp, ref, scale, what))
    cat, interp = _gp_inputs(gpu_device, real, fake, None, what=what)
    assert interp is None and np.array_equal(cat, ref_cat), what + ' without interp'
  for name, real, real_rows, fake, fake_rows, alpha in R.gp_row_cases(np_dtype, 5):
    ref_cat, ref, scale = R.gp_inputs(real, fake, alpha, real_rows, fake_rows)
    cat, interp = _gp_inputs(gpu_device, real, fake, alpha, real_rows, fake_rows, what=name)
    assert np.array_equal(cat, ref_cat), name
    worst = max(worst, R.check_interp(interp, ref, scale, name))
    cat, interp = _gp_inputs(gpu_device, real, fake, None, real_rows, fake_rows, what=name)
    assert np.array_equal(cat, ref_cat), name + ' without interp'
  _show('gp_inputs', dict(interp=worst))


# ---- expo_grad_penalty_fwd / _bwd -------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', R.PEN_ELEMS)
def test_grad_penalty_against_the_float64_reference(m, gpu_device):
  """Seven images per size: all zero, norm 1 - 1e-3, 1 + 1e-3, 0.5, 3 (twice), 1.7; dterm of both signs and 0."""
  dev = gpu_device
  g, dterm = R.penalty_images(m, m)
  n = len(g)
  out = Outputs(dev)
  norm, term, dg = out.new(n), out.new(n), out.new(n, m)
  gt = _dev(g, dev)
  _cabi.grad_penalty_fwd(gt, norm, term)
  ref_norm, ref_term = R.penalty_fwd(g)
  norm_np, term_np = norm.cpu().numpy(), term.cpu().numpy()
  worst = R.check_penalty_fwd(norm_np, term_np, ref_norm, ref_term, 'm = %d' % m)
  assert norm_np[0] == np.sqrt(f32(1e-6)) and term_np[0] == 0, 'the all-zero image'
  assert (term_np[[1, 3]] == 0).all() and (term_np[[2, 4, 5, 6]] > 0).all()
  _cabi.grad_penalty_bwd(gt, norm, _dev(dterm, dev), dg)
  torch.cuda.synchronize()
  out.guards_untouched('m = %d' % m)
  dg_np = dg.cpu().numpy()
  worst['dg'] = R.check_dg(dg_np, R.penalty_bwd(g, norm_np, dterm), 'm = %d' % m)
  assert (dg_np[[0, 1, 3, 5]] == 0).all(), 'below the kink, the all-zero image and dterm = 0: exactly 0'
  assert (np.sign(dg_np[4]) == -np.sign(g[4])).all() and (np.sign(dg_np[6]) == np.sign(g[6])).all()
  _show('grad_penalty m = %d' % m, worst)


# ---- expo_planes_concat -----------------------------------------------------------------------------------------------
def _concat(dev, img, vec, what):
  out = Outputs(dev)
  v = 0 if vec is None else vec.shape[1]
  o = out.new(*(img.shape[:-1] + (3 + v,)))
  _cabi.planes_concat(_dev(img, dev), None if vec is None else _dev(vec, dev), o, 0.5)
  torch.cuda.synchronize()
  out.guards_untouched(what)
  return o.cpu().numpy()


@pytest.mark.parametrize('np_dtype', [np.float16, f32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('v', R.CONCAT_VS)
def test_planes_concat_bit_equal(v, np_dtype, gpu_device):
  """1 .. 4096 pixels (less than a block, 255 / 256 / 257, several blocks) x v planes: every element one float32 rounding of
  the formula.  v = 1 also at 513 x 512 pixels: 1027 blocks capped to 1024, blocks 0 and 1 on a second trip."""
  shapes = R.CONCAT_SHAPES + ((R.CONCAT_BIG,) if v == 1 else ())
  for shape in shapes:
    img, vec = R.concat_case(shape, v, np_dtype, v + shape[1])
    what = 'planes_concat %s v %d' % (shape, v)
    got = _concat(gpu_device, img, vec, what)
    want = R.planes_concat(img, vec, 0.5)
    assert got.dtype == f32
    R.check_bit_equal(got, want, what)


def test_planes_concat_refuses_62_planes(gpu_device):
  img, vec = R.concat_case((1, 2, 2), 62, f32, 0)
  out = Outputs(gpu_device)
  o = out.new(1, 2, 2, 65)
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.planes_concat(_dev(img, gpu_device), _dev(vec, gpu_device), o, 0.5)
  torch.cuda.synchronize()
  assert bool(torch.isnan(o).all())
  out.guards_untouched('62 planes')


# ---- expo_generator_losses --------------------------------------------------------------------------------------------
def _generator(dev, x, use_td, use_penalty, counters, what):
  n = len(x['fake_logit'])
  out = Outputs(dev)
  losses, reward, q, coef = out.new(2), out.new(n), out.new(n), out.new(5, n)
  steps = [torch.full((1,), start, dtype=torch.float32, device=dev) if on else None for on, start in zip(counters, (3.0, 41.0))]
  t = {k: _dev(v, dev) for k, v in x.items()}
  _cabi.generator_losses(t['fake_logit'], t['fake_input_logit'], t['new_value'], t['old_value'], t['new_states'],
                         t['penalty'] if use_penalty else None, t['surrogate'], [float(c) for c in R.GEN_CONSTS], use_td,
                         losses, reward, q, coef, adam_steps=tuple(steps))
  torch.cuda.synchronize()
  out.guards_untouched(what)
  for s, start in zip(steps, (3.0, 41.0)):
    assert s is None or float(s) == start + 1.0, what + ': an Adam counter advances by exactly 1'
  return dict(losses=losses.cpu().numpy(), reward=reward.cpu().numpy(), q=q.cpu().numpy(), coef=coef.cpu().numpy())


@pytest.mark.parametrize('n', R.GEN_NS)
def test_generator_losses_against_the_float64_reference(n, gpu_device):
  """use_td x penalty, state_dim 3 and 11, steps max_len - 1 / max_len / max_len + 1 x stopped 0 / 1, both Adam counters, one,
  none: reward, q, all five coef rows (those that must be 0 exactly 0) and the two losses."""
  worst = {}
  for i, (use_td, use_penalty) in enumerate(((1, 1), (1, 0), (0, 1), (0, 0))):
    x = R.gen_inputs(n, (3, 11)[i % 2], 10 * n + i)
    counters = ((True, True), (True, False), (False, True), (False, False))[i]
    what = 'n %d use_td %d penalty %d' % (n, use_td, use_penalty)
    got = _generator(gpu_device, x, use_td, use_penalty, counters, what)
    ref = R.generator_losses(x, R.GEN_CONSTS, use_td, use_penalty)
    _merge(worst, R.check_generator(got, ref, what))
    if not use_td:
      assert (got['coef'][1] == 0).all(), what
    if not use_penalty:
      assert (got['coef'][3] == 0).all(), what
    past = x['new_states'][:, 2] > R.GEN_CONSTS[4]
    if use_td:
      assert (got['coef'][1][past] == 0).all() and (got['coef'][1][x['new_states'][:, 1] == 1] == 0).all(), what
  _show('generator_losses n = %d' % n, worst)


# ---- expo_critic_head_fwd / _bwd --------------------------------------------------------------------------------------
def _head_fwd(dev, hpre, b1, w2, b2, rows, inv_n, what):
  m, hidden = hpre.shape[-2:]
  out = Outputs(dev)
  logits, h, dh = out.new(m), out.new(m, hidden), out.new(m, hidden)
  hp = _dev(hpre[0] if b1 is None else hpre, dev)
  _cabi.critic_head_fwd(hp, _dev(w2, dev), _dev(b2, dev), rows[0], rows[1], rows[2], inv_n, logits, h, dh,
                        float(R.LEAK), None if b1 is None else _dev(b1, dev))
  torch.cuda.synchronize()
  out.guards_untouched(what)
  return dict(logits=logits.cpu().numpy(), h=h.cpu().numpy(), dh=dh.cpu().numpy())


def _head_bwd(dev, dh, h, thpre, rows, inv_n, what):
  hidden = h.shape[1]
  out = Outputs(dev)
  gb1, gw2, gb2 = out.new(hidden), out.new(hidden), out.new(1)
  _cabi.critic_head_bwd(_dev(dh, dev), _dev(h, dev), None if thpre is None else _dev(thpre, dev), rows[0], rows[1], rows[2],
                        inv_n, gb1, gw2, gb2, float(R.LEAK))
  torch.cuda.synchronize()
  out.guards_untouched(what)
  return dict(gb1=gb1.cpu().numpy(), gw2=gw2.cpu().numpy(), gb2=gb2.cpu().numpy())


@pytest.mark.parametrize('hidden', R.HEAD_HIDDEN)
def test_critic_head_fwd_against_the_float64_reference(hidden, gpu_device):
  """Every row case with one slab (no b1) and with 2 .. 64 slabs and b1; pre-activations of exactly 0 and -0.0 (slope
  0.6).  h bit-equal to the float32 restatement, logits and dh inside their bounds."""
  worst = {}
  for i, (rows, slabs, _) in enumerate(R.head_cases(hidden)):
    inv_n = 1.0 / max(rows[0], 1)
    hpre, b1, w2, b2 = R.head_inputs(rows, hidden, slabs, 100 * hidden + i)
    what = 'hidden %d rows %s slabs %d' % (hidden, rows, slabs)
    got = _head_fwd(gpu_device, hpre, b1, w2, b2, rows, inv_n, what)
    ref, r32 = R.head_fwd(hpre, b1, w2, b2, rows, inv_n), R.head_fwd(hpre, b1, w2, b2, rows, inv_n, dtype=f32)
    _merge(worst, R.check_head_fwd(got, ref, r32, what))
    zero = ref['h'] == 0
    want = (f32(0.5) * (f32(1) + R.LEAK)) * (R.row_signs(rows, inv_n, f32)[:, None] * w2[None, :])
    assert zero.any() or hidden * sum(rows) < 20
    assert np.array_equal(got['dh'][zero], want[zero]), what + ': a pre-activation of exactly 0 takes slope 0.6'
  _show('critic_head_fwd hidden = %d' % hidden, worst)


def test_critic_head_refuses_65_slabs(gpu_device):
  dev = gpu_device
  out = Outputs(dev)
  logits, h, dh, gb1, gw2, gb2 = out.new(3), out.new(3, 16), out.new(3, 16), out.new(16), out.new(16), out.new(1)
  z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.critic_head_fwd(z(65, 3, 16), z(16), z(1), 1, 1, 1, 1.0, logits, h, dh, 0.2, z(16))
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.critic_head_bwd(z(3, 16), z(3, 16), z(65, 1, 16), 1, 1, 1, 1.0, gb1, gw2, gb2, 0.2)
  torch.cuda.synchronize()
  for t in (logits, h, dh, gb1, gw2, gb2):
    assert bool(torch.isnan(t).all())
  out.guards_untouched('65 slabs')


@pytest.mark.parametrize('hidden', R.HEAD_HIDDEN)
def test_critic_head_bwd_against_the_float64_reference(hidden, gpu_device):
  """The same rows with 1 / 9 / 64 tangent slabs: gb1 bit-equal to the float32 restatement in the kernel's order (additions
  only, in a fixed order) and inside its bound, gw2 and gb2 inside theirs."""
  worst = {}
  for i, (rows, _, th_slabs) in enumerate(R.head_cases(hidden)):
    inv_n = 1.0 / max(rows[0], 1)
    dh, h, thpre = R.bwd_inputs(rows, hidden, th_slabs, 100 * hidden + i)
    what = 'hidden %d rows %s th_slabs %d' % (hidden, rows, th_slabs)
    got = _head_bwd(gpu_device, dh, h, thpre, rows, inv_n, what)
    ref, r32 = R.head_bwd(dh, h, thpre, rows, inv_n), R.head_bwd(dh, h, thpre, rows, inv_n, dtype=f32)
    _merge(worst, R.check_head_bwd(got, ref, r32, what))
  _show('critic_head_bwd hidden = %d' % hidden, worst)


@pytest.mark.parametrize('n', R.PAIRED_NS)
def test_gb1_is_exactly_zero_where_paired_rows_share_their_slopes(n, gpu_device):
  """What critic_head_bwd_kernel's comment promises: n real rows and n fake rows with pairwise equal slopes (1, 0.2 and the
  0.6 of an exact zero) give gb1 == 0.0 in every unit, for every row count; with one pair of one unit made to differ that
  unit is non-zero and the others stay 0.  Where each row group holds one row per side (n a power of two up to 64) the sum
  is also bit for bit what the order 'a group's real rows, then its fake rows' gives on a dh where nothing cancels."""
  hidden = 128
  rows = (n, n, 0)
  dh, h, inv_n = R.paired_inputs(n, hidden, n)
  got = _head_bwd(gpu_device, dh, h, None, rows, inv_n, 'paired n = %d' % n)
  nonzero = int((got['gb1'] != 0).sum())
  print('n = %d: non-zero gb1 units of %d: %d' % (n, hidden, nonzero))
  assert nonzero == 0 and np.isfinite(got['gb1']).all(), 'n = %d: %d of %d units of gb1 are not exactly 0' % (n, nonzero, hidden)
  unit = 37
  dh, h, inv_n = R.paired_inputs(n, hidden, n, odd_unit=unit)
  got = _head_bwd(gpu_device, dh, h, None, rows, inv_n, 'paired n = %d, one unit odd' % n)
  assert got['gb1'][unit] != 0 and (np.delete(got['gb1'], unit) == 0).all()
  if n <= 64 and n & (n - 1) == 0:
    dh, h, _ = R.bwd_inputs(rows, hidden, 1, n)
    got = _head_bwd(gpu_device, dh, h, None, rows, inv_n, 'general n = %d' % n)
    assert np.array_equal(got['gb1'], R.head_bwd(dh, h, None, rows, inv_n, dtype=f32, order='parent')['gb1'])


# ---- expo_critic_report -----------------------------------------------------------------------------------------------
def test_critic_report_against_the_float64_reference(gpu_device):
  """Rows up to (130, 130, 70) (the 64-lane stride), empty blocks, n_interp = 0; ema and adam_step given and absent."""
  dev = gpu_device
  worst = {}
  for i, rows in enumerate(R.REPORT_ROWS):
    logits, norm, term = R.report_inputs(rows, i)
    ref = R.critic_report(logits, norm, term, rows, 10.0, 0.99, 0.25)
    for with_ema, with_step in ((True, True), (True, False), (False, True), (False, False)):
      what = 'rows %s ema %d step %d' % (rows, with_ema, with_step)
      out = Outputs(dev)
      rep, ema = out.new(5), out.new(1)
      ema[0] = 0.25
      step = torch.full((1,), 6.0, dtype=torch.float32, device=dev) if with_step else None
      _cabi.critic_report(_dev(logits, dev), _dev(norm, dev), _dev(term, dev), rows[0], rows[1], rows[2], 10.0, rep,
                          ema if with_ema else None, 0.99, adam_step=step)
      torch.cuda.synchronize()
      out.guards_untouched(what)
      assert step is None or float(step) == 7.0, what
      ema_np = ema.cpu().numpy()[0]
      if with_ema:
        _merge(worst, R.check_report(rep.cpu().numpy(), ema_np, ref, what))
      else:
        assert ema_np == f32(0.25), what
        _merge(worst, dict(out=R.assert_within(rep.cpu().numpy(), ref[0], R.C_REPORT * ref[2], what)))
      if rows[2] == 0:
        assert (rep.cpu().numpy()[[2, 3]] == 0).all(), what
  _show('critic_report', worst)


# ---- expo_plane_sums / expo_gp_direct ---------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', R.SUM_PIXELS, ids=lambda hw: '%dpx' % (hw[0] * hw[1]))
def test_plane_sums_and_gp_direct_against_the_float64_reference(hw, gpu_device):
  """1 .. 5760 pixels (fewer than threads, 1023 / 1024 / 1025, several trips) x 1 / 3 / 14 / 16 planes from channel 0 or 3;
  gp_direct with 3, 6 and 17 input channels on the all-zero (u = -ds), below-1, near-1 and above-1 images."""
  dev = gpu_device
  i = R.SUM_PIXELS.index(hw)
  worst = {}
  for planes in R.SUM_PLANES:
    first = (0, 3)[(i + planes) % 2]
    x = (0.02 * np.random.default_rng(planes + i).standard_normal((3,) + hw + (first + planes,))).astype(f32)
    what = 'plane_sums %s planes %d first %d' % (hw, planes, first)
    out = Outputs(dev)
    sums = out.new(3, planes)
    _cabi.plane_sums(_dev(x, dev), sums, first)
    torch.cuda.synchronize()
    out.guards_untouched(what)
    _merge(worst, dict(plane=R.check_plane_sums(sums.cpu().numpy(), R.plane_sums(x, first), what)))
  for c in (3, 6, 17):
    u, ds = R.gp_direct_inputs(hw, c, 7 * i + c)
    n = len(u)
    what = 'gp_direct %s u_channels %d' % (hw, c)
    out = Outputs(dev)
    v, norm, term = out.new(*ds.shape), out.new(n), out.new(n)
    _cabi.gp_direct(_dev(u, dev), _dev(ds, dev), 0.37, v, norm, term)
    torch.cuda.synchronize()
    out.guards_untouched(what)
    got = dict(v=v.cpu().numpy(), norm=norm.cpu().numpy(), term=term.cpu().numpy())
    _merge(worst, R.check_gp_direct(got, R.gp_direct(u, ds, 0.37), 0.37, what))
    assert got['norm'][0] == np.sqrt(f32(1e-6)) and got['term'][0] == 0, what
    assert (got['v'][[0, 1, 3]] == 0).all() and (got['term'][[1, 3]] == 0).all() and (got['term'][[2, 4, 5, 6]] > 0).all(), what
  _show('plane_sums / gp_direct %s' % (hw,), worst)


def test_plane_sums_refuses_17_planes(gpu_device):
  out = Outputs(gpu_device)
  sums = out.new(2, 17)
  x = torch.zeros((2, 3, 3, 17), dtype=torch.float32, device=gpu_device)
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.plane_sums(x, sums, 0)
  torch.cuda.synchronize()
  assert bool(torch.isnan(sums).all())
  out.guards_untouched('17 planes')
