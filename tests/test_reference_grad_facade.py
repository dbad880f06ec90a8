"""GRADIENT COMPOSITION PIN (TF primitive gradients assumed and listed): the fixture tests/golden/reference_grad_facade.npz
holds what torch autograd computes when it back-propagates through the BODIES of the reference's TensorFlow methods,
executed in the build container with a torch float64 stand-in in place of `tf` (tests/golden/make_reference_grad_facade.py:
`process` / `filter_param_regressor` of the eight filters and LevelFilter, Filter.get_mask and filters.py:88, util.py's
helpers, pdf_sample, agent.py:100-123, 208-252).  The forward sibling is tests/test_reference_facade.py; both fixtures
are cut from the same text (same sha256).  Held against it:

  CPU  dx / dparams of oracle/filters_np.py (hand-derived), oracle/filters_torch.py (autograd over the build's own
       transcription) and oracle/filters_c.py at 8 steps, Tone / Color at cfg.curve_steps 1, 3, 5, 16, the analytic HSV
       mode on smooth pixels, the masked apply; dfeatures of the product regressors and of _agent_glue_ref.heads_bwd;
       d_logits of _agent_glue_ref.select_bwd; lrelu'(0).  Tolerance |err| <= 1e-10 max|ref| per array (C oracle 1e-9,
       where float32 constants enter 1e-6); nothing is excluded, the tie pixels are the point.  Four MUTANTS (exclusive
       clip, exclusive Gamma floor, exclusive luminance clamp, no entropy / no white-balance cross term) must FAIL the
       same assertions.
  GPU  every backward kernel the fixture reaches, fp32 storage, tests/_tol.py's bounds unchanged.

It pins how the hand-derived backward code COMPOSES the primitive gradients -- not the primitive gradients (the stand-in's
maximum / minimum / clip / abs rules are TF's as READ by this build, written down in the generator and listed in the
fixture), and the `hsv1_` arrays pin only the composition around THE BUILD'S statement of TF's HSV formulas.

Ties under fp32.  0, 1, (0, 0, 0) and the knots of a power-of-two step count are exact in fp32 and the kernels must follow
the fixture there.  Two constructed ties have a side that depends on the precision (lum of (1, 1, 1) against 1.0, x = 0.001
against the float32 0.001): there the comparison against the FIXTURE skips dx where the float64 oracle on the kernel's
own fp32 inputs and the fixture differ, at most 4 of 720 pixels per filter, every one a constructed pixel; the kernel is
still held to the same-input oracle there.  A THIRD family was found in writing this test: the knots i / L of a step count
that is no power of two (L = 3, 5), x = 1.0 included.  `x - (L - 1) / L <= 1 / L` at x = 1 is decided by rounding in
EVERY precision (float64 gives NO gradient at x = 1.0, L = 3; the reference's float32 graph gives one; at x = 3/5 float32
drops the lower segment and float64 keeps it), so the fixture, the same-input oracle and the reference's own float32
arithmetic disagree with each other there.  At those L constructed pixels per case the kernel's dx must equal one of the
sub-gradients an inclusive clip can give: dy (L / S) (k_i [+ k_(i-1)]), i < L; dy (L / S) k_(L-1) or 0 at i = L.
(tests/test_hip_curve_dispatch.py masks such elements out altogether.)  dparams are never skipped."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import filters_np as fnp
from oracle import filters_torch as ft
from oracle import nets_np
from tests import _agent_glue_ref as R
from tests._tol import assert_image_close, assert_param_grad_close, image_tol, param_grad_tol

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FILTERS = ['ExposureFilter', 'GammaFilter', 'ImprovedWhiteBalanceFilter', 'SaturationPlusFilter', 'ToneFilter',
           'ContrastFilter', 'WNBFilter', 'ColorFilter', 'LevelFilter']  # C-ABI ids 0 .. 8
MASKED = [0, 3, 5, 7]  # case C: E, S+, Ct, C
CURVE_STEPS = (1, 3, 5, 16)  # case B
KNOT_FIRST = 20  # case B: pixels 20 .. 20 + L of image 0 hold the knots 0 / L .. L / L
# the constructed pixels (image, row, column) whose side of a tie depends on the precision: (1, 1, 1) and 0.001
PRECISION_TIES = {(0, 1, 1), (0, 1, 2)}
SHARP, MIN_STRENGTH = 1.0, 0.3
f32, f64 = np.float32, np.float64


@pytest.fixture(scope='module')
def fwd():
  return np.load(os.path.join(HERE, 'reference_facade.npz'))


@pytest.fixture(scope='module')
def g():
  return np.load(os.path.join(HERE, 'reference_grad_facade.npz'))


def packed_params(fwd, fid):
  p = fwd[FILTERS[fid] + '_params']
  return p.reshape(p.shape[0], -1)


def x_of_case_b(fwd, g, L):
  x = fwd['x'].copy()
  x[0].reshape(-1, 3)[KNOT_FIRST:KNOT_FIRST + L + 1, :] = g['B_L%d_knots' % L][:, None]
  return x


def gap(got, want, scale=None):
  """max |err| / max |ref| of one array (or / `scale` where the array is analytically zero)."""
  got, want = np.asarray(got, dtype=f64), np.asarray(want, dtype=f64)
  assert got.shape == want.shape, (got.shape, want.shape)
  return float(np.abs(got - want).max() / (max(np.abs(want).max(), 1e-300) if scale is None else scale))


def assert_gap(got, want, bound, what, scale=None):
  r = gap(got, want, scale)
  assert r <= bound, '%s: max |err| / max |ref| = %.3g > %.1g' % (what, r, bound)
  return r


def check_filter_grads(backward, g, prefix, x, packed, bound, what, smooth=None, dp_scale=None):
  """`backward(x, packed, dy) -> (dx, dparams)` against the fixture's arrays `prefix_dx`, `prefix_dparams`."""
  dx, dp = backward(x, packed, g['dy'])
  dx, want = np.asarray(dx), g[prefix + '_dx']
  if smooth is not None:
    dx, want = dx[smooth], want[smooth]
  return max(assert_gap(dx, want, bound, what + ' dx'), assert_gap(np.asarray(dp), g[prefix + '_dparams'], bound, what + ' dparams', dp_scale))


def via_torch(fid, mode=0):

  def backward(x, packed, dy):
    dx, dp = ft.backward_packed(fid, torch.from_numpy(x), torch.from_numpy(np.ascontiguousarray(packed)), torch.from_numpy(dy), mode)
    return dx.numpy(), dp.numpy()

  return backward


# ---- provenance ------------------------------------------------------------------------------------------------------------
def test_fixture_names_its_sources_its_stand_ins_and_its_rewrites(fwd, g):
  prov = [str(p) for p in g['provenance']]
  assert [p.split(' ')[0] for p in prov] == ['util.py', 'filters.py', 'pdf_sample_layer.py', 'agent.py']
  assert all(len(p.split('sha256=')[1]) == 64 for p in prov)
  assert prov == [str(p) for p in fwd['provenance']], 'the two fixtures were cut from different texts'
  common = {'argmax', 'cast', 'concat', 'constant', 'cos', 'cumsum', 'exp', 'less', 'log', 'nn.softmax', 'one_hot', 'pow',
            'reduce_mean', 'reduce_sum', 'reshape', 'sigmoid', 'tanh', 'abs [sign(x), 0 at 0]',
            'clip_by_value [minimum(maximum(x, lo), hi): passes on lo <= x <= hi]',
            'maximum [scalar: gradient to x where x >= c]', 'minimum [scalar: gradient to x where x <= c]'}
  hsv0 = {'image.rgb_to_hsv [NumPy facade on detached values: a constant (TF-1: not differentiable)]',
          'image.hsv_to_rgb [NumPy facade on detached values: a constant (TF-1: not differentiable)]',
          'maximum [two tensors, no gradient]'}
  assert set(str(o) for o in g['standin_ops']) == common | hsv0
  # the second stand-in ran SaturationPlus alone
  assert set(str(o) for o in g['standin_ops_hsv1']) == {
      'image.rgb_to_hsv [TF formula in differentiable torch ops: hsv_grad_mode 1]',
      'image.hsv_to_rgb [TF formula in differentiable torch ops: hsv_grad_mode 1]', 'abs [sign(x), 0 at 0]', 'concat', 'sigmoid',
      'minimum [scalar: gradient to x where x <= c]'}
  rewrites = [str(r) for r in g['rewrites']]
  assert [r.split(':')[0] for r in rewrites] == ['np.array -> float64 tensor', 'AugAssign -> Assign', 'builtin abs -> the stand-in']
  assert set(str(s) for s in g['pen_is_plain']) == {'A_SaturationPlusFilter', 'A_ToneFilter', 'A_ColorFilter', 'A_LevelFilter',
                                                   'B_L5_ToneFilter', 'B_L5_ColorFilter', 'B_L16_ToneFilter', 'B_L16_ColorFilter'}
  assert int(g['hsv1_non_smooth_count']) == int((~g['hsv1_smooth']).sum()) <= 24
  for L in CURVE_STEPS:
    assert np.array_equal(g['B_L%d_knots' % L], np.arange(L + 1) / float(L))
  for a in (g['agent_g_s'], g['agent_g_q'], g['dpen']):  # what the kernels are handed must be exact in fp32
    assert np.array_equal(a, a.astype(f32).astype(f64))


# ---- filter gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fid', range(9))
def test_numpy_and_torch_oracles_backpropagate_like_the_reference(fwd, g, fid):
  """Case A: all nine filters at 8 steps, on the forward fixture's x (knots, 0.001, lum 0 / 1, negative channels)."""
  name = FILTERS[fid]
  x, packed = fwd['x'], packed_params(fwd, fid)
  r_np = check_filter_grads(lambda *a: fnp.backward_packed(fid, *a), g, 'A_' + name, x, packed, 1e-10, name + ' (NumPy oracle)')
  r_t = check_filter_grads(via_torch(fid), g, 'A_' + name, x, packed, 1e-10, name + ' (torch oracle)')
  print('GRADPIN cpu A %s: NumPy %.2e torch %.2e (bound 1e-10)' % (name, r_np, r_t))


def test_oracles_backpropagate_contrast_with_a_live_parameter_at_the_luminance_tie(fwd, g):
  """Case A2: Contrast with param tanh(0.75) in image 0, whose pixel (1, 1, 1) has luminance exactly 1.0 in float64."""
  from oracle import filters_c as fc
  x, packed = fwd['x'], g['A2_ContrastFilter_params']
  assert fnp.rgb2lum(x)[0, 1, 1, 0] == 1.0 and packed[0, 0] == np.tanh(0.75)
  assert_gap(fnp.regress_packed(5, g['A2_ContrastFilter_features']), packed, 1e-13, 'regressor')
  check_filter_grads(lambda *a: fnp.backward_packed(5, *a), g, 'A2_ContrastFilter', x, packed, 1e-10, 'Contrast A2 (NumPy oracle)')
  check_filter_grads(via_torch(5), g, 'A2_ContrastFilter', x, packed, 1e-10, 'Contrast A2 (torch oracle)')
  check_filter_grads(lambda *a: fc.backward_packed(5, *a), g, 'A2_ContrastFilter', x, packed, 1e-9, 'Contrast A2 (C oracle)')


@pytest.mark.parametrize('fid', range(8))
def test_c_oracle_backpropagates_like_the_reference(fwd, g, fid):
  from oracle import filters_c as fc
  name = FILTERS[fid]
  r = check_filter_grads(lambda *a: fc.backward_packed(fid, *a), g, 'A_' + name, fwd['x'], packed_params(fwd, fid), 1e-9,
                         name + ' (C oracle)')
  print('GRADPIN cpu A %s: C %.2e (bound 1e-9)' % (name, r))


@pytest.mark.parametrize('fid', [4, 7])
@pytest.mark.parametrize('L', CURVE_STEPS)
def test_oracles_backpropagate_curves_of_any_step_count_like_the_reference(fwd, g, L, fid):
  """Case B: x on every knot i / L (exact for L = 1, 16; the float64 nearest for 3, 5)."""
  prefix = 'B_L%d_%s' % (L, FILTERS[fid])
  x, packed = x_of_case_b(fwd, g, L), g[prefix + '_params']
  cfg = dict(fnp.DEFAULT_CFG, curve_steps=L)
  assert_gap(fnp.regress_packed(fid, g[prefix + '_features'], cfg), packed, 1e-13, prefix + ' regressor')
  assert_gap(fnp.process_packed(fid, x, packed), g[prefix + '_y'], 1e-12, prefix + ' forward')
  # a one-step curve is clip(x, 0, 1) whatever its parameter: dparams is float64 rounding noise around an exact 0 in the
  # fixture and in the oracles, and "relative to max |ref|" has no meaning; the scale is that of the two sums that cancel
  scale = fnp.curve_grad_abs_pieces(fid, x, packed, g['dy']).max() if L == 1 else None
  r_np = check_filter_grads(lambda *a: fnp.backward_packed(fid, *a), g, prefix, x, packed, 1e-10, prefix + ' (NumPy oracle)',
                            dp_scale=scale)
  r_t = check_filter_grads(via_torch(fid), g, prefix, x, packed, 1e-10, prefix + ' (torch oracle)', dp_scale=scale)
  print('GRADPIN cpu %s: NumPy %.2e torch %.2e (bound 1e-10)' % (prefix, r_np, r_t))


def test_oracles_backpropagate_the_analytic_hsv_mode_like_the_stand_in(fwd, g):
  """Case D, hsv_grad_mode = 1, on the smooth pixels (composition against the build's statement of TF's HSV formulas)."""
  smooth = g['hsv1_smooth']
  assert (~smooth).sum() <= 24 and smooth.shape == fwd['x'].shape[:3]
  x, packed = g['hsv1_x'], packed_params(fwd, 3)
  assert_gap(fnp.process_packed(3, x, packed), g['hsv1_SaturationPlusFilter_y'], 1e-12, 'forward')
  r_np = check_filter_grads(lambda *a: fnp.backward_packed(3, *a, hsv_grad_mode=1), g, 'hsv1_SaturationPlusFilter', x, packed,
                            1e-10, 'S+ analytic (NumPy oracle)', smooth)
  r_t = check_filter_grads(via_torch(3, 1), g, 'hsv1_SaturationPlusFilter', x, packed, 1e-10, 'S+ analytic (torch oracle)', smooth)
  print('GRADPIN cpu D: NumPy %.2e torch %.2e (bound 1e-10), %d non-smooth pixels' % (r_np, r_t, (~smooth).sum()))


def masked_backward(fid, x, packed, raw, dy):
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f64))
  _, dx, dp, draw = ft.apply_masked_backward(fid, t(x), t(packed), t(raw), t(dy), SHARP, MIN_STRENGTH)
  return dx.numpy(), dp.numpy(), draw.numpy()


@pytest.mark.parametrize('fid', MASKED)
def test_torch_oracle_backpropagates_the_masked_apply_like_the_reference(fwd, g, fid):
  """Case C: Filter.get_mask + filters.py:88; image 0 has all-zero raw mask parameters, image 1 saturated ones (+-20)."""
  name = FILTERS[fid]
  raw = g['C_%s_mask_params' % name]
  assert (raw[0] == 0).all() and (np.abs(raw[1]) == 20).all()
  dx, dp, draw = masked_backward(fid, fwd['x'], packed_params(fwd, fid), raw, g['dy'])
  r = max(assert_gap(dx, g['C_%s_dx' % name], 1e-10, name + ' masked dx'),
          assert_gap(dp, g['C_%s_dparams' % name], 1e-10, name + ' masked dparams'),
          assert_gap(draw, g['C_%s_dmask_params' % name], 1e-10, name + ' masked dmask_params'))
  print('GRADPIN cpu C %s: torch %.2e (bound 1e-10)' % (name, r))


# ---- regressor gradients ---------------------------------------------------------------------------------------------------
def product_filter(fid, L=8):
  from exposure_amd import filters as F
  from exposure_amd.config import make_cfg
  cfg = make_cfg()
  cfg.curve_steps = L
  classes = [F.ExposureFilter, F.GammaFilter, F.ImprovedWhiteBalanceFilter, F.SaturationPlusFilter, F.ToneFilter,
             F.ContrastFilter, F.WNBFilter, F.ColorFilter, F.LevelFilter]
  return classes[fid]((1, 64, 64, 3), cfg)


def regressor_cases(g, fwd):
  """(label, fid, L, features, dparams, dfeatures) of cases A and B."""
  for fid, name in enumerate(FILTERS):
    yield 'A_' + name, fid, 8, fwd[name + '_features'], g['A_%s_dparams' % name], g['A_%s_dfeatures' % name]
  p = 'A2_ContrastFilter'
  yield p, 5, 8, g[p + '_features'], g[p + '_dparams'], g[p + '_dfeatures']
  for L in CURVE_STEPS:
    for fid in (4, 7):
      p = 'B_L%d_%s' % (L, FILTERS[fid])
      yield p, fid, L, g[p + '_features'], g[p + '_dparams'], g[p + '_dfeatures']


def test_product_regressors_backpropagate_like_the_reference(fwd, g):
  """exposure_amd.filters.<Filter>.filter_param_regressor under torch float64 autograd."""
  for label, fid, L, features, dparams, want in regressor_cases(g, fwd):
    f = torch.from_numpy(features).requires_grad_(True)
    params = product_filter(fid, L).filter_param_regressor(f)
    got, = torch.autograd.grad(params, [f], torch.from_numpy(dparams).reshape(params.shape))
    r = assert_gap(got.numpy(), want, 1e-10, label + ' dfeatures')
    print('GRADPIN cpu regressor %s: %.2e (bound 1e-10)' % (label, r))


# heads_bwd takes `ranges` at their float32 values (the C ABI's float[9]).  Exposure (3.5, bias 0), Tone (0.5, 2, bias 0)
# and the filters without a range are exact there: 1e-10.  Gamma's log(3) carries a relative 2^-25 = 3e-8; the colour
# curve's width is the DIFFERENCE of the float32 1.1 and 0.9, each off by up to 2^-25 of itself: 2 * 3e-8 / 0.2 = 3e-7 of
# the gradient, plus the float32 bias through tanh'(x + b) (at most 2 |tanh| 2^-25 |b| = 4e-8): 1e-6 covers the worst case.
HEADS_BOUND = {0: 1e-10, 1: 1e-6, 2: 1e-10, 3: 1e-10, 4: 1e-10, 5: 1e-10, 6: 1e-10, 7: 1e-6, 8: 1e-10}


def heads_bwd_on(fid, features, dparams, **kw):
  pad = np.zeros((features.shape[0], R.MAX_PARAMS))
  pad[:, :dparams.shape[1]] = dparams
  draws, _ = R.heads_bwd([features], [fid], R.shipped_ranges(), np.zeros(features.shape[0], dtype=np.int32), pad, **kw)
  return draws[0]


def test_heads_bwd_backpropagates_like_the_reference(fwd, g):
  for fid, name in enumerate(FILTERS):
    got = heads_bwd_on(fid, fwd[name + '_features'], g['A_%s_dparams' % name])
    r = assert_gap(got, g['A_%s_dfeatures' % name], HEADS_BOUND[fid], name + ' heads_bwd')
    print('GRADPIN cpu heads_bwd %s: %.2e (bound %.0e)' % (name, r, HEADS_BOUND[fid]))


# ---- the agent's selection ---------------------------------------------------------------------------------------------------
AGENT_TAGS = {'agent': 8, 'agentx': 8, 'agentK5': 5, 'agentK12': 12}


def agent_inputs(fwd, g, tag):
  src, pre = (fwd, 'agent') if tag in ('agent', 'agentx') else (g, tag)
  gs, gq = (g['agent_g_s'], g['agent_g_q']) if src is fwd else (g[tag + '_g_s'], g[tag + '_g_q'])
  eps = 0.0625 if tag == 'agentx' else 0.05
  consts = np.array([eps, eps, 1.0, 1.0, 5], dtype=f32)  # exploration, exploration_penalty, usage, early stop, test_steps
  return dict(logits=src[pre + '_logits'], states=src[pre + '_states'], net=src[pre + '_net'], g_s=gs[:, 0], g_q=gq[:, 0],
              consts=consts, progress=0.25)


def check_select_bwd(fwd, g, tag, mode, bound, **kw):
  a = agent_inputs(fwd, g, tag)
  name = '%s_%s' % (tag, mode)
  sel = g[name + '_selected_filter_id']
  zero = np.zeros_like(a['g_s'])
  worst = 0.0
  for key, gs, gq in (('d_logits_surrogate', a['g_s'], zero), ('d_logits_penalty', zero, a['g_q']), ('d_logits', a['g_s'], a['g_q'])):
    got, _ = R.select_bwd(a['logits'], sel, a['progress'], a['consts'], gs, gq, **kw)
    scale = max(np.abs(g[name + '_d_logits']).max(), 1e-300)
    err = np.abs(got - g['%s_%s' % (name, key)]).max() / scale
    assert err <= bound, '%s %s: %.3g relative to max |d_logits| > %.1g' % (name, key, err, bound)
    worst = max(worst, err)
  return worst


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('tag', list(AGENT_TAGS))
def test_select_bwd_backpropagates_like_the_reference(fwd, g, tag, mode):
  """Case E: d(surrogate) / d(logits) and d(penalty) / d(logits) separately and summed.  select_bwd takes its constants at
  their float32 values: 1e-6 at the shipped 0.05, 1e-10 where they are exact in float32 (0.0625)."""
  name = '%s_%s' % (tag, mode)
  if mode == 'train':
    assert g[name + '_selected_filter_id'][0] == -1 and (g[name + '_d_logits_surrogate'][0] == 0).all()
  bound = 1e-10 if tag == 'agentx' else 1e-6
  r = check_select_bwd(fwd, g, tag, mode, bound)
  print('GRADPIN cpu select_bwd %s: %.2e (bound %.0e)' % (name, r, bound))


def test_overexposure_gradient_like_the_reference(fwd, g):
  """d_net of agent.py:249-250 against the restatement the CPU stand-in of the kernel uses (2 (y - 1)+ g / count)."""
  for tag in AGENT_TAGS:
    a = agent_inputs(fwd, g, tag)
    net = a['net']
    want = 2.0 * np.maximum(net - 1, 0) * a['g_q'][:, None, None, None] / (net.shape[1] * net.shape[2] * 3)
    for mode in ('train', 'eval'):
      assert_gap(want, g['%s_%s_d_net' % (tag, mode)], 1e-10, tag + ' d_net')


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
def fails(fn, *args, **kw):
  try:
    fn(*args, **kw)
  except AssertionError:
    return True
  return False


def _curve_backward_exclusive(img, k, dy, L):
  """filters_np._curve_backward with the MUTATION `t > 0` (an exclusive lower end of the clip's gradient)."""
  S = k.sum(axis=4) + 1e-30
  T, slope, clips = img * 0, img * 0, []
  for i in range(L):
    t = img - 1.0 * i / L
    c = np.clip(t, 0, 1.0 / L)
    clips.append(c)
    T = T + c * k[..., i]
    slope = slope + k[..., i] * ((t > 0) & (t <= 1.0 / L))
  y = T * (L / S)
  return dy * (L / S) * slope, np.stack([dy * ((L / S) * clips[i] - y / S) for i in range(L)], axis=-1)


def _tone_mutant(img, p, dy):
  dx, dk = _curve_backward_exclusive(img, p.reshape(-1, 1, 1, 1, p.shape[1]), dy, p.shape[1])
  return dx, dk.sum(axis=(1, 2, 3))


def _gamma_mutant(img, p, dy):
  """filters_np.gamma_backward with the MUTATION `img > 0.001`."""
  gm = p[:, None, None, :]
  xm = np.maximum(img, 0.001)
  return dy * gm * np.power(xm, gm - 1) * (img > 0.001), (dy * np.power(xm, gm) * np.log(xm)).reshape(img.shape[0], -1).sum(axis=1)[:, None]


def _contrast_mutant(img, p, dy):
  """filters_np.contrast_backward with the MUTATION of an exclusive luminance mask."""
  pp = p[:, :, None, None]
  w = np.array(fnp.LUM_W, dtype=img.dtype)
  lraw = fnp.rgb2lum(img)
  l = np.minimum(np.maximum(lraw, 0.0), 1.0)
  m = ((lraw > 0.0) & (lraw < 1.0)).astype(img.dtype)
  cl = -np.cos(math.pi * l) * 0.5 + 0.5
  ratio = cl / (l + 1e-6)
  G = 0.5 * math.pi * np.sin(math.pi * l) / (l + 1e-6) - cl / (l + 1e-6)**2
  dot = (dy * img).sum(axis=3, keepdims=True)
  dx = (1 - pp) * dy + pp * (dy * ratio + w * (m * G * dot))
  return dx, (dy * (img * ratio - img)).reshape(img.shape[0], -1).sum(axis=1)[:, None]


def test_the_assertions_reject_wrong_tie_conventions(fwd, g):
  """The same assertions as above, fed four mutants, must fail (and must pass on the unmutated copies' originals)."""
  x = fwd['x']
  for fid, mutant in ((4, _tone_mutant), (1, _gamma_mutant), (5, _contrast_mutant)):
    name = FILTERS[fid]
    # (Contrast: case A2 -- in case A the parameter of the image that holds the lum = 1 tie is tanh(0) = 0)
    args = (g, 'A2_' + name, x, g['A2_ContrastFilter_params'], 1e-10, name) if fid == 5 else \
        (g, 'A_' + name, x, packed_params(fwd, fid), 1e-10, name)
    assert not fails(check_filter_grads, lambda *a: fnp.backward_packed(fid, *a), *args)
    assert fails(check_filter_grads, mutant, *args), 'the %s mutant passed: the fixture lacks the pixel that separates it' % name
  # (iii) is separated by (1, 1, 1) alone, whose float64 luminance is exactly 1.0: at (0, 0, 0) the masked term is times dy . x = 0
  assert fnp.rgb2lum(x)[0, 1, 1, 0] == 1.0
  for mode in ('train', 'eval'):
    assert not fails(check_select_bwd, fwd, g, 'agentx', mode, 1e-10)
    assert fails(check_select_bwd, fwd, g, 'agentx', mode, 1e-10, entropy_term=False)
    assert fails(check_select_bwd, fwd, g, 'agent', mode, 1e-6, entropy_term=False)
  name = FILTERS[2]
  good = heads_bwd_on(2, fwd[name + '_features'], g['A_%s_dparams' % name])
  bad = heads_bwd_on(2, fwd[name + '_features'], g['A_%s_dparams' % name], wb_cross_term=False)
  assert not fails(assert_gap, good, g['A_%s_dfeatures' % name], 1e-10, name)
  assert fails(assert_gap, bad, g['A_%s_dfeatures' % name], 1e-10, name)


# ---- lrelu ---------------------------------------------------------------------------------------------------------------------
def test_lrelu_slope_at_zero(fwd, g):
  """util.py:225-229 is 0.6 x + 0.4 |x|: under abs'(0) = 0 its derivative at 0 (and -0.0) is 0.6, not the 0.2 or 1 of
  where(x > 0, x, 0.2 x).  The oracle and the kernels' restatement (tests/_fake_hip.py; nn_ops.hip's lrelu_slope has the same
  three branches) give the same 0.6: no deviation to record."""
  from tests import _fake_hip
  x, dx = fwd['util_lrelu_x'], g['util_lrelu_dx']
  assert x[0] == 0 and x[1] == 0 and np.signbit(x[1]) and x[2] == 1e-30
  assert dx[0] == 0.6 and dx[1] == 0.6 and dx[2] == 1.0
  np.testing.assert_array_equal(dx, np.where(x > 0, 1.0, np.where(x < 0, 0.6 - 0.4, 0.6)))
  np.testing.assert_allclose(nets_np.lrelu_grad(x), dx, rtol=1e-15)
  assert nets_np.lrelu_grad(np.zeros(1))[0] == 0.6
  z = torch.from_numpy(x[:3].astype(f32))
  out = torch.empty_like(z)
  _fake_hip._lrelu_bwd(z, torch.ones_like(z), out)
  assert out.tolist() == [f32(0.6), f32(0.6), 1.0]


# ---- ties under fp32: what the fixture comparison on the GPU may skip, checked on the CPU -------------------------------------
def knot_elements(x, L):
  """L no power of two: the elements that sit on a knot 1 / L .. L / L (at the precision of `x`) -- the L constructed
  pixels of case B and the constructed 0.2, 0.4 and 1.0 of the forward fixture's x (see the module docstring)."""
  m = np.zeros(x.shape, dtype=bool)
  if L & (L - 1):
    m = np.isin(x, (np.arange(1, L + 1) / float(L)).astype(x.dtype))
  return m


def tie_skips(same_dx, fix_dx, imgs, exempt, what):
  """Pixels where the float64 oracle on the fp32-rounded inputs and the fixture differ by more than the image tolerance:
  at most 4 per filter, each one a constructed precision-dependent tie (`exempt`: elements held otherwise)."""
  differ = ((np.abs(same_dx - fix_dx) > image_tol(fix_dx, f32)) & ~exempt).any(axis=-1)
  where = {(int(imgs[i]), int(r), int(c)) for i, r, c in zip(*np.nonzero(differ))}
  assert where <= PRECISION_TIES and differ.sum() <= 4, '%s: the fixture and the same-input oracle differ at %s' % (what, sorted(where))
  return differ


def to32(a):
  return np.ascontiguousarray(a, dtype=f32)


def same_input_oracle(fid, x32, p32, dy32, mode=0, dpen=None):
  """float64 oracle on the kernel's own fp32 inputs -> (dx, dparams, A, the cotangent with the penalty's share)."""
  x64, p64, gy = x32.astype(f64), p32.astype(f64), dy32.astype(f64)
  if dpen is not None:
    y = fnp.process_packed(fid, x64, p64)
    gy = gy + 2.0 * np.maximum(y - 1, 0) * dpen.astype(f64)[:, None, None, None] / (x64.shape[1] * x64.shape[2] * 3)
  dx, dp = fnp.backward_packed(fid, x64, p64, gy, mode)
  one_step = fid in (4, 7) and p64.shape[1] == (1 if fid == 4 else 3)
  # (a one-step curve's parameter gradient is exactly 0 term by term: the scale of its two-sum evaluation, filters_np)
  a = (fnp.curve_grad_abs_pieces if one_step else fnp.param_grad_abs)(fid, x64, p64, gy)
  return dx, dp, a


def test_the_fixture_and_the_same_input_oracle_differ_only_at_the_constructed_ties(fwd, g):
  imgs = np.arange(6)
  none = np.zeros(fwd['x'].shape, dtype=bool)
  total = {}
  for fid, name in enumerate(FILTERS):
    dx, _, _ = same_input_oracle(fid, to32(fwd['x']), to32(packed_params(fwd, fid)), to32(g['dy']))
    total[name] = int(tie_skips(dx, g['A_%s_dx' % name], imgs, none, name).sum())
  assert total['GammaFilter'] <= 1 and total['ContrastFilter'] <= 1
  for L in CURVE_STEPS:
    for fid in (4, 7):
      p = 'B_L%d_%s' % (L, FILTERS[fid])
      xb = x_of_case_b(fwd, g, L)
      knots = knot_elements(xb, L)
      assert knots.any(axis=-1).sum() == {1: 0, 3: 3 + 2, 5: 5 + 6, 16: 0}[L]  # (the second number: 0.2, 0.4, 1.0 in the fixture's x)
      dx, _, _ = same_input_oracle(fid, to32(xb), to32(g[p + '_params']), to32(g['dy']))
      total[p] = int(tie_skips(dx, g[p + '_dx'], imgs, knots, p).sum())
  print('GRADPIN cpu skipped tie pixels (fixture vs same-input oracle): %s' % {k: v for k, v in total.items() if v})


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def dev32(a, dev):
  return torch.from_numpy(to32(a)).to(dev)


def worst_image(got, ref):
  return float((np.abs(np.asarray(got, dtype=f64) - ref) / image_tol(ref, f32)).max()) if np.size(ref) else 0.0


def worst_param(got, ref, a):
  tol = param_grad_tol(ref, a) + 1e-10 * a.max()
  return float((np.abs(np.asarray(got, dtype=f64) - ref) / np.maximum(tol, 1e-300)).max())


def hold_knot_elements(got_dx, x32, p32, dy32, fid, L, knots, what):
  """The kernel's dx at the inexact knots i / L: one of the sub-gradients of an inclusive clip (module docstring)."""
  cc = 1 if fid == 4 else 3
  k = p32.astype(f64).reshape(-1, cc, L)
  for n, r, c, ch in zip(*np.nonzero(knots)):
    kk = k[n, 0 if cc == 1 else ch]
    i = int(round(float(x32[n, r, c, ch]) * L))
    assert 1 <= i <= L and abs(float(x32[n, r, c, ch]) - i / L) < 1e-7
    scale = float(dy32[n, r, c, ch]) * L / (kk.sum() + 1e-30)
    upper = kk[i] if i < L else 0.0
    cands = np.array([scale * upper, scale * (upper + kk[i - 1])])
    err = np.abs(float(got_dx[n, r, c, ch]) - cands)
    assert (err <= image_tol(cands, f32)).any(), '%s: dx %.7g at knot %d / %d is none of %s' % (what, got_dx[n, r, c, ch], i, L, cands)


def hold_rows(what, fid, got_dx, got_dp, x32, p32, dy32, fix_dx, fix_dp, imgs, mode=0, dpen=None, smooth=None, L=8):
  """One filter's rows of a launch against the same-input oracle everywhere and against the fixture outside the
  precision-dependent ties; returns (worst err / tol of dx, of dparams, skipped pixels) against the FIXTURE."""
  same_dx, same_dp, a = same_input_oracle(fid, x32, p32, dy32, mode, dpen)
  keep = np.ones(x32.shape, dtype=bool)
  if smooth is not None:
    keep &= smooth[np.asarray(imgs)][..., None]
  knots = np.zeros_like(keep)
  if fid in (4, 7) and L & (L - 1):
    assert dpen is None or (fnp.process_packed(fid, x32.astype(f64), p32.astype(f64)) <= 1 + 1e-6).all()  # (the penalty's share is 0)
    knots = knot_elements(x32, L)
    hold_knot_elements(got_dx, x32, p32, dy32, fid, L, knots, what)
  keep &= ~knots
  assert_image_close(got_dx[keep], same_dx[keep], f32, what + ' dx vs the same-input oracle')
  assert_param_grad_close(got_dp, same_dp, a, what + ' dparams vs the same-input oracle')
  skip = tie_skips(same_dx, fix_dx, imgs, ~keep, what)
  keep &= ~skip[..., None]
  assert_image_close(got_dx[keep], fix_dx[keep], f32, what + ' dx vs the fixture')
  assert_param_grad_close(got_dp, fix_dp, a, what + ' dparams vs the fixture')
  return worst_image(got_dx[keep], fix_dx[keep]), worst_param(got_dp, fix_dp, a), int(skip.sum())


@pytest.mark.gpu
@pytest.mark.parametrize('fid', range(9))
def test_hip_filter_bwd_backpropagates_like_the_reference(fwd, g, fid, gpu_device):
  """expo_filter_bwd, hsv_grad_mode 0, against case A."""
  from exposure_amd import _cabi
  name = FILTERS[fid]
  x32, p32, dy32 = to32(fwd['x']), to32(packed_params(fwd, fid)), to32(g['dy'])
  x, p, dy = (torch.from_numpy(a).to(gpu_device) for a in (x32, p32, dy32))
  dx, dp = torch.full_like(x, float('nan')), torch.full_like(p, float('nan'))
  _cabi.filter_bwd(fid, x, dy, dx, p, dp, hsv_grad_mode=0)
  r = hold_rows(name, fid, dx.cpu().numpy(), dp.cpu().numpy(), x32, p32, dy32, g['A_%s_dx' % name], g['A_%s_dparams' % name],
                np.arange(6))
  print('GRADPIN gpu filter_bwd %s: dx %.3f dparams %.3f of tol, %d tie pixels skipped' % ((name,) + r))
  if fid == 5:  # case A2: a live parameter on the image that holds the lum = 1 tie
    p32 = to32(g['A2_ContrastFilter_params'])
    _cabi.filter_bwd(fid, x, dy, dx, torch.from_numpy(p32).to(gpu_device), dp, hsv_grad_mode=0)
    r = hold_rows(name + ' A2', fid, dx.cpu().numpy(), dp.cpu().numpy(), x32, p32, dy32, g['A2_ContrastFilter_dx'],
                  g['A2_ContrastFilter_dparams'], np.arange(6))
    print('GRADPIN gpu filter_bwd %s A2: dx %.3f dparams %.3f of tol, %d tie pixels skipped' % ((name,) + r))


@pytest.mark.gpu
def test_hip_filter_bwd_analytic_hsv_mode_like_the_stand_in(fwd, g, gpu_device):
  """expo_filter_bwd, SaturationPlus, hsv_grad_mode 1, against case D on its smooth pixels."""
  from exposure_amd import _cabi
  x32, p32, dy32 = to32(g['hsv1_x']), to32(packed_params(fwd, 3)), to32(g['dy'])
  x, p, dy = (torch.from_numpy(a).to(gpu_device) for a in (x32, p32, dy32))
  dx, dp = torch.full_like(x, float('nan')), torch.full_like(p, float('nan'))
  _cabi.filter_bwd(3, x, dy, dx, p, dp, hsv_grad_mode=1)
  r = hold_rows('S+ analytic', 3, dx.cpu().numpy(), dp.cpu().numpy(), x32, p32, dy32, g['hsv1_SaturationPlusFilter_dx'],
                g['hsv1_SaturationPlusFilter_dparams'], np.arange(6), mode=1, smooth=g['hsv1_smooth'])
  print('GRADPIN gpu filter_bwd S+ hsv_grad_mode 1: dx %.3f dparams %.3f of tol, %d tie pixels skipped' % r)


@pytest.mark.gpu
@pytest.mark.parametrize('curves', [1, 3])
@pytest.mark.parametrize('L', CURVE_STEPS)
def test_hip_curve_bwd_backpropagates_like_the_reference(fwd, g, L, curves, gpu_device):
  """expo_curve_bwd (curve_generic.hip) against case B."""
  from exposure_amd import _cabi
  fid = 4 if curves == 1 else 7
  prefix = 'B_L%d_%s' % (L, FILTERS[fid])
  x32, p32, dy32 = to32(x_of_case_b(fwd, g, L)), to32(g[prefix + '_params']), to32(g['dy'])
  x, p, dy = (torch.from_numpy(a).to(gpu_device) for a in (x32, p32, dy32))
  dx, dp = torch.full_like(x, float('nan')), torch.full_like(p, float('nan'))
  _cabi.curve_bwd(x, dy, dx, p, dp, curves, L)
  r = hold_rows(prefix, fid, dx.cpu().numpy(), dp.cpu().numpy(), x32, p32, dy32, g[prefix + '_dx'], g[prefix + '_dparams'],
                np.arange(6), L=L)
  print('GRADPIN gpu curve_bwd %s: dx %.3f dparams %.3f of tol, %d tie pixels skipped' % ((prefix,) + r))


def dispatch_batch(fwd, g, L):
  """24 images: ids -1, 0 .. 8, -1, 0 .. 8, -1, 0, 1, 2; the first ten are image 0 of the fixture (every tie pixel), the
  next ten image 1 (negative and > 1 channels), the rest image 2.  -> ids, imgs, x, dy, rows (width 24 or 48), prefixes."""
  width = 24 if L == 8 else 48
  ids = (np.arange(24) % 10 - 1).astype(np.int32)
  imgs = np.arange(24) // 10
  xs, rows, prefixes = [], np.zeros((24, width), dtype=f32), []
  for s, (fid, i) in enumerate(zip(ids, imgs)):
    curve = fid in (4, 7) and L != 8
    prefix = None if fid < 0 else ('B_L%d_%s' % (L, FILTERS[fid]) if curve else 'A_' + FILTERS[fid])
    xs.append((x_of_case_b(fwd, g, L) if curve else fwd['x'])[i])
    if fid >= 0:
      p = g[prefix + '_params'] if curve else packed_params(fwd, fid)
      rows[s, :p.shape[1]] = p[i]
    prefixes.append(prefix)
  return ids, imgs, to32(np.stack(xs)), to32(g['dy'][imgs]), rows, prefixes


def hold_dispatch(what, g, got_dx, got_dp, ids, imgs, x32, dy32, rows, prefixes, L, dpen):
  none = ids < 0
  assert none.sum() == 3 and (got_dx[none] == 0).all() and (got_dp[none] == 0).all(), what + ': the rows that selected nothing'
  worst = [0.0, 0.0, 0]
  for fid in range(9):
    sel = np.flatnonzero(ids == fid)
    prefix = prefixes[sel[0]]
    pen = dpen is not None and prefix not in set(str(s) for s in g['pen_is_plain'])
    fix_dx, fix_dp = g[prefix + ('_pen_dx' if pen else '_dx')], g[prefix + ('_pen_dparams' if pen else '_dparams')]
    width = fix_dp.shape[1]
    assert (got_dp[sel, width:] == 0).all(), what + ': behind the parameters'
    r = hold_rows('%s %s' % (what, prefix), fid, got_dx[sel], got_dp[sel, :width], x32[sel], rows[sel, :width], dy32[sel],
                  fix_dx[imgs[sel]], fix_dp[imgs[sel]], imgs[sel], dpen=None if dpen is None else dpen[sel],
                  L=L if fid in (4, 7) else 8)
    worst = [max(worst[0], r[0]), max(worst[1], r[1]), worst[2] + r[2]]
  return tuple(worst)


@pytest.mark.gpu
@pytest.mark.parametrize('with_penalty', [False, True], ids=['plain', 'dpenalty'])
def test_hip_dispatch_bwd_backpropagates_like_the_reference(fwd, g, with_penalty, gpu_device):
  """expo_filter_dispatch_bwd, one launch over all nine filters and id -1: every image equals its filter's fixture rows;
  with dpenalty the loss also holds the over-exposure penalty of y (agent.py:249-250)."""
  from exposure_amd import _cabi
  dev = gpu_device
  ids, imgs, x32, dy32, rows, prefixes = dispatch_batch(fwd, g, 8)
  dpen = to32(g['dpen'][imgs]) if with_penalty else None
  dx, dp = torch.full((24, 12, 10, 3), float('nan'), device=dev), torch.full((24, 24), float('nan'), device=dev)
  _cabi.dispatch_bwd(torch.from_numpy(ids).to(dev), dev32(x32, dev), dev32(dy32, dev), dx, dev32(rows, dev), dp,
                     None if dpen is None else dev32(dpen, dev))
  r = hold_dispatch('dispatch_bwd', g, dx.cpu().numpy(), dp.cpu().numpy(), ids, imgs, x32, dy32, rows, prefixes, 8, dpen)
  print('GRADPIN gpu dispatch_bwd%s: dx %.3f dparams %.3f of tol, %d tie pixels skipped' % ((' + dpenalty' if with_penalty else '',) + r))


@pytest.mark.gpu
@pytest.mark.parametrize('with_penalty', [False, True], ids=['plain', 'dpenalty'])
@pytest.mark.parametrize('L', [5, 16])
def test_hip_dispatch_curves_bwd_backpropagates_like_the_reference(fwd, g, L, with_penalty, gpu_device):
  """expo_filter_dispatch_curves_bwd (dispatch_curves.hip): Tone / Color rows against case B, the light rows against A."""
  from exposure_amd import _cabi
  dev = gpu_device
  ids, imgs, x32, dy32, rows, prefixes = dispatch_batch(fwd, g, L)
  dpen = to32(g['dpen'][imgs]) if with_penalty else None
  dx, dp = torch.full((24, 12, 10, 3), float('nan'), device=dev), torch.full((24, 48), float('nan'), device=dev)
  _cabi.dispatch_curves_bwd(torch.from_numpy(ids).to(dev), dev32(x32, dev), dev32(dy32, dev), dx, dev32(rows, dev), dp, L,
                            None if dpen is None else dev32(dpen, dev))
  r = hold_dispatch('dispatch_curves_bwd L = %d' % L, g, dx.cpu().numpy(), dp.cpu().numpy(), ids, imgs, x32, dy32, rows,
                    prefixes, L, dpen)
  print('GRADPIN gpu dispatch_curves_bwd L = %d%s: dx %.3f dparams %.3f of tol, %d tie pixels skipped' %
        ((L, ' + dpenalty' if with_penalty else '') + r))


def masked_inputs(fwd, g, fids):
  """Rows of the masked cases (six images per filter): x, packed (24 wide), raw mask parameters, post-tanh_range mask
  parameters (what the kernels take) and d mp / d raw = 5 (1 - tanh(raw)^2) of tanh_range(-5, 5, initial=0)."""
  n = 6 * len(fids)
  ids = np.repeat(np.asarray(fids, dtype=np.int32), 6)
  imgs = np.tile(np.arange(6), len(fids))
  rows, raw = np.zeros((n, 24), dtype=f32), np.zeros((n, 6))
  for j, fid in enumerate(fids):
    p = packed_params(fwd, fid)
    rows[6 * j:6 * j + 6, :p.shape[1]] = p
    raw[6 * j:6 * j + 6] = g['C_%s_mask_params' % FILTERS[fid]]
  raw32 = to32(raw)
  mp = fnp.tanh_range(-5, 5, initial=0)(raw32.astype(f64))
  dmp_draw = 5.0 * (1.0 - np.tanh(raw32.astype(f64))**2)
  return ids, imgs, to32(fwd['x'][imgs]), to32(g['dy'][imgs]), rows, raw32, to32(mp), dmp_draw


def hold_masked(what, g, fid, got_dx, got_dp, got_draw, x32, p32, raw32, dy32, imgs):
  name = FILTERS[fid]
  x64, p64, raw64, dy64 = (a.astype(f64) for a in (x32, p32, raw32, dy32))
  same_dx, same_dp, same_draw = masked_backward(fid, x64, p64, raw64, dy64)
  a_p = fnp.abs_terms_fd(lambda q: fnp.apply_masked(fid, x64, q, raw64, SHARP, MIN_STRENGTH), p64, dy64)
  a_raw = fnp.masked_raw_grad_abs(fid, x64, p64, raw64, dy64, SHARP, MIN_STRENGTH)
  assert_image_close(got_dx, same_dx, f32, what + ' dx vs the same-input oracle')
  assert_param_grad_close(got_dp, same_dp, a_p, what + ' dparams vs the same-input oracle')
  assert_param_grad_close(got_draw, same_draw, a_raw, what + ' dmask_params vs the same-input oracle')
  fix_dx = g['C_%s_dx' % name][imgs]
  keep = ~tie_skips(same_dx, fix_dx, imgs, np.zeros(x32.shape, dtype=bool), what)
  assert_image_close(got_dx[keep], fix_dx[keep], f32, what + ' dx vs the fixture')
  fix_dp, fix_draw = g['C_%s_dparams' % name][imgs], g['C_%s_dmask_params' % name][imgs]
  assert_param_grad_close(got_dp, fix_dp, a_p, what + ' dparams vs the fixture')
  assert_param_grad_close(got_draw, fix_draw, a_raw, what + ' dmask_params vs the fixture')
  return (worst_image(got_dx[keep], fix_dx[keep]), worst_param(got_dp, fix_dp, a_p), worst_param(got_draw, fix_draw, a_raw),
          int((~keep).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize('fid', MASKED)
def test_hip_apply_bwd_backpropagates_like_the_reference(fwd, g, fid, gpu_device):
  """expo_filter_apply_bwd against case C (the kernel differentiates with respect to the post-tanh_range mask
  parameters; the chain rule through tanh_range is applied here in float64)."""
  from exposure_amd import _cabi
  dev = gpu_device
  _, imgs, x32, dy32, rows, raw32, mp32, dmp_draw = masked_inputs(fwd, g, [fid])
  p32 = np.ascontiguousarray(rows[:, :fnp.NUM_PARAMS[fid]])
  dx, dp, dmp = torch.full((6, 12, 10, 3), float('nan'), device=dev), torch.full(p32.shape, float('nan'), device=dev), \
      torch.full((6, 6), float('nan'), device=dev)
  _cabi.apply_bwd(fid, dev32(x32, dev), dev32(dy32, dev), dx, dev32(p32, dev), dp, dev32(mp32, dev), dmp, SHARP, MIN_STRENGTH)
  r = hold_masked('apply_bwd ' + FILTERS[fid], g, fid, dx.cpu().numpy(), dp.cpu().numpy(),
                  dmp.cpu().numpy().astype(f64) * dmp_draw, x32, p32, raw32, dy32, imgs)
  print('GRADPIN gpu apply_bwd %s: dx %.3f dparams %.3f dmask_params %.3f of tol, %d tie pixels skipped' % ((FILTERS[fid],) + r))


@pytest.mark.gpu
def test_hip_apply_dispatch_bwd_backpropagates_like_the_reference(fwd, g, gpu_device):
  """expo_filter_apply_dispatch_bwd, one launch over the four filters of case C."""
  from exposure_amd import _cabi
  dev = gpu_device
  ids, imgs, x32, dy32, rows, raw32, mp32, dmp_draw = masked_inputs(fwd, g, MASKED)
  dx, dp, dmp = torch.full((24, 12, 10, 3), float('nan'), device=dev), torch.full((24, 24), float('nan'), device=dev), \
      torch.full((24, 6), float('nan'), device=dev)
  _cabi.apply_dispatch_bwd(torch.from_numpy(ids).to(dev), dev32(x32, dev), dev32(dy32, dev), dx, dev32(rows, dev), dp,
                           dev32(mp32, dev), dmp, SHARP, MIN_STRENGTH)
  got_dx, got_dp, got_draw = dx.cpu().numpy(), dp.cpu().numpy(), dmp.cpu().numpy().astype(f64) * dmp_draw
  for fid in MASKED:
    sel = np.flatnonzero(ids == fid)
    width = fnp.NUM_PARAMS[fid]
    assert (got_dp[sel, width:] == 0).all()
    r = hold_masked('apply_dispatch_bwd ' + FILTERS[fid], g, fid, got_dx[sel], got_dp[sel, :width], got_draw[sel], x32[sel],
                    np.ascontiguousarray(rows[sel, :width]), raw32[sel], dy32[sel], imgs[sel])
    print('GRADPIN gpu apply_dispatch_bwd %s: dx %.3f dparams %.3f dmask_params %.3f of tol, %d tie pixels skipped' % ((FILTERS[fid],) + r))


def product_ranges():
  """The C ABI's float[9] exactly as exposure_amd.filters.heads_regress_select builds it from make_cfg()."""
  from exposure_amd.config import make_cfg
  cfg = make_cfg()
  tl, tr = cfg.tone_curve_range
  cl, cr = cfg.color_curve_range
  bias = lambda l, r, initial: math.atanh(2 * (initial - l) / (r - l) - 1) if initial is not None else 0.0
  return (float(cfg.exposure_range), math.log(cfg.gamma_range), float(tl), float(tr), 0.0, float(cl), float(cr), bias(cl, cr, 1),
          bias(-cfg.exposure_range, cfg.exposure_range, 0))


def heads_case(cases, width):
  """One launch: head j's six rows are rows 6 j .. 6 j + 5; every other head's features there are other rows' (ignored)."""
  n = 6 * len(cases)
  raws = [np.tile(to32(features), (len(cases), 1)) for _, _, _, features, _, _ in cases]
  selected = np.repeat(np.arange(len(cases), dtype=np.int32), 6)
  dparams = np.zeros((n, width), dtype=f32)
  for j, (_, _, _, _, dp, _) in enumerate(cases):
    dparams[6 * j:6 * j + 6, :dp.shape[1]] = dp
  return raws, selected, dparams


def hold_heads(what, cases, draws, raws, selected, dparams, ranges, L):
  from tests import _curve_dispatch_ref as C
  ids = [fid for _, fid, _, _, _, _ in cases]
  _, scale = (R.heads_bwd(raws, ids, ranges, selected, dparams) if L == 8 else C.heads_bwd(raws, ids, ranges, selected, dparams, L))
  worst = 0.0
  for j, (label, fid, _, features, _, want) in enumerate(cases):
    got = draws[j]
    assert (got[selected != j] == 0).all(), label
    r = R.assert_close(got[6 * j:6 * j + 6], want, 0, R.C_DRAW, scale[j][6 * j:6 * j + 6], '%s %s dfeatures' % (what, label))
    worst = max(worst, r)
  return worst


@pytest.mark.gpu
def test_hip_heads_regress_bwd_backpropagates_like_the_reference(fwd, g, gpu_device):
  """expo_heads_regress_bwd: dfeatures of case A for all nine heads in one launch, C_DRAW x the sum of the absolute terms."""
  from exposure_amd import _cabi
  dev = gpu_device
  cases = [c for c in regressor_cases(g, fwd) if c[2] == 8 and c[0].startswith('A_')]
  raws, selected, dparams = heads_case(cases, R.MAX_PARAMS)
  ids, ranges = [c[1] for c in cases], product_ranges()
  traws = [dev32(r, dev) for r in raws]
  draws = [torch.full(tuple(r.shape), float('nan'), device=dev) for r in raws]
  _cabi.heads_regress_bwd(traws, draws, ids, ranges, torch.from_numpy(selected).to(dev), dev32(dparams, dev))
  r = hold_heads('heads_regress_bwd', cases, [d.cpu().numpy() for d in draws], raws, selected, dparams, ranges, 8)
  print('GRADPIN gpu heads_regress_bwd: %.3f of tol' % r)


@pytest.mark.gpu
@pytest.mark.parametrize('L', CURVE_STEPS)
def test_hip_heads_regress_curves_bwd_backpropagates_like_the_reference(fwd, g, L, gpu_device):
  """expo_heads_regress_curves_bwd: dfeatures of case B (a Tone and a Color head of L steps)."""
  from exposure_amd import _cabi
  dev = gpu_device
  cases = [c for c in regressor_cases(g, fwd) if c[0].startswith('B_L%d_' % L)]
  raws, selected, dparams = heads_case(cases, 48)
  ids, ranges = [c[1] for c in cases], product_ranges()
  traws = [dev32(r, dev) for r in raws]
  draws = [torch.full(tuple(r.shape), float('nan'), device=dev) for r in raws]
  _cabi.heads_regress_curves_bwd(traws, draws, ids, ranges, torch.from_numpy(selected).to(dev), dev32(dparams, dev), L)
  r = hold_heads('heads_regress_curves_bwd L = %d' % L, cases, [d.cpu().numpy() for d in draws], raws, selected, dparams, ranges, L)
  print('GRADPIN gpu heads_regress_curves_bwd L = %d: %.3f of tol' % (L, r))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('tag', ['agent', 'agentK5', 'agentK12'])
def test_hip_agent_select_bwd_backpropagates_like_the_reference(fwd, g, tag, mode, gpu_device):
  """expo_agent_select_bwd (K = 8, 5, 12) against case E, C_DLOGITS (|ref| + select_bwd's sum of absolute terms)."""
  from exposure_amd import _cabi
  dev = gpu_device
  a = agent_inputs(fwd, g, tag)
  name = '%s_%s' % (tag, mode)
  sel = g[name + '_selected_filter_id'].astype(np.int32)
  n, k = a['logits'].shape
  d_logits = torch.full((n, k), float('nan'), device=dev)
  _cabi.agent_select_bwd(dev32(a['logits'], dev), torch.from_numpy(sel).to(dev), torch.tensor([a['progress']], dtype=torch.float32, device=dev),
                         a['consts'], 3 + k, dev32(a['g_s'], dev), dev32(a['g_q'], dev), d_logits)
  _, scale = R.select_bwd(to32(a['logits']), sel, a['progress'], a['consts'], a['g_s'], a['g_q'])
  r = R.assert_close(d_logits.cpu().numpy(), g[name + '_d_logits'], R.C_DLOGITS, R.C_DLOGITS, scale, name + ' d_logits')
  print('GRADPIN gpu agent_select_bwd %s: %.3f of tol' % (name, r))


@pytest.mark.gpu
def test_hip_overexposure_penalty_bwd_backpropagates_like_the_reference(fwd, g, gpu_device):
  """expo_overexposure_penalty_bwd against d_net of case E."""
  from exposure_amd import _cabi
  dev = gpu_device
  worst = 0.0
  for tag in ('agent', 'agentK5', 'agentK12'):
    a = agent_inputs(fwd, g, tag)
    net = dev32(a['net'], dev)
    d_net = torch.full_like(net, float('nan'))
    _cabi.overexposure_penalty_bwd(net, dev32(a['g_q'], dev), d_net)
    want = g[tag + '_train_d_net']
    assert (want != 0).any() and np.array_equal(want, g[tag + '_eval_d_net'])
    # an element within float32 rounding of 1.0 may fall on the other side of the kink: its gradient is below 1e-7 either way
    assert_image_close(d_net.cpu().numpy(), want, f32, tag + ' d_net')
    worst = max(worst, worst_image(d_net.cpu().numpy(), want))
  print('GRADPIN gpu overexposure_penalty_bwd: %.3f of tol' % worst)
