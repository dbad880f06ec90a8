"""CPU: the reference of the training step's loss-glue kernels (tests/_step_glue_ref.py) checked against the oracle it is
built on (``oracle/nets_np.py``'s two loss graphs), its hand-derived gradients against torch's float64 autograd of the
formula written in torch ops and against central differences with the scheme's own error estimate, the float32
restatements' error against the constants the GPU tests use (each constant is at least 4 x that error, on exactly the inputs
of tests/test_hip_step_glue.py) and the GPU tests' comparisons against wrong results they have to reject."""
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import nets_np
from tests import _step_glue_ref as R
from tests._glue_checks import fd_check as _fd_check, rejected as _rejected
from tests.test_oracle_nets import random_critic_weights, small_cfg

f32, f64 = np.float32, np.float64


# ---- the reference is the oracle ---------------------------------------------------------------------------------------
def test_penalty_and_report_are_the_oracles_critic_losses():
  rng = np.random.default_rng(3)
  cfg = small_cfg()
  weights = random_critic_weights(rng, cfg, 'critic/', 6)
  weights['critic/fully_connected_1/weights'] *= 0.15  # gradient norms on both sides of 1
  n = 5
  real, fake = rng.random((n, 16, 16, 3)), 1.5 * rng.random((n, 16, 16, 3))
  alpha = rng.random((n, 1, 1, 1))
  want = nets_np.critic_losses(real, fake, alpha, cfg, weights)
  norm, term = R.penalty_fwd(want['gradients'])
  assert (norm > 1).any() and (norm < 1).any()
  logits = np.concatenate([nets_np.critic(real, cfg, weights), nets_np.critic(fake, cfg, weights), want['inte_logit']])[:, 0]
  out, _, _, _ = R.critic_report(logits, norm, term, (n, n, n), cfg['gradient_penalty_lambda'], 0.99, 0.0)
  for got, name in zip(out, ('c_loss', 'emd', 'gradient_norm', 'gradient_penalty', 'c_average')):
    np.testing.assert_allclose(got, want[name], rtol=1e-13, atol=1e-15, err_msg=name)
  _, interp, _ = R.gp_inputs(real, fake, alpha.reshape(n))  # (alpha: float32 values in the reference)
  np.testing.assert_allclose(interp, real + alpha.astype(f32) * (fake - real), rtol=1e-15)


@pytest.mark.parametrize('use_td', [True, False])
@pytest.mark.parametrize('use_penalty', [True, False])
def test_generator_losses_are_the_oracles(use_td, use_penalty):
  """``nets_np.generator_losses`` with the networks replaced by the per-image scalars: the loss graph from ``stopped`` on."""
  n, d = 37, 11
  x = R.gen_inputs(n, d, 5)
  col = lambda k: x[k].astype(f64)[:, None]
  a, mult, disc, plm, max_len = [float(v) for v in R.GEN_CONSTS]
  cfg = dict(all_reward=a, critic_logit_multiplier=mult, discount_factor=disc, parameter_lr_mul=plm,
             maximum_trajectory_length=max_len, use_penalty=use_penalty, use_TD=use_td, gan='w')
  agent = ((np.zeros((n, 2, 2, 3)), x['new_states'].astype(f64), col('surrogate'), col('penalty')), {})
  critics = [col('fake_logit'), col('fake_input_logit'), col('old_value'), col('new_value')]
  with mock.patch.object(nets_np, 'agent_generator', return_value=agent), mock.patch.object(nets_np, 'critic', side_effect=critics):
    want = nets_np.generator_losses(np.zeros((n, 2, 2, 3)), None, np.zeros((n, d)), 0.3, cfg, {}, None)
  got = R.generator_losses(x, R.GEN_CONSTS, use_td, use_penalty)
  np.testing.assert_allclose(got['losses'], [want['g_loss'], want['v_loss']], rtol=1e-13)
  np.testing.assert_allclose(got['reward'], want['reward'][:, 0], rtol=1e-14)
  np.testing.assert_allclose(got['q'], want['q_value'][:, 0], rtol=1e-14)
  np.testing.assert_allclose(got['coef'][2] * n, want['weight'][:, 0], rtol=1e-13)
  assert (got['scale']['reward'] >= np.abs(got['reward'])).all() and (got['scale']['q'] >= np.abs(got['q'])).all()
  steps = x['new_states'][:, 2]
  assert {float(v) for v in steps} == {max_len - 1, max_len, max_len + 1}


def test_head_and_concat_are_the_oracles_layers():
  hpre, b1, w2, b2 = R.head_inputs((3, 5, 2), 65, 9, 4)
  ref = R.head_fwd(hpre, b1, w2, b2, (3, 5, 2), 1 / 3)
  pre = hpre.astype(f64).sum(axis=0) + b1
  np.testing.assert_allclose(ref['h'], nets_np.lrelu(pre, float(R.LEAK)), rtol=1e-15, atol=1e-15)
  np.testing.assert_allclose(ref['logits'], nets_np.fully_connected(nets_np.lrelu(pre, float(R.LEAK)), w2.astype(f64)[:, None], b2.astype(f64))[:, 0],
                             rtol=1e-13, atol=1e-14)
  assert (pre == 0).any() and (ref['dh'][pre == 0] != 0).any()
  ops = R.head_fwd(hpre, b1, w2, b2, (3, 5, 2), 1 / 3, dtype=f32)
  assert np.array_equal(ops['h'].astype(f64), np.where(pre > 0, pre, (pre.astype(f32) * R.LEAK).astype(f64)))
  img, vec = R.concat_case((2, 16, 12), 3, np.float16, 1)
  out = R.planes_concat(img, vec, 0.5)
  assert out.dtype == f32 and np.array_equal(out[..., :3], img.astype(f32) - f32(0.5))
  assert np.array_equal(out[..., 3:], np.broadcast_to((vec - f32(0.5))[:, None, None, :], out[..., 3:].shape))


# ---- the hand-derived gradients ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_td', [True, False])
@pytest.mark.parametrize('use_penalty', [True, False])
def test_coef_rows_against_autograd_and_differences(use_td, use_penalty):
  n = 13
  x = R.gen_inputs(n, 5, 8)
  ref = R.generator_losses(x, R.GEN_CONSTS, use_td, use_penalty)
  a, mult, disc, plm, max_len = [float(v) for v in R.GEN_CONSTS]
  names = ('fake_logit', 'new_value', 'surrogate', 'penalty', 'old_value')
  t = {k: torch.tensor(x[k].astype(f64), requires_grad=k in names) for k in x}
  stopped, step = t['new_states'][:, 1], t['new_states'][:, 2]
  nv = t['new_value'] * (step <= max_len).double()
  raw = (a + (1 - a) * stopped) * (t['fake_logit'] - t['fake_input_logit']) * mult
  reward = raw - t['penalty'] if use_penalty else raw
  q = reward + (1 - stopped) * disc * nv
  adv = q.detach() - t['old_value']
  routine, weight = (-q * plm, -adv) if use_td else (-reward, -reward)
  g_loss, v_loss = (routine + t['surrogate'] * weight.detach()).mean(), (adv**2).mean()
  np.testing.assert_allclose(ref['losses'], [g_loss.item(), v_loss.item()], rtol=1e-13)
  grads = torch.autograd.grad(g_loss, [t[k] for k in names[:4]], allow_unused=True) + torch.autograd.grad(v_loss, [t['old_value']])
  for row, g in enumerate(grads):
    want = np.zeros(n) if g is None else g.numpy()
    assert R.within(ref['coef'][row], want, 1e-13 * ref['scale']['coef'][row]) <= 1.0, names[row]
    if not use_td and row == 1 or not use_penalty and row == 3:
      assert (ref['coef'][row] == 0).all()

  def loss_rows(cols):  # per image: its g term with the weight frozen + its v term with q frozen, both over N
    y = dict(x, **{k: cols[:, i] for i, k in enumerate(names)})
    out = R.generator_losses(y, R.GEN_CONSTS, use_td, use_penalty)
    routine = -out['q'] * plm if use_td else -out['reward']
    return (routine + y['surrogate'] * ref['frozen']['weight'] + (ref['frozen']['q'] - y['old_value'])**2) / n

  cols = np.stack([x[k].astype(f64) for k in names], axis=1)
  analytic = ref['coef'].T.copy()
  _fd_check(loss_rows, cols, analytic, 'coef')


def test_penalty_gradient_against_autograd_and_differences():
  rng = np.random.default_rng(2)
  g = rng.standard_normal((5, 6))
  g *= (np.array([0.5, 1.2, 3.0, 0.9, 1.05]) / np.sqrt((g**2).sum(axis=1)))[:, None]
  dterm = np.array([0.8, -1.3, 0.9, 0.4, -0.6])
  norm, term = R.penalty_fwd(g)
  dg = g * (dterm * R.penalty_coef(norm))[:, None]
  gt = torch.tensor(g, requires_grad=True)
  nt = torch.sqrt(1e-6 + (gt**2).sum(dim=1))
  (torch.clamp_min(nt - 1.0, 0.0)**2 * torch.tensor(dterm)).sum().backward()
  assert R.within(dg, gt.grad.numpy(), 1e-13 * np.abs(dg)) <= 1.0 and (dg[[0, 3]] == 0).all() and (dg[1] != 0).all()
  _fd_check(lambda v: dterm * R.penalty_fwd(v)[1], g, dg, 'dg')
  # gp_direct's v is the same gradient of scale * term at g = u[..., :3] + ds
  u, ds = R.gp_direct_inputs((2, 3), 6, 4)
  ref = R.gp_direct(u, ds, 0.37)
  g64 = (u[..., :3].astype(f64) + ds).reshape(len(u), -1)
  gt = torch.tensor(g64, requires_grad=True)
  (float(f32(0.37)) * torch.clamp_min(torch.sqrt(1e-6 + (gt**2).sum(dim=1)) - 1.0, 0.0)**2).sum().backward()
  assert R.within(ref['v'].reshape(g64.shape), gt.grad.numpy(), 1e-12 * np.abs(gt.grad.numpy())) <= 1.0
  rows = [3, 4, 6]  # away from the kink (0.5, 3, 1.7): a difference straddling norm = 1 sees both sides
  _fd_check(lambda v: float(f32(0.37)) * R.penalty_fwd(v)[1], g64[rows], ref['v'].reshape(g64.shape)[rows], 'v')


def test_head_gradients_against_autograd_and_differences():
  rows, hidden, inv_n = (3, 5, 4), 9, 1 / 3
  nl = rows[0] + rows[1]
  hpre, b1, w2, b2 = R.head_inputs(rows, hidden, 2, 6)
  thpre = np.random.default_rng(1).standard_normal((3, rows[2], hidden)).astype(f32)
  fwd = R.head_fwd(hpre, b1, w2, b2, rows, inv_n)
  bwd = R.head_bwd(fwd['dh'], fwd['h'], thpre, rows, inv_n)
  dl = R.row_signs(rows, inv_n, f64)
  lk = float(R.LEAK)
  pre0 = hpre.astype(f64).sum(axis=0)
  assert (pre0 + b1 == 0).any()
  t_sum = thpre.astype(f64).sum(axis=0)
  sl_interp = nets_np.lrelu_grad(fwd['h'][nl:], lk)

  def torch_loss(pre, bias, w, b):
    z = pre + bias
    h = 0.5 * (1 + lk) * z + 0.5 * (1 - lk) * z.abs()  # util.py:225-229; abs'(0) = 0 in torch as in TF
    logits = h @ w + b
    return (torch.tensor(dl[:nl]) * logits[:nl]).sum(), logits[nl:].sum(), (torch.tensor(t_sum * sl_interp) * w).sum()

  tp, tb1 = torch.tensor(pre0, requires_grad=True), torch.tensor(b1.astype(f64), requires_grad=True)
  tw, tb2 = torch.tensor(w2.astype(f64), requires_grad=True), torch.tensor(b2.astype(f64), requires_grad=True)
  loss, inner, tangent = torch_loss(tp, tb1, tw, tb2)
  g_pre, = torch.autograd.grad(loss + inner, [tp], retain_graph=True)
  g_b1, g_b2 = torch.autograd.grad(loss, [tb1, tb2], retain_graph=True)
  g_w2, = torch.autograd.grad(loss + tangent, [tw])
  assert R.within(fwd['dh'], g_pre.numpy(), 1e-13 * np.abs(fwd['dh'])) <= 1.0
  assert R.within(bwd['gb1'], g_b1.numpy(), 1e-13 * bwd['scale']['gb1']) <= 1.0
  assert R.within(bwd['gw2'], g_w2.numpy(), 1e-13 * bwd['scale']['gw2']) <= 1.0
  assert R.within(bwd['gb2'], g_b2.numpy(), 1e-13 * bwd['scale']['gb2']) <= 1.0

  def logits_of(pre, bias, w, b):
    return nets_np.lrelu(pre + bias, lk) @ w + b

  w64, b164, b264 = w2.astype(f64), b1.astype(f64), float(b2[0])
  _fd_check(lambda p: dl * logits_of(p, b164, w64, b264), pre0, fwd['dh'], 'dh', h0=1e-5)
  loss_rows = lambda m: np.array([(dl[:nl] * m[:nl]).sum()])
  _fd_check(lambda v: loss_rows(logits_of(pre0, v[0], w64, b264)), b164[None], bwd['gb1'][None], 'gb1', h0=1e-5)
  _fd_check(lambda v: loss_rows(logits_of(pre0, b164, v[0], b264)) + ((t_sum * sl_interp) @ v[0]).sum(), w64[None], bwd['gw2'][None], 'gw2')
  _fd_check(lambda v: loss_rows(logits_of(pre0, b164, w64, v[0, 0])), np.array([[b264]]), bwd['gb2'][None], 'gb2')


# ---- the constants: four times the float32 restatement's error on the inputs of the GPU tests ------------------------
def _four_times(worst, constant, name):
  """constant / 5 <= the restatement's worst error <= constant / 4: the constant IS four times that error, rounded up."""
  assert constant / 5 <= worst <= constant / 4, '%s: the restatement needs %.3g, the constant is %.3g' % (name, worst, constant)


def _np_dtypes():
  return (np.float16, f32)


def penalty_errors():
  worst = dict(norm=0.0, dg=0.0, term=0.0)
  for m in R.PEN_ELEMS:
    g, dterm = R.penalty_images(m, m)
    (n64, t64), (n32, t32) = R.penalty_fwd(g), R.penalty_fwd(g, dtype=f32)
    worst['norm'] = max(worst['norm'], R.needed(n32, n64, n64))
    worst['term'] = max(worst['term'], R.within(t32, t64, R.term_tol(n64, R.C_NORM * n64)))
    assert n32[0] == np.sqrt(f32(1e-6)) and t32[0] == 0
    a, b = R.penalty_bwd(g, n32, dterm), R.penalty_bwd(g, n32, dterm, dtype=f32)
    worst['dg'] = max(worst['dg'], R.needed(b, a, np.abs(a)))
  return worst


def test_penalty_constants_are_four_times_the_restatement_error():
  worst = penalty_errors()
  interp = 0.0
  for shape in R.GP_SHAPES:
    for dt in _np_dtypes():
      real, fake, alpha = R.gp_case(shape, dt, len(shape) + shape[1])
      (_, a, scale), (_, b, _) = R.gp_inputs(real, fake, alpha), R.gp_inputs(real, fake, alpha, dtype=f32)
      interp = max(interp, R.needed(b, a, scale))
  print('float32 restatement, smallest constants that hold: interp %.3g, %s' % (interp, worst))
  _four_times(interp, R.C_INTERP, 'interp'), _four_times(worst['norm'], R.C_NORM, 'norm'), _four_times(worst['dg'], R.C_DG, 'dg')
  # the propagated bound has no constant of its own and leaves term's own two roundings to the factor 4 in the norm's: the
  # restatement sits inside half of it
  assert worst['term'] <= 0.5


def generator_errors():
  worst = dict(rows=0.0, losses=0.0)
  for n in R.GEN_NS:
    for i, (use_td, use_penalty) in enumerate(((1, 1), (1, 0), (0, 1), (0, 0))):
      x = R.gen_inputs(n, (3, 11)[i % 2], 10 * n + i)
      a, b = R.generator_losses(x, R.GEN_CONSTS, use_td, use_penalty), R.generator_losses(x, R.GEN_CONSTS, use_td, use_penalty, dtype=f32)
      for k in ('reward', 'q', 'coef'):
        worst['rows'] = max(worst['rows'], R.needed(b[k], a[k], a['scale'][k]))
      worst['losses'] = max(worst['losses'], R.needed(b['losses'], a['losses'], a['scale']['losses']))
  return worst


def test_generator_constants_are_four_times_the_restatement_error():
  worst = generator_errors()
  print('float32 restatement, smallest constants that hold: %s' % worst)
  _four_times(worst['rows'], R.C_GEN_ROWS, 'rows'), _four_times(worst['losses'], R.C_GEN_LOSS, 'losses')


def head_errors(hidden):
  worst = dict(logits=0.0, dh=0.0, gb1=0.0, gw2=0.0, gb2=0.0)
  for i, (rows, slabs, th_slabs) in enumerate(R.head_cases(hidden)):
    inv_n = 1.0 / max(rows[0], 1)
    hpre, b1, w2, b2 = R.head_inputs(rows, hidden, slabs, 100 * hidden + i)
    a, b = R.head_fwd(hpre, b1, w2, b2, rows, inv_n), R.head_fwd(hpre, b1, w2, b2, rows, inv_n, dtype=f32)
    assert np.array_equal(a['h'].astype(f32), b['h'])
    worst['logits'] = max(worst['logits'], R.needed(b['logits'], a['logits'], a['logit_scale']))
    worst['dh'] = max(worst['dh'], R.needed(b['dh'], a['dh'], np.abs(a['dh'])))
    dh, h, thpre = R.bwd_inputs(rows, hidden, th_slabs, 100 * hidden + i)
    a, b = R.head_bwd(dh, h, thpre, rows, inv_n), R.head_bwd(dh, h, thpre, rows, inv_n, dtype=f32)
    for k in ('gb1', 'gw2', 'gb2'):
      worst[k] = max(worst[k], R.needed(b[k], a[k], a['scale'][k]))
  return worst


def test_head_constants_are_four_times_the_restatement_error():
  worst = {}
  for hidden in R.HEAD_HIDDEN:
    for k, v in head_errors(hidden).items():
      worst[k] = max(worst.get(k, 0.0), v)
  print('float32 restatement over the seven widths, smallest constants that hold: %s' % worst)
  for k, c in (('logits', R.C_LOGIT), ('dh', R.C_DH), ('gb1', R.C_GB1), ('gw2', R.C_GW2), ('gb2', R.C_GB2)):
    _four_times(worst[k], c, k)


def report_errors():
  worst = 0.0
  for i, rows in enumerate(R.REPORT_ROWS):
    logits, norm, term = R.report_inputs(rows, i)
    out64, ema64, scale, ema_scale = R.critic_report(logits, norm, term, rows, 10.0, 0.99, 0.25)
    out32, ema32 = R.critic_report(logits, norm, term, rows, 10.0, 0.99, 0.25, dtype=f32)
    worst = max(worst, R.needed(out32, out64, scale), R.needed(ema32, ema64, ema_scale))
  return worst


def plane_errors():
  worst = dict(plane=0.0, gpnorm=0.0, v=0.0, term=0.0)
  for i, hw in enumerate(R.SUM_PIXELS):
    for planes in R.SUM_PLANES:
      first = (0, 3)[(i + planes) % 2]
      x = (0.02 * np.random.default_rng(planes + i).standard_normal((3,) + hw + (first + planes,))).astype(f32)
      (s64, a64), s32 = R.plane_sums(x, first), R.plane_sums(x, first, dtype=f32)
      worst['plane'] = max(worst['plane'], R.needed(s32, s64, a64))
    for c in (3, 6, 17):
      u, ds = R.gp_direct_inputs(hw, c, 7 * i + c)
      a, b = R.gp_direct(u, ds, 0.37), R.gp_direct(u, ds, 0.37, dtype=f32)
      worst['gpnorm'] = max(worst['gpnorm'], R.needed(b['norm'], a['norm'], a['norm_scale']))
      at = R.gp_direct(u, ds, 0.37, at_norm=b['norm'])
      worst['v'] = max(worst['v'], R.needed(b['v'], at['v'], at['g_abs'] * np.abs(at['coef']).reshape(-1, 1, 1, 1)))
      worst['term'] = max(worst['term'], R.within(b['term'], a['term'], R.term_tol(a['norm'], R.C_GPNORM * a['norm_scale'])))
      assert b['norm'][0] == np.sqrt(f32(1e-6)) and b['term'][0] == 0 and (b['v'][[0, 1, 3]] == 0).all()
      R.check_gp_direct(b, a, 0.37, 'the restatement')
  return worst


def test_report_and_plane_constants_are_four_times_the_restatement_error():
  report, worst = report_errors(), plane_errors()
  print('float32 restatement, smallest constants that hold: report %.3g, %s' % (report, worst))
  _four_times(report, R.C_REPORT, 'report'), _four_times(worst['plane'], R.C_PLANE, 'plane sums')
  _four_times(worst['gpnorm'], R.C_GPNORM, 'gp_direct norm'), _four_times(worst['v'], R.C_V, 'v')
  assert worst['term'] <= 0.5


# ---- the exact zero of gb1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', R.PAIRED_NS)
def test_paired_rows_cancel_exactly_in_the_kernels_order_and_not_in_the_parents(n):
  """The promise of critic_head_bwd_kernel's comment, on the restatements: with pairwise equal slopes every unit of gb1 is
  exactly 0 in the kernel's order for every row count; in the parent's order (a group's real rows, then its fake rows) only
  where a group holds one row per side -- n a power of two up to 64, where both orders are the same additions."""
  hidden = 128
  dh, h, inv_n = R.paired_inputs(n, hidden, n)
  kernel = R.head_bwd(dh, h, None, (n, n, 0), inv_n, dtype=f32)['gb1']
  parent = R.head_bwd(dh, h, None, (n, n, 0), inv_n, dtype=f32, order='parent')['gb1']
  assert (kernel == 0).all()
  one_per_group = n <= 64 and n & (n - 1) == 0
  print('n = %d: non-zero gb1 units of %d in the parent order: %d' % (n, hidden, int((parent != 0).sum())))
  assert (parent == 0).all() == one_per_group
  # a general dh (nothing cancels): where each group holds one row per side the two orders are bit for bit the same
  dh2, h2, _ = R.bwd_inputs((n, n, 0), hidden, 1, n)
  a = R.head_bwd(dh2, h2, None, (n, n, 0), inv_n, dtype=f32)
  b = R.head_bwd(dh2, h2, None, (n, n, 0), inv_n, dtype=f32, order='parent')
  assert np.array_equal(a['gw2'], b['gw2'])
  if one_per_group:
    assert np.array_equal(a['gb1'], b['gb1'])
  unit = 37
  dh, h, inv_n = R.paired_inputs(n, hidden, n, odd_unit=unit)
  odd = R.head_bwd(dh, h, None, (n, n, 0), inv_n, dtype=f32)['gb1']
  assert odd[unit] != 0 and (np.delete(odd, unit) == 0).all()
  if not one_per_group:  # the GPU test's comparison tells the two orders apart
    ref, now = R.head_bwd(dh, h, None, (n, n, 0), inv_n), R.head_bwd(dh, h, None, (n, n, 0), inv_n, dtype=f32)
    reals_first = R.head_bwd(dh, h, None, (n, n, 0), inv_n, dtype=f32, order='parent')
    assert _rejected(lambda v: R.check_head_bwd(v, ref, now, 'gb1 summed reals first'), reals_first)


# ---- the comparisons of the GPU tests must be able to fail -------------------------------------------------------------
def _four(check, want, honest, name):
  assert not _rejected(check, want) and not _rejected(check, honest), name
  assert _rejected(check, np.zeros_like(want)), name + ': zeros passed'
  assert _rejected(check, 0.99 * want), name + ': 0.99 x passed'
  assert _rejected(check, -want), name + ': -x passed'
  one = np.array(want, dtype=f64)
  one.flat[np.abs(one).argmax()] *= 1.001
  assert _rejected(check, one), name + ': one element off by 0.1 % passed'


def test_wrong_penalty_results_are_rejected():
  m = 17280
  g, dterm = R.penalty_images(m, m)
  (n64, t64), (n32, t32) = R.penalty_fwd(g), R.penalty_fwd(g, dtype=f32)
  _four(lambda v: R.check_penalty_fwd(v, t64, n64, t64, 'p'), n64, n32, 'norm')
  _four(lambda v: R.check_penalty_fwd(n64, v, n64, t64, 'p'), t64, t32, 'term')
  dg64, dg32 = R.penalty_bwd(g, n32, dterm), R.penalty_bwd(g, n32, dterm, dtype=f32)
  _four(lambda v: R.check_dg(v, dg64, 'p'), dg64, dg32, 'dg')
  assert _rejected(lambda v: R.check_dg(v, dg64, 'p'), R.penalty_bwd(g, n32, dterm, with_norm=False)), 'dg without 1 / norm passed'
  assert _rejected(lambda v: R.check_dg(v, dg64, 'p'), R.penalty_bwd(g, n32, dterm, dtype=f32, one_trip=True))
  n1, t1 = R.penalty_fwd(g, dtype=f32, one_trip=True)
  assert _rejected(lambda v: R.check_penalty_fwd(v, t64, n64, t64, 'p'), n1)
  real, fake, alpha = R.gp_case(R.GP_SHAPES[3], f32, 1)
  (cat, a, scale), (_, b, _) = R.gp_inputs(real, fake, alpha), R.gp_inputs(real, fake, alpha, dtype=f32)
  _four(lambda v: R.check_interp(v, a, scale, 'p'), a, b, 'interp')
  cat1, b1, _ = R.gp_inputs(real, fake, alpha, dtype=f32, one_trip=True)
  assert _rejected(lambda v: R.check_interp(v, a, scale, 'p'), b1) and not np.array_equal(cat1, cat)
  # gp_direct: the same mutants through its own comparison
  u, ds = R.gp_direct_inputs((41, 25), 6, 3)
  ref, r32 = R.gp_direct(u, ds, 0.37), R.gp_direct(u, ds, 0.37, dtype=f32)
  for key in ('norm', 'term', 'v'):
    _four(lambda v: R.check_gp_direct(dict(r32, **{key: v}), ref, 0.37, 'p'), ref[key], r32[key], 'gp_direct ' + key)
  assert _rejected(lambda v: R.check_gp_direct(v, ref, 0.37, 'p'), R.gp_direct(u, ds, 0.37, dtype=f32, with_norm=False))
  assert _rejected(lambda v: R.check_gp_direct(v, ref, 0.37, 'p'), R.gp_direct(u, ds, 0.37, dtype=f32, one_trip=True))
  x = (0.02 * np.random.default_rng(1).standard_normal((2, 41, 25, 6))).astype(f32)
  sums = R.plane_sums(x, 3)
  _four(lambda v: R.check_plane_sums(v, sums, 'p'), sums[0], R.plane_sums(x, 3, dtype=f32), 'plane sums')
  assert _rejected(lambda v: R.check_plane_sums(v, sums, 'p'), R.plane_sums(x, 3, dtype=f32, one_trip=True))


def test_a_planes_concat_that_stops_after_one_trip_is_rejected():
  """513 x 512 pixels are 1027 blocks of 256 capped to 1024: what a kernel whose blocks leave after their first 256 pixels
  writes (the last 512 pixels stay NaN) fails the GPU test's bit comparison; at 4096 pixels there is no second trip."""
  img, vec = R.concat_case(R.CONCAT_BIG, 1, np.float16, 1 + R.CONCAT_BIG[1])
  want = R.planes_concat(img, vec, 0.5)
  R.check_bit_equal(want.copy(), want, 'honest')
  assert _rejected(lambda v: R.check_bit_equal(v, want, 'p'), R.planes_concat(img, vec, 0.5, one_trip=True))
  off = want.copy()
  off[0, -1, -1, 3] = np.nextafter(off[0, -1, -1, 3], f32(1))
  assert _rejected(lambda v: R.check_bit_equal(v, want, 'p'), off), 'one element off by one ulp passed'
  img, vec = R.concat_case(R.CONCAT_SHAPES[-1], 1, np.float16, 1)
  assert np.array_equal(R.planes_concat(img, vec, 0.5, one_trip=True), R.planes_concat(img, vec, 0.5))


@pytest.mark.parametrize('use_td', [True, False])
def test_wrong_generator_results_are_rejected(use_td):
  x = R.gen_inputs(700, 11, 3)
  ref = R.generator_losses(x, R.GEN_CONSTS, use_td, True)
  r32 = R.generator_losses(x, R.GEN_CONSTS, use_td, True, dtype=f32)
  for key in ('reward', 'q', 'losses'):
    _four(lambda v: R.check_generator(dict(r32, **{key: v}), ref, 'p'), ref[key], r32[key], key)
  for row in range(5):
    if (ref['coef'][row] == 0).all():
      continue

    def check(v):
      coef = ref['coef'].copy()
      coef[row] = v
      R.check_generator(dict(r32, coef=coef), ref, 'p')

    _four(check, ref['coef'][row], r32['coef'][row], 'coef row %d' % row)
  check = lambda v: R.check_generator(v, ref, 'p')
  assert _rejected(check, R.generator_losses(x, R.GEN_CONSTS, use_td, True, dtype=f32, keep_ge=True)), 'keep with >='
  assert _rejected(check, R.generator_losses(x, R.GEN_CONSTS, use_td, True, dtype=f32, gated=False)), 'reward without the gate'
  assert _rejected(check, R.generator_losses(x, R.GEN_CONSTS, use_td, True, dtype=f32, one_trip=True)), 'one trip'
  ge = R.generator_losses(x, R.GEN_CONSTS, use_td, True, dtype=f32, keep_ge=True)
  assert _rejected(lambda v: R.check_generator(dict(r32, q=v), ref, 'p'), ge['q'])  # (q carries the bootstrap value in both modes)


def test_wrong_head_results_are_rejected():
  rows, hidden, inv_n = (130, 130, 3), 65, 1 / 130
  hpre, b1, w2, b2 = R.head_inputs(rows, hidden, 9, 1)
  ref, r32 = R.head_fwd(hpre, b1, w2, b2, rows, inv_n), R.head_fwd(hpre, b1, w2, b2, rows, inv_n, dtype=f32)
  for key in ('logits', 'dh'):
    _four(lambda v: R.check_head_fwd(dict(r32, **{key: v}), ref, r32, 'p'), ref[key], r32[key], key)
  short = R.head_fwd(hpre, b1, w2, b2, rows, inv_n, dtype=f32, slabs_read=8)
  assert _rejected(lambda v: R.check_head_fwd(v, ref, r32, 'p'), short), 'a slab left out passed'
  dh, h, thpre = R.bwd_inputs(rows, hidden, 9, 2)
  ref, r32 = R.head_bwd(dh, h, thpre, rows, inv_n), R.head_bwd(dh, h, thpre, rows, inv_n, dtype=f32)
  _four(lambda v: R.check_head_bwd(dict(r32, gw2=v), ref, r32, 'p'), ref['gw2'], r32['gw2'], 'gw2')
  uneven = (3, 5, 0)
  dh3, h3, _ = R.bwd_inputs(uneven, hidden, 1, 3)
  ref3, r3 = R.head_bwd(dh3, h3, None, uneven, 1 / 3), R.head_bwd(dh3, h3, None, uneven, 1 / 3, dtype=f32)
  _four(lambda v: R.check_head_bwd(dict(r3, gb2=v), ref3, r3, 'p'), ref3['gb2'], r3['gb2'], 'gb2')
  _four(lambda v: R.check_head_bwd(dict(r32, gb1=v), ref, r32, 'p'), r32['gb1'], r32['gb1'], 'gb1')
  assert _rejected(lambda v: R.check_head_bwd(v, ref, r32, 'p'), R.head_bwd(dh, h, thpre, rows, inv_n, dtype=f32, th_read=8))
  assert _rejected(lambda v: R.check_head_bwd(v, ref, r32, 'p'), R.head_bwd(dh, h, thpre, rows, inv_n, dtype=f32, order='parent'))
  rows = (130, 130, 70)
  logits, norm, term = R.report_inputs(rows, 6)
  ref = R.critic_report(logits, norm, term, rows, 10.0, 0.99, 0.25)
  out32, ema32 = R.critic_report(logits, norm, term, rows, 10.0, 0.99, 0.25, dtype=f32)
  _four(lambda v: R.check_report(v, ema32, ref, 'p'), ref[0], out32, 'report')
  out1, ema1 = R.critic_report(logits, norm, term, rows, 10.0, 0.99, 0.25, dtype=f32, one_trip=True)
  assert _rejected(lambda v: R.check_report(v, ema32, ref, 'p'), out1)
  assert _rejected(lambda v: R.check_report(out32, v, ref, 'p'), np.float64(0.25)), 'an ema that did not move passed'
