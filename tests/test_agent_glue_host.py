"""CPU: the reference of the agent step's selection and head-regression kernels (tests/_agent_glue_ref.py) checked against
the oracle it is built on, its hand-derived gradients against central differences and torch's float64 autograd, the float32
restatement's error against the constants the GPU tests use (each constant is at least 4 x that error), and the comparison
helper against wrong results it has to reject."""
import math

import numpy as np
import pytest
import torch

from oracle import agent_np
from oracle import filters_np as fnp
from tests import _agent_glue_ref as R
from tests._glue_checks import fd_check as _fd_check, rejected as _rejected

f32, f64 = np.float32, np.float64


def _case(k, index):
  c = R.select_cases(k)[index]
  return c, R.select_inputs(k, c['n'], c['eps'], c['seed'], c['trailing'])


# ---- the reference is the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', R.SELECT_KS)
def test_select_fwd_float64_is_the_oracle(k):
  for index in (8, 9, 18, 27):  # n = 63 / 64, both modes, three exploration values, trailing columns or none
    c, x = _case(k, index)
    eps, c_e, c_u, c_s, steps = [float(v) for v in c['consts']]
    ref = R.select_fwd(x['logits'], x['noise'], x['states'], c['progress'], c['consts'], c['is_train'])
    l64, s64 = x['logits'].astype(f64), x['states'].astype(f64)
    pdf, ent, sel, onehot, sur = agent_np.action_selection(l64, x['noise'].astype(f64)[:, None], c['is_train'], eps)
    head, usage, last, sub = agent_np.new_states(s64[:, :3 + k], onehot, steps)
    pen = agent_np.penalty(np.zeros((c['n'], 2, 2, 3)), ent, usage, last, sub, float(f32(c['progress'])), k, c_e, c_u, c_s)
    assert (ref['selected'] == sel).all() and (ref['onehot'] == onehot).all()
    for name, want in (('pdf', pdf), ('entropy', ent[:, 0]), ('surrogate', sur[:, 0]), ('penalty_base', pen[:, 0])):
      assert np.array_equal(ref[name], want), name
    assert np.array_equal(ref['new_states'][:, :3 + k], head) and np.array_equal(ref['new_states'][:, 3 + k:], s64[:, 3 + k:])
    assert ref['new_states'].shape == s64.shape
    if c['is_train']:
      assert (sel == x['target']).all() and sel[0] == -1 and ref['surrogate'][0] == 0 and not onehot[0].any()
    # the operation-by-operation restatement states the same formula: run in float64 it is the definition up to rounding
    ops = R._select_fwd_ops(x['logits'], x['noise'], x['states'], c['progress'], c['consts'], c['is_train'], f64)
    assert (ops['selected'] == sel).all() and np.array_equal(ops['new_states'], ref['new_states'])
    for name in ('pdf', 'entropy', 'surrogate', 'penalty_base'):
      np.testing.assert_allclose(ops[name], ref[name], rtol=1e-13, atol=1e-14, err_msg=name)


@pytest.mark.parametrize('fid', range(9))
def test_heads_fwd_is_regress_packed_row_by_row(fid):
  rng = np.random.default_rng(fid)
  ids = (fid, (fid + 3) % 9)
  raws = [rng.standard_normal((7, fnp.NUM_PARAMS[i] + 6)) * 1.5 for i in ids]
  selected = np.array([0, 1, -1, 0, 0, 1, -1])
  got = R.heads_fwd(raws, ids, R.shipped_ranges(), selected)
  for r, j in enumerate(selected):
    want = np.zeros(R.MAX_PARAMS)
    if j >= 0:
      p = fnp.NUM_PARAMS[ids[j]]
      # (the cfg heads_fwd rebuilds from the float32 ranges differs from DEFAULT_CFG by float32 rounding of 0.9, 1.1 and log 3)
      want[:p] = fnp.regress_packed(ids[j], raws[j][r:r + 1, :p])[0]
    np.testing.assert_allclose(got[r], want, rtol=3e-7, atol=0)
    assert (got[r, fnp.NUM_PARAMS[ids[j]] if j >= 0 else 0:] == 0).all()


# ---- the hand-derived gradients ----------------------------------------------------------------------------------------
def _torch_select_loss(l, ids, gs, gq, eps, c_e, progress, k):
  sm = torch.softmax(l, dim=1)
  b = (sm + 1e-37) * (1 - eps) + eps / k
  p = b / (b.sum(dim=1, keepdim=True) + 1e-30)
  ent = -(p * p.log()).sum(dim=1)
  picked = p.gather(1, ids.clamp(min=0)[:, None])[:, 0]
  sur = torch.where(ids >= 0, (picked + 1e-10).log(), torch.zeros_like(picked))
  return gs * sur + gq * ((1 - progress) * c_e * (math.log(k) - ent))


@pytest.mark.parametrize('k', R.SELECT_KS)
@pytest.mark.parametrize('eps', [0.05, 0.0, 0.3, 1.0])
def test_select_bwd_against_differences_and_autograd(k, eps):
  n = 12
  x = R.select_inputs(k, n, eps, 31 * k + 7, 0)
  logits = x['logits'].astype(f64)
  logits[2] = np.linspace(0, 30, k)  # (the underflowing row has no derivative a difference could see)
  logits[3] -= 1e4
  consts = np.array([eps, 0.07, 1.3, 0.6, 5], dtype=f32)
  progress = 0.3
  fwd = R.select_fwd(logits, x['noise'], x['states'], progress, consts, 1)
  ids = fwd['selected']
  gs, gq = x['d_surrogate'].astype(f64), x['d_penalty_base'].astype(f64)
  got, scale = R.select_bwd(logits, ids, progress, consts, gs, gq)
  assert got.dtype == f64 and (scale >= np.abs(got) * (1 - 1e-12)).all()
  if eps == 1.0 or k == 1:
    assert (got == 0).all()

  def loss_rows(l):
    pdf, ent, _, _, _ = agent_np.action_selection(l, np.zeros((n, 1)), 0, float(f32(eps)))
    rows = np.arange(n)
    sur = np.where(ids >= 0, np.log(pdf[rows, np.maximum(ids, 0)] + 1e-10), 0.0)
    pen = (1.0 - float(f32(progress))) * float(consts[1]) * (math.log(k) - ent[:, 0])
    return gs * sur + gq * pen

  _fd_check(loss_rows, logits, got, 'd_logits')
  lt = torch.tensor(logits, requires_grad=True)
  _torch_select_loss(lt, torch.tensor(ids, dtype=torch.int64), torch.tensor(gs), torch.tensor(gq), float(f32(eps)), float(consts[1]),
                     float(f32(progress)), k).sum().backward()
  assert R.worst_ratio(got, lt.grad.numpy(), 0, 1e-13, scale) <= 1.0


def _torch_regress(fid, x, ranges):
  er, lg, tl, th, tb, cl, ch, cb, eb = [float(v) for v in ranges]
  t01 = lambda v: torch.tanh(v) * 0.5 + 0.5
  if fid == 0:
    return t01(x + eb) * (2 * er) - er
  if fid == 1:
    return torch.exp(t01(x) * (2 * lg) - lg)
  if fid == 2:
    s = torch.exp(t01(x * torch.tensor([0.0, 1.0, 1.0], dtype=x.dtype)) - 0.5)
    return s / (1e-5 + (s * torch.tensor(fnp.LUM_W, dtype=x.dtype)).sum(dim=1, keepdim=True))
  if fid in (3, 6, 8):
    return torch.sigmoid(x)
  if fid == 4:
    return t01(x + tb) * (th - tl) + tl
  if fid == 5:
    return torch.tanh(x)
  return t01(x + cb) * (ch - cl) + cl


@pytest.mark.parametrize('ranges', [R.shipped_ranges(), R.biased_ranges()], ids=['shipped', 'biased'])
@pytest.mark.parametrize('heads', ['nine_with_level', 'tone_twice'])
def test_heads_bwd_against_differences_and_autograd(heads, ranges):
  ids = R.HEAD_LISTS[heads]
  n = 2 * (len(ids) + 1)
  raws, selected, dparams = R.heads_inputs(ids, n, 6, 5)
  raws = [r.astype(f64) for r in raws]
  for r in raws:
    r[len(ids) + 1:] *= 0.1  # (the pass of 20s: mildly saturated instead, so that a difference still sees the slope)
  dp = dparams.astype(f64)
  got, scale = R.heads_bwd(raws, ids, ranges, selected, dp)
  r64 = ranges.astype(f64)
  for j, fid in enumerate(ids):
    p = fnp.NUM_PARAMS[fid]
    assert (got[j][selected != j] == 0).all() and (got[j][:, p:] == 0).all()
    assert (scale[j] >= np.abs(got[j]) * (1 - 1e-12)).all()

    def loss_rows(xj):
      params = R.heads_fwd(raws[:j] + [xj] + raws[j + 1:], ids, ranges, selected)
      return (params * dp).sum(axis=1)

    _fd_check(loss_rows, raws[j], got[j], 'd raw of head %d (filter %d)' % (j, fid))
    rows = np.flatnonzero(selected == j)
    xt = torch.tensor(raws[j][rows, :p], requires_grad=True)
    out = _torch_regress(fid, xt, r64)
    np.testing.assert_allclose(out.detach().numpy(), R.heads_fwd(raws, ids, ranges, selected)[rows, :p], rtol=1e-12, atol=1e-15)
    (out * torch.tensor(dp[rows, :p])).sum().backward()
    assert R.worst_ratio(got[j][rows, :p], xt.grad.numpy(), 0, 1e-13, scale[j][rows, :p]) <= 1.0


# ---- float32 and float64 oracles pick the same ids; the constants are four times the restatement's error ---------------
def _restatement_errors(k):
  worst = dict(pdf=0.0, entropy=0.0, surrogate=0.0, penalty_base=0.0, d_logits=0.0)
  for c in R.select_cases(k):
    x = R.select_inputs(k, c['n'], c['eps'], c['seed'], c['trailing'])
    args = (x['logits'], x['noise'], x['states'], c['progress'], c['consts'], c['is_train'])
    a, b = R.select_fwd(*args), R.select_fwd(*args, dtype=f32)
    assert all(v.dtype == (np.int32 if name == 'selected' else f32) for name, v in b.items())
    assert (a['selected'] == b['selected']).all(), 'the float32 and float64 oracles disagree on an id'
    assert np.array_equal(a['onehot'], b['onehot']) and np.array_equal(a['new_states'], b['new_states'])
    for name, r in (('pdf', R.needed_constant(b['pdf'], a['pdf'], 1, 0)),
                    ('entropy', R.needed_constant(b['entropy'], a['entropy'], 1, 1)),
                    ('surrogate', R.needed_constant(b['surrogate'], a['surrogate'], 1, 1)),
                    ('penalty_base', R.needed_constant(b['penalty_base'], a['penalty_base'], 0, a['penalty_scale']))):
      worst[name] = max(worst[name], r)
    back = (x['logits'], a['selected'], c['progress'], c['consts'], x['d_surrogate'], x['d_penalty_base'])
    (g64, scale), (g32, _) = R.select_bwd(*back), R.select_bwd(*back, dtype=f32)
    worst['d_logits'] = max(worst['d_logits'], R.needed_constant(g32, g64, 1, scale))
  return worst


@pytest.mark.parametrize('k', R.SELECT_KS)
def test_selection_constants_are_four_times_the_restatement_error(k):
  worst = _restatement_errors(k)
  print('K = %d: float32 restatement, smallest constant that holds: %s' % (k, worst))
  assert worst['pdf'] <= R.C_PDF / 4
  assert worst['entropy'] <= R.C_ENTROPY / 4
  assert worst['surrogate'] <= R.C_SURROGATE / 4
  assert worst['penalty_base'] <= R.C_PENALTY / 4
  assert worst['d_logits'] <= R.C_DLOGITS / 4


def _heads_cases():
  for name, ids in R.HEAD_LISTS.items():
    for n in R.HEAD_NS:
      for mask_features in (6, 0):
        for rname, ranges in (('shipped', R.shipped_ranges()), ('biased', R.biased_ranges())):
          yield name, ids, n, mask_features, rname, ranges


def test_params_constant_is_four_times_the_restatement_error():
  worst = 0.0
  for name, ids, n, mask_features, rname, ranges in _heads_cases():
    raws, selected, _ = R.heads_inputs(ids, n, mask_features, 7)
    a, b = R.heads_fwd(raws, ids, ranges, selected), R.heads_fwd(raws, ids, ranges, selected, dtype=f32)
    assert b.dtype == f32 and np.isfinite(a).all()
    worst = max(worst, R.needed_constant(b, a, 1, 1))
  print('heads: float32 restatement, smallest constant that holds: %.3g' % worst)
  assert worst <= R.C_PARAMS / 4


# ---- the comparisons of the GPU tests must be able to fail -------------------------------------------------------------
def test_wrong_selection_results_are_rejected():
  k = 8
  c, x = _case(k, 10)  # n = 63, exploration 0, training mode, progress 0.3
  assert c['eps'] == 0 and c['is_train'] == 1 and c['progress'] < 1
  args = (x['logits'], x['noise'], x['states'], c['progress'], c['consts'], 1)
  ref, r32 = R.select_fwd(*args), R.select_fwd(*args, dtype=f32)
  back = (x['logits'], ref['selected'], c['progress'], c['consts'], x['d_surrogate'], x['d_penalty_base'])
  (g, scale), (g32, _) = R.select_bwd(*back), R.select_bwd(*back, dtype=f32)
  checks = {
      'pdf': (lambda v: R.assert_close(v, ref['pdf'], R.C_PDF, 0, 0, 'pdf'), r32['pdf']),
      'entropy': (lambda v: R.assert_close(v, ref['entropy'], R.C_ENTROPY, R.C_ENTROPY, 1, 'entropy'), r32['entropy']),
      'surrogate': (lambda v: R.assert_close(v, ref['surrogate'], R.C_SURROGATE, R.C_SURROGATE, 1, 'surrogate'), r32['surrogate']),
      'penalty_base': (lambda v: R.assert_close(v, ref['penalty_base'], 0, R.C_PENALTY, ref['penalty_scale'], 'penalty_base'),
                       r32['penalty_base']),
      'd_logits': (lambda v: R.assert_close(v, g, R.C_DLOGITS, R.C_DLOGITS, scale, 'd_logits'), g32),
  }
  for name, (check, honest) in checks.items():
    want = g if name == 'd_logits' else ref[name]
    assert not _rejected(check, want) and not _rejected(check, honest), name
    assert _rejected(check, np.zeros_like(want)), name + ': zeros passed'
    assert _rejected(check, 0.99 * want), name + ': 0.99 x passed'
    assert _rejected(check, -want), name + ': -x passed'
    one = np.array(want, dtype=f64)
    one.flat[np.abs(one).argmax()] *= 1.001
    assert _rejected(check, one), name + ': one element off by 0.1 % passed'
  # a surrogate without the + 1e-10 (row 2 selected a probability of exp(-120 / 7))
  rows = np.arange(c['n'])
  no_tiny = np.where(ref['selected'] >= 0, np.log(ref['pdf'][rows, np.maximum(ref['selected'], 0)]), 0.0)
  assert ref['pdf'][2, ref['selected'][2]] < 1e-7
  assert _rejected(checks['surrogate'][0], no_tiny)
  assert _rejected(checks['d_logits'][0], R.select_bwd(*back, tiny=0.0)[0])
  # d_logits without the entropy path (row 0 selected nothing: its gradient is the entropy path alone)
  assert ref['selected'][0] == -1 and np.abs(g[0]).max() > 0
  assert _rejected(checks['d_logits'][0], R.select_bwd(*back, entropy_term=False)[0])


def test_wrong_head_results_are_rejected():
  ids, ranges = R.HEAD_LISTS['default8'], R.biased_ranges()
  raws, selected, dparams = R.heads_inputs(ids, 19, 6, 7)
  ref = R.heads_fwd(raws, ids, ranges, selected)
  check_p = lambda v: R.assert_close(v, ref, R.C_PARAMS, R.C_PARAMS, 1, 'params')
  assert not _rejected(check_p, ref) and not _rejected(check_p, R.heads_fwd(raws, ids, ranges, selected, dtype=f32))
  for bad, what in ((np.zeros_like(ref), 'zeros'), (0.99 * ref, '0.99 x'), (-ref, '-x')):
    assert _rejected(check_p, bad), what
  # a tone / colour / exposure regressor that forgets its bias
  forgot = R.heads_fwd(raws, ids, ranges, selected, zero_bias=True)
  for j in (0, 4, 7):
    rows = selected == j
    assert rows.any() and _rejected(lambda v: R.assert_close(v[rows], ref[rows], R.C_PARAMS, R.C_PARAMS, 1, 'params'), forgot), j
  g, scale = R.heads_bwd(raws, ids, ranges, selected, dparams)
  for j in range(len(ids)):
    check = lambda v: R.assert_close(v, g[j], 0, R.C_DRAW, scale[j], 'd raw')
    assert not _rejected(check, g[j])
    for bad, what in ((np.zeros_like(g[j]), 'zeros'), (0.99 * g[j], '0.99 x'), (-g[j], '-x')):
      assert _rejected(check, bad), (j, what)
  # white balance without the cross term dot * inv^2 * w_k (dparams[:, 0] != 0 on its rows)
  assert (dparams[selected == 2, 0] != 0).all()
  dropped, _ = R.heads_bwd(raws, ids, ranges, selected, dparams, wb_cross_term=False)
  assert _rejected(lambda v: R.assert_close(v, g[2], 0, R.C_DRAW, scale[2], 'd raw'), dropped[2])
