"""The reference of ``expo_agent_select_fwd / _bwd`` and ``expo_heads_regress_fwd / _bwd`` (include/exposure_hip.h): float64
definitions built on ``oracle/agent_np.py`` and ``oracle/filters_np.py``, hand-derived float64 gradients, float32
restatements operation for operation (they say what float32 rounding alone costs: the tolerances of the GPU tests are
four times their worst error), the error models' comparison helper, and the inputs both test modules run.

TEST INFRASTRUCTURE ONLY, NumPy only."""
import math

import numpy as np

from oracle import agent_np
from oracle import filters_np as fnp

f32, f64 = np.float32, np.float64
MAX_PARAMS = 24
MAX_HEADS = 16


# ---- comparison: |got - ref| <= c_rel |ref| + c_abs scale, every element finite ---------------------------------------
def worst_ratio(got, ref, c_rel, c_abs, scale):
  """max over the elements of err / tol, tol = c_rel |ref| + c_abs scale + 2^-126: below float32's smallest normal number
  a float32 result has no relative precision left (and hardware may flush it to zero).  Anything non-finite: infinity."""
  got, ref = np.asarray(got, dtype=f64), np.asarray(ref, dtype=f64)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  if got.size == 0:
    return 0.0
  tol = c_rel * np.abs(ref) + c_abs * np.broadcast_to(np.asarray(scale, dtype=f64), ref.shape) + 2.0**-126
  with np.errstate(invalid='ignore'):
    ratio = np.abs(got - ref) / tol
  ratio = np.where(np.isfinite(got) & np.isfinite(ratio), ratio, np.inf)
  return float(ratio.max())


def needed_constant(got, ref, rel, scale):
  """The smallest C with |got - ref| <= C (rel |ref| + scale) + 2^-126 on every element (how the restatement is measured)."""
  got, ref = np.asarray(got, dtype=f64), np.asarray(ref, dtype=f64)
  excess = np.maximum(np.abs(got - ref) - 2.0**-126, 0.0)
  with np.errstate(divide='ignore', invalid='ignore'):
    c = np.where(excess == 0, 0.0, excess / (rel * np.abs(ref) + np.broadcast_to(np.asarray(scale, dtype=f64), ref.shape)))
  assert np.isfinite(got).all()
  return float(c.max()) if c.size else 0.0


def assert_close(got, ref, c_rel, c_abs, scale, what):
  r = worst_ratio(got, ref, c_rel, c_abs, scale)
  assert r <= 1.0, '%s: worst err / tol = %.3g (c_rel %.3g, c_abs %.3g)' % (what, r, c_rel, c_abs)
  return r


# The constants ("The agent step's glue"): 4 x the float32 restatement's worst error against the float64
# reference over the inputs below, rounded up (tests/test_agent_glue_host.py recomputes that error and holds it under a
# quarter of each).  Every tolerance also carries worst_ratio's 2^-126.      restatement's worst        model
C_PDF = 1.6e-5        # 3.86e-6 (the rounding of l - max, up to 120 x 2^-24, in the exponent)   C |ref|
C_ENTROPY = 7.5e-7    # 1.76e-7                                                                  C (|ref| + 1)
C_SURROGATE = 7.5e-7  # 1.82e-7                                                                  C (|ref| + 1)
C_PENALTY = 6e-7      # 1.41e-7                                          C (sum of the absolute terms of penalty_base)
C_DLOGITS = 4.5e-5    # 1.07e-5                    c_rel |ref| + c_abs scale, c_rel = c_abs = C (select_bwd's scale)
C_PARAMS = 1.1e-6     # 2.63e-7                                                                  C (|ref| + 1)
# d raw: no restatement; the longest expression (white balance, heads_bwd's docstring) is 61 roundings of 2^-24 -> 64
C_DRAW = 4 * 64 * 2.0**-24  # |err| <= C (sum of the absolute terms of the output)


# ---- selection --------------------------------------------------------------------------------------------------------
def _seq_sum(cols, dt):
  """0 + c0 + c1 + ... left to right in ``dt`` (the kernels' accumulation loops)."""
  total = np.zeros_like(cols[0], dtype=dt)
  for c in cols:
    total = total + c
  return total


def _pdf_ops(logits, eps, dt):
  """softmax -> exploration mix -> renormalisation in the kernel's operation order; returns (pdf, softmax, tot)."""
  l = np.asarray(logits).astype(dt)
  k = l.shape[1]
  one = dt(1)
  e = np.exp(l - l.max(axis=1, keepdims=True))
  den = _seq_sum([e[:, i] for i in range(k)], dt)
  sm = e / den[:, None]
  b = (sm + dt(1e-37)) * (one - eps) + eps * one / dt(k)
  tot = _seq_sum([b[:, i] for i in range(k)], dt) + dt(1e-30)
  return b / tot[:, None], sm, tot


def _select_fwd_ops(logits, noise, states, progress, consts, is_train, dt):
  """The forward, operation for operation in ``dt`` (float32: what the kernel computes up to its library functions)."""
  eps, c_e, c_u, c_s, test_steps = [dt(v) for v in np.asarray(consts, dtype=f32)]
  progress = dt(f32(progress))
  states = np.asarray(states).astype(dt)
  k = np.asarray(logits).shape[1]
  one = dt(1)
  pdf, _, _ = _pdf_ops(logits, eps, dt)
  ent = _seq_sum([-pdf[:, i] * np.log(pdf[:, i]) for i in range(k)], dt)
  rnd = agent_np.pdf_sample(pdf, np.asarray(noise, dtype=f32).astype(dt)[:, None])
  selected = (rnd if is_train else np.argmax(pdf, axis=1)).astype(np.int32)
  onehot = (selected[:, None] == np.arange(k)[None, :]).astype(dt)
  step = states[:, 2]
  submitted = (np.abs(step + one - test_steps) < dt(1e-4)).astype(dt)
  usage = states[:, 3:3 + k]
  new_states = np.concatenate([submitted[:, None], submitted[:, None], (step + one)[:, None], np.maximum(usage, onehot),
                               states[:, 3 + k:]], axis=1)
  usage_pen = _seq_sum([usage[:, i] * onehot[:, i] for i in range(k)], dt)
  rows = np.arange(len(selected))
  with np.errstate(divide='ignore'):
    surrogate = np.where(selected >= 0, np.log(pdf[rows, np.maximum(selected, 0)] + dt(1e-10)), dt(0)).astype(dt)
  ent_pen = (one - progress) * c_e * (-ent + np.log(dt(k)))
  pen = ent_pen + usage_pen * c_u + (one - submitted) * submitted * c_s
  return dict(pdf=pdf, entropy=ent, selected=selected, onehot=onehot, surrogate=surrogate, new_states=new_states,
              penalty_base=pen)


def select_fwd(logits, noise, states, progress, consts, is_train, dtype=f64):
  """expo_agent_select_fwd.  ``consts`` = (exploration, exploration_penalty, filter_usage_penalty, early_stop_penalty,
  test_steps) and ``progress`` are taken at their float32 values (what the kernel is handed).  float64: the definition,
  ``agent_np.action_selection`` + ``new_states`` + ``penalty`` without its image term, trailing state columns copied
  through; float32: every operation rounded in float32, in the kernel's order.  Returns a dict; ``penalty_scale`` (float64
  only) is the sum of the absolute terms of penalty_base."""
  if np.dtype(dtype) == np.float32:
    return _select_fwd_ops(logits, noise, states, progress, consts, is_train, f32)
  eps, c_e, c_u, c_s, test_steps = [float(v) for v in np.asarray(consts, dtype=f32)]
  progress = float(f32(progress))
  logits, states = np.asarray(logits, dtype=f64), np.asarray(states, dtype=f64)
  n, k = logits.shape
  z = np.asarray(noise, dtype=f32).astype(f64)[:, None]
  pdf, ent, selected, onehot, surrogate = agent_np.action_selection(logits, z, int(bool(is_train)), exploration=eps)
  head, usage_pen, is_last, submitted = agent_np.new_states(states[:, :3 + k], onehot, test_steps=test_steps)
  no_image = np.zeros((n, 1, 1, 3))
  pen = agent_np.penalty(no_image, ent, usage_pen, is_last, submitted, progress, k=k, exploration_penalty=c_e,
                         filter_usage_penalty=c_u, early_stop_penalty=c_s)
  scale = abs(1.0 - progress) * c_e * (np.abs(ent) + math.log(k)) + usage_pen * c_u
  return dict(pdf=pdf, entropy=ent[:, 0], selected=selected, onehot=onehot, surrogate=surrogate[:, 0],
              new_states=np.concatenate([head, states[:, 3 + k:]], axis=1), penalty_base=pen[:, 0],
              penalty_scale=scale[:, 0])


def select_bwd(logits, selected, progress, consts, d_surrogate, d_penalty_base, dtype=f64, entropy_term=True, tiny=1e-10):
  """expo_agent_select_bwd: (d_logits, scale).  With L = sum_n gs_n surrogate_n + gq_n penalty_base_n, per image

    surrogate = log(p_id + 1e-10), penalty_base = (1 - progress) c_e (log K - H) + ..., H = -sum_i p_i log p_i
      gp_i  = dL/dp_i  = gq (1 - progress) c_e (log p_i + 1) + [i == id] gs / (p_i + 1e-10)
    p = b / tot, tot = sum_j b_j + 1e-30:   dp_i/db_j = delta_ij / tot - b_i / tot^2
      dL/db_j = (gp_j - sum_i gp_i p_i) / tot
    b = (s + 1e-37)(1 - eps) + eps / K:
      gsm_j = dL/ds_j = dL/db_j (1 - eps)
    s = softmax(l):  ds_j/dl_i = s_j (delta_ij - s_i)
      d_logits_i = s_i (gsm_i - sum_j gsm_j s_j)

  ``scale_i = s_i (|gsm_i| + sum_j |gsm_j| s_j)``: the sum of the absolute terms of d_logits_i.  float32 (the tolerances'
  restatement) follows the kernel's operation order.  ``entropy_term=False`` / ``tiny=0`` are the mutants of
  tests/test_agent_glue_host.py."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  eps, c_e = [dt(v) for v in np.asarray(consts, dtype=f32)[:2]]
  progress, one = dt(f32(progress)), dt(1)
  k = np.asarray(logits).shape[1]
  selected = np.asarray(selected)
  gs, gq = np.asarray(d_surrogate, dtype=f32).astype(dt), np.asarray(d_penalty_base, dtype=f32).astype(dt)
  if dt is f64:
    l = np.asarray(logits, dtype=f64)
    sm = agent_np.softmax(l)
    b = (sm + 1e-37) * (one - eps) + eps / k
    tot = b.sum(axis=1) + 1e-30
    p = b / tot[:, None]
  else:
    p, sm, _ = _pdf_ops(logits, eps, dt)
    tot = _seq_sum([(sm[:, i] + dt(1e-37)) * (one - eps) + eps * one / dt(k) for i in range(k)], dt) + dt(1e-30)
  g_h = gq * (one - progress) * c_e * dt(-1) if entropy_term else np.zeros_like(gq)
  hit = selected[:, None] == np.arange(k)[None, :]
  gp = g_h[:, None] * (-(np.log(p) + one)) + np.where(hit, gs[:, None] / (p + dt(tiny)), dt(0))
  dot = _seq_sum([gp[:, i] * p[:, i] for i in range(k)], dt)
  gsm = (gp - dot[:, None]) / tot[:, None] * (one - eps)
  dot2 = _seq_sum([gsm[:, i] * sm[:, i] for i in range(k)], dt)
  d_logits = sm * (gsm - dot2[:, None])
  scale = sm * (np.abs(gsm) + (np.abs(gsm) * sm).sum(axis=1, keepdims=True))
  assert d_logits.dtype == dt
  return d_logits, scale.astype(f64)


def midpoint_noise(pdf64, rng, min_width=1e-4):
  """Per row a uniform draw that lands in the middle of a cdf interval at least ``min_width`` wide (the interval picked
  at random), computed in float64 and rounded to float32; returns (noise, the interval's index)."""
  pn = pdf64 / (pdf64.sum(axis=1, keepdims=True) + 1e-36)
  edges = np.concatenate([np.zeros((len(pn), 1)), np.cumsum(pn, axis=1)], axis=1)
  noise, target = np.zeros(len(pn), dtype=f32), np.zeros(len(pn), dtype=np.int32)
  for r in range(len(pn)):
    wide = np.flatnonzero(pn[r] >= min_width)
    j = int(rng.choice(wide))
    noise[r], target[r] = f32(0.5 * (edges[r, j] + edges[r, j + 1])), j
  return noise, target


def select_inputs(k, n, eps, seed, trailing=0):
  """Logits (N(0, 3); from row 1 on an all-equal row, a ``linspace(0, 120, K)`` row whose softmax underflows and a row
  around 1e4), states (steps 0..5, random 0/1 usage with one row all used, random reward / stopped / trailing columns),
  midpoint noise for the pdf these logits give at exploration ``eps`` (row 0: noise 0, nothing selected; row 2 at
  exploration 0: see below) and the incoming gradients of the backward."""
  rng = np.random.default_rng(seed)
  logits = (3.0 * rng.standard_normal((n, k))).astype(f32)
  if n > 1:
    logits[1] = f32(0.7)
  if n > 2:
    logits[2] = np.linspace(0, 120, k).astype(f32)
  if n > 3:
    logits[3] = (1e4 + 2.0 * rng.standard_normal(k)).astype(f32)
  states = rng.random((n, 3 + k + trailing)).astype(f32)
  states[:, 2] = np.arange(n) % 6
  states[:, 3:3 + k] = rng.integers(0, 2, (n, k))
  states[n // 2, 3:3 + k] = 1
  states[:, 3 + k:] = rng.standard_normal((n, trailing)).astype(f32)
  pdf64, _, _ = _pdf_ops(logits, f64(f32(eps)), f64)
  noise, target = midpoint_noise(pdf64, rng)
  noise[0], target[0] = 0.0, -1
  if n > 2 and k > 1 and eps == 0:
    # one selected probability far below 1e-10 .. 1e-4, where the surrogate's + 1e-10 decides the value: the last but one
    # entry of the linspace row, p = exp(-120 / (K - 1)).  Its interval lies next to 0, where the edges (sums of positive
    # terms) and the noise keep their RELATIVE precision, so the midpoint is as far from an edge as in a wide interval.
    pn = pdf64[2] / (pdf64[2].sum() + 1e-36)
    noise[2], target[2] = f32(pn[:k - 2].sum() + 0.5 * pn[k - 2]), k - 2
  d_surrogate = rng.standard_normal(n).astype(f32)
  d_penalty_base = (2.0 * rng.standard_normal(n)).astype(f32)
  return dict(logits=logits, states=states, noise=noise, target=target, d_surrogate=d_surrogate, d_penalty_base=d_penalty_base)


SELECT_KS = (1, 2, 3, 7, 8, 9, 16)
SELECT_NS = (1, 63, 64, 65, 130)
SELECT_EPS = (0.05, 0.0, 0.3, 1.0)


def select_cases(k):
  """Every (n, exploration, is_train) for K = ``k``; progress, the penalty constants, test_steps, the trailing state
  columns and the layout of the noise tensor go round with the case's index, so every value meets every K."""
  cases, i = [], 0
  for n in SELECT_NS:
    for eps in SELECT_EPS:
      for is_train in (1, 0):
        consts = np.array([eps, (0.05, 0.07)[i % 2], (1.0, 1.3)[(i // 2) % 2], (1.0, 0.6)[i % 2], (5, 3)[(i // 3) % 2]],
                          dtype=f32)
        cases.append(dict(k=k, n=n, eps=eps, is_train=is_train, consts=consts, progress=(0.0, 0.3, 1.0)[i % 3],
                          trailing=(0, 2)[(i // 2) % 2], noise_2d=bool(i % 2 == 0), seed=1000 * k + i))
        i += 1
  return cases


# ---- heads ------------------------------------------------------------------------------------------------------------
def _cfg_and_shift(fid, ranges):
  """The filters_np cfg that matches ``ranges`` and what has to be added to the raw features so that the regressor's own
  bias (util.py:281-294, fixed by the cfg) becomes the one ``ranges`` carries."""
  er, lg, tl, th, tb, cl, ch, cb, eb = [float(v) for v in ranges]
  cfg = dict(curve_steps=8, gamma_range=math.exp(lg), exposure_range=er, color_curve_range=(cl, ch), tone_curve_range=(tl, th))
  shift = 0.0
  if fid == 0:
    shift = eb - math.atanh(2 * (0 + er) / (2 * er) - 1)
  elif fid == 4:
    shift = tb
  elif fid == 7:
    assert cl < 1 < ch, 'the colour curve regressor starts from 1'
    shift = cb - math.atanh(2 * (1 - cl) / (ch - cl) - 1)
  return cfg, shift


def heads_fwd(raws, abi_ids, ranges, selected, dtype=f64, zero_bias=False):
  """expo_heads_regress_fwd: params (n, 24) = the regressor of head selected[n] (``filters_np.regress_packed`` with the cfg
  that ``ranges`` describes) on that head's first P features, zero behind them and in the rows that selected nothing.
  ``ranges`` = the C ABI's float[9].  ``zero_bias``: the mutant that forgets the biases."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  ranges = np.asarray(ranges, dtype=f32).astype(f64)
  if zero_bias:
    ranges = ranges.copy()
    ranges[[4, 7, 8]] = 0.0
  n = raws[0].shape[0]
  out = np.zeros((n, MAX_PARAMS), dtype=dt)
  for j, (raw, fid) in enumerate(zip(raws, abi_ids)):
    rows = np.flatnonzero(np.asarray(selected) == j)
    if len(rows) == 0:
      continue
    p = fnp.NUM_PARAMS[fid]
    cfg, shift = _cfg_and_shift(fid, ranges)
    f = np.asarray(raw)[rows, :p].astype(dt)
    if shift != 0.0:
      f = f + dt(shift)
    with np.errstate(over='ignore'):
      out[rows, :p] = fnp.regress_packed(fid, f, cfg)
  assert out.dtype == dt
  return out


def heads_bwd(raws, abi_ids, ranges, selected, dparams, wb_cross_term=True):
  """expo_heads_regress_bwd in float64, by hand: (d raw of every head, the sum of the absolute terms of every element).
  t01(x) = tanh(x) / 2 + 1 / 2, t01'(x) = (1 - tanh(x)^2) / 2 (absolute terms: (1 + tanh^2) / 2); sigmoid' = y (1 - y)
  (absolute terms y (1 + y)).
    Exposure  dp t01'(x + b) 2 r          Gamma  dp y t01'(x) 2 lg,  y = exp(t01(x) 2 lg - lg)
    Tone / Colour  dp t01'(x + b) (hi - lo)      Contrast  dp (1 - tanh(x)^2)      Saturation / BW / Level  dp y (1 - y)
    White balance: s_c = exp(t01(m_c f_c) - 1/2), m = (0, 1, 1), inv = 1 / (1e-5 + sum_c w_c s_c), out_c = s_c inv:
      d out_c / d s_k = delta_ck inv - s_c inv^2 w_k,   d s_k / d f_k = m_k s_k t01'(f_k)
      d f_k = m_k s_k t01'(f_k) (dp_k inv - (sum_c dp_c s_c) inv^2 w_k)
  Roundings of 2^-24 in the kernel's float32 evaluation of the white-balance line, relative to the absolute terms, with 2 ulp
  (4 roundings) for tanhf / expf: s_k 8 (tanh 4 halved, two adds, exp 4); inv 13 (s 8, a product, three adds, the division);
  t01' 10 (t^2: 9, the subtraction); s_k t01' 19; dp_k inv 14; the cross term 40 (dot 11, inv twice 26, three products); their
  difference 41; the final product 61.  Every other filter's line is shorter (Gamma: 27)."""
  ranges = np.asarray(ranges, dtype=f32).astype(f64)
  er, lg, tl, th, tb, cl, ch, cb, eb = ranges
  selected = np.asarray(selected)
  dparams = np.asarray(dparams, dtype=f64)
  t01 = lambda x: np.tanh(x) * 0.5 + 0.5
  dt01 = lambda x: 0.5 * (1.0 - np.tanh(x)**2)
  adt01 = lambda x: 0.5 * (1.0 + np.tanh(x)**2)
  sig = lambda x: 1.0 / (1.0 + np.exp(-x))
  draws, scales = [], []
  for j, (raw, fid) in enumerate(zip(raws, abi_ids)):
    raw = np.asarray(raw, dtype=f64)
    g, a = np.zeros_like(raw), np.zeros_like(raw)
    rows = np.flatnonzero(selected == j)
    p = fnp.NUM_PARAMS[fid]
    x, dp = raw[rows, :p], dparams[rows, :p]
    if fid == 0:
      gg, aa = dp * dt01(x + eb) * (2 * er), np.abs(dp) * adt01(x + eb) * (2 * er)
    elif fid == 1:
      y = np.exp(t01(x) * (2 * lg) - lg)
      gg, aa = dp * y * dt01(x) * (2 * lg), np.abs(dp) * y * adt01(x) * abs(2 * lg)
    elif fid == 2:
      m = np.array([0.0, 1.0, 1.0])
      w = np.array(fnp.LUM_W)
      s = np.exp(t01(x * m) - 0.5)
      inv = 1.0 / (1e-5 + (s * w).sum(axis=1, keepdims=True))
      dot = (dp * s).sum(axis=1, keepdims=True)
      cross = dot * inv**2 * w if wb_cross_term else 0.0
      gg = m * s * dt01(x) * (dp * inv - cross)
      aa = m * s * adt01(x) * (np.abs(dp) * inv + (np.abs(dp) * s).sum(axis=1, keepdims=True) * inv**2 * w)
    elif fid in (3, 6, 8):
      with np.errstate(over='ignore'):
        y = sig(x)
      gg, aa = dp * y * (1.0 - y), np.abs(dp) * y * (1.0 + y)
    elif fid == 4:
      gg, aa = dp * dt01(x + tb) * (th - tl), np.abs(dp) * adt01(x + tb) * abs(th - tl)
    elif fid == 5:
      gg, aa = dp * (1.0 - np.tanh(x)**2), np.abs(dp) * (1.0 + np.tanh(x)**2)
    else:
      gg, aa = dp * dt01(x + cb) * (ch - cl), np.abs(dp) * adt01(x + cb) * abs(ch - cl)
    g[rows, :p], a[rows, :p] = gg, aa
    draws.append(g)
    scales.append(a)
  return draws, scales


def shipped_ranges():
  cfg = fnp.DEFAULT_CFG
  (tl, th), (cl, ch) = cfg['tone_curve_range'], cfg['color_curve_range']
  return np.array([cfg['exposure_range'], math.log(cfg['gamma_range']), tl, th, 0.0, cl, ch,
                   math.atanh(2 * (1 - cl) / (ch - cl) - 1), 0.0], dtype=f32)


def biased_ranges():
  """Non-zero tone, colour and exposure biases; the colour bias by filters.heads_regress_select's atanh formula for
  color_curve_range = (0.8, 1.1), the other two (0 for every cfg) as the C ABI carries them: any value."""
  cl, ch = 0.8, 1.1
  return np.array([2.0, math.log(2.5), 0.4, 1.7, 0.3, cl, ch, math.atanh(2 * (1 - cl) / (ch - cl) - 1), -0.2], dtype=f32)


HEAD_LISTS = {
    'default8': (0, 1, 2, 3, 4, 5, 6, 7),
    'nine_with_level': (0, 1, 2, 3, 4, 5, 6, 7, 8),
    'gamma_exposure_color': (1, 0, 7),
    'tone_twice': (4, 2, 4, 6),
    'sixteen': (7, 0, 1, 2, 3, 4, 5, 6, 8, 7, 2, 4, 0, 1, 2, 5),
}
HEAD_NS = (1, 19, 257)


def heads_inputs(abi_ids, n, mask_features, seed):
  """Raw features N(0, 1.5); behind the first pass of ``selected`` over the heads, one pass each of rows of 20, -20, 100,
  -100 and exact 0 (as far as n reaches); ``selected`` cycling through -1 and every head, dparams N(0, 1) (all 24 columns: what lies behind a filter's parameters must not reach
  d raw)."""
  rng = np.random.default_rng(seed)
  raws = [(1.5 * rng.standard_normal((n, fnp.NUM_PARAMS[fid] + mask_features))).astype(f32) for fid in abi_ids]
  h = len(abi_ids)
  selected = ((np.arange(n) + (0 if n > 1 else 3)) % (h + 1) - 1).astype(np.int32)
  special = (20.0, -20.0, 100.0, -100.0, 0.0)
  for r in range(n):
    block = r // (h + 1)  # one pass of ``selected`` over the heads per block
    if 1 <= block <= len(special):
      for raw in raws:
        raw[r] = special[block - 1]
  dparams = rng.standard_normal((n, MAX_PARAMS)).astype(f32)
  return raws, selected, dparams
