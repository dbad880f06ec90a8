"""The reference of the training step's loss glue (include/exposure_hip.h): ``expo_gp_inputs / _rows``,
``expo_grad_penalty_fwd / _bwd``, ``expo_planes_concat``, ``expo_generator_losses`` (csrc/nn_ops.hip) and
``expo_critic_head_fwd / _bwd``, ``expo_critic_report``, ``expo_plane_sums``, ``expo_gp_direct`` (csrc/critic_step.hip).

Per entry point: the float64 definition (on ``oracle/nets_np.py`` where it states the formula: ``lrelu``, ``lrelu_grad``,
``enrich_image_input``; tests/test_step_glue_host.py holds the losses against ``nets_np.critic_losses`` /
``generator_losses``), the hand-derived float64 gradients (derivations in the docstrings), a float32 restatement in the
kernel's own operation order (what float32 rounding alone costs: every constant below is four times its worst error),
and the inputs both test modules run.

Error models.  A reduced quantity is judged against the sum of the ABSOLUTE values of its terms;
an element-wise one against |ref|, or, where its expression subtracts (``reward = raw - penalty``, ``g = u + ds``), against
the absolute terms of that expression, which is |ref| wherever nothing cancels.  ``term`` / ``coef`` / ``v`` of the two
penalty kernels inherit the norm's bound (``term_tol`` / ``coef_tol``): continuous across the kink at norm = 1.
Every tolerance carries 2^-126.  Scalars a kernel is handed as float (leak, 1 / N, lambda, ...) are taken at their float32
values.

TEST INFRASTRUCTURE ONLY, NumPy only."""
import numpy as np

from oracle import nets_np
from tests._agent_glue_ref import worst_ratio

f32, f64 = np.float32, np.float64
GUARD = 64  # elements behind every output buffer of the GPU tests

# ---- the constants: 4 x the float32 restatement's worst error on the inputs below, rounded up --------------------------
# (tests/test_step_glue_host.py::test_*_constant_is_four_times_the_restatement_error recomputes every one)
#                       restatement's worst    model
C_INTERP = 4.7e-7     # 1.17e-7   C (|r| + |a| (|f| + |r|))
C_NORM = 3.7e-7       # 9.25e-8   C |norm|            (grad_penalty_fwd: the squared norm is a sum of squares)
C_DG = 4.4e-7         # 1.08e-7   C |ref|             (grad_penalty_bwd: the norm is an input)
C_GEN_ROWS = 7.6e-7   # 1.88e-7   C (absolute terms of reward, q, each coef row)
C_GEN_LOSS = 3.5e-7   # 8.63e-8   C (mean of the absolute terms of the g / v terms)
C_LOGIT = 4.9e-7      # 1.22e-7   C (sum |h w2| + |b2|)
C_DH = 5.4e-7         # 1.33e-7   C |ref|
C_GB1 = 4.6e-7        # 1.13e-7   C sum |dh|          (and bit-equal to the ordered restatement)
C_GW2 = 4.5e-7        # 1.12e-7   C (sum |dl h| + sum_s |thpre_s| slope)
C_GB2 = 9e-8          # 2.24e-8   C (n_real + n_fake) / N
C_REPORT = 4.2e-7     # 1.04e-7   C (absolute terms of each reported scalar)
C_PLANE = 1.6e-7      # 3.97e-8   C sum |x|
C_GPNORM = 3.6e-7     # 8.94e-8   C sqrt(1e-6 + sum (|u| + |ds|)^2)   (gp_direct: g = u + ds may cancel)
C_V = 6.9e-7          # 1.71e-7   (|u| + |ds|) (coef_tol + C |coef|), the restatement measured at its own norm


def within(got, ref, tol):
  """worst |got - ref| / (tol + 2^-126) over the elements; anything non-finite: infinity."""
  return worst_ratio(got, ref, 0.0, 1.0, tol)


def assert_within(got, ref, tol, what):
  r = within(got, ref, tol)
  assert r <= 1.0, '%s: worst err / tol = %.3g' % (what, r)
  return r


def needed(got, ref, scale, slack=0.0):
  """The smallest C with |got - ref| <= slack + C scale + 2^-126 everywhere (how a restatement is measured)."""
  got, ref = np.asarray(got, dtype=f64), np.asarray(ref, dtype=f64)
  assert np.isfinite(got).all() and got.shape == ref.shape
  excess = np.maximum(np.abs(got - ref) - slack - 2.0**-126, 0.0)
  scale = np.broadcast_to(np.asarray(scale, dtype=f64), ref.shape)
  with np.errstate(divide='ignore', invalid='ignore'):
    c = np.where(excess == 0, 0.0, excess / scale)
  return float(c.max()) if c.size else 0.0


def _in(x, dt):
  """An input as the kernel sees it: float32 values (float64 inputs stay as they are when the float64 definition is asked)."""
  return np.asarray(x, dtype=f32) if dt is f32 else np.asarray(x).astype(f64)


def fma(a, b, c, dt):
  """fmaf in float32 (the product of two float32 is exact in float64; the double rounding of the sum is far below what the
  constants resolve); plain a b + c in float64."""
  if dt is f64:
    return a * b + c
  return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def tree(part):
  """part[k] += part[k + w] for w = len / 2, len / 4 ... 1 along axis 0: the LDS trees and the lane-0 view of wave_sum's
  xor butterfly (lane i adds lane i ^ w: float addition commutes)."""
  part = np.array(part)
  w = part.shape[0] // 2
  while w > 0:
    part = part[:w] + part[w:2 * w]
    w //= 2
  return part[0]


def strided(values, width, dt, op=None):
  """acc[t] = op(acc[t], values[t + k width]) for k = 0, 1, ...: ``width`` threads' loops over the elements along axis 0 (plain
  addition without ``op``; a thread past the end adds nothing)."""
  values = np.asarray(values)
  acc = np.zeros((width,) + values.shape[1:], dtype=dt)
  for start in range(0, values.shape[0], width):
    chunk = values[start:start + width]
    k = chunk.shape[0]
    acc[:k] = (acc[:k] + chunk) if op is None else op(acc[:k], chunk)
  return acc


# ---- expo_gp_inputs / expo_gp_inputs_rows -----------------------------------------------------------------------------
GP_SHAPES = ((1, 1, 1, 3), (3, 7, 5, 3), (2, 9, 9, 3), (1, 75, 73, 3), (2, 80, 72, 3))  # 16425: one element past 64 x 256


def gp_inputs(real, fake, alpha, real_rows=None, fake_rows=None, dtype=f64, one_trip=False):
  """(cat, interp, scale): cat = [real rows | fake rows] as float32 (exact: no arithmetic), interp = r + alpha (f - r)
  (net.py:170-172), scale = |r| + |alpha| (|f| + |r|): the absolute terms of interp.  ``alpha`` None: no interp.
  ``one_trip``: the mutant whose threads leave after 64 blocks x 256 elements (interp and cat stay NaN behind them)."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  r = np.asarray(real)[np.arange(len(real)) if real_rows is None else np.asarray(real_rows)]
  f = np.asarray(fake)[np.arange(len(fake)) if fake_rows is None else np.asarray(fake_rows)]
  cat = np.concatenate([r, f]).astype(f32)
  interp = scale = None
  if alpha is not None:
    a = np.asarray(alpha, dtype=f32).astype(dt).reshape((-1,) + (1,) * (r.ndim - 1))
    rr, ff = r.astype(dt), f.astype(dt)
    interp = rr + a * (ff - rr)
    scale = (np.abs(rr) + np.abs(a) * (np.abs(ff) + np.abs(rr))).astype(f64)
    assert interp.dtype == dt
  if one_trip:
    n = len(r)
    cat.reshape(2 * n, -1)[:, 64 * 256:] = np.nan
    if interp is not None:
      interp.reshape(n, -1)[:, 64 * 256:] = np.nan
  return cat, interp, scale


def gp_case(shape, np_dtype, seed):
  rng = np.random.default_rng(seed)
  real = rng.random(shape).astype(np_dtype)
  fake = (1.5 * rng.random(shape)).astype(np_dtype)
  alpha = rng.random(shape[0]).astype(f32)
  alpha[0] = (0.0, 1.0)[seed % 2]
  return real, fake, alpha


def gp_row_cases(np_dtype, seed):
  """(name, real, real_rows, fake, fake_rows, alpha): a permutation, a repeated row, rows into a pool of 9 images with
  n = 4, and rows on one side only (each side once)."""
  rng = np.random.default_rng(seed)
  img = lambda k: rng.random((k, 7, 5, 3)).astype(np_dtype)
  alpha = lambda k: rng.random(k).astype(f32)
  i64 = lambda v: np.asarray(v, dtype=np.int64)
  return [('permutation', img(5), i64([3, 0, 4, 1, 2]), img(5), i64([1, 4, 0, 2, 3]), alpha(5)),
          ('repeated row', img(4), i64([2, 2, 0, 2]), img(4), i64([0, 1, 1, 3]), alpha(4)),
          ('pool of 9', img(6), i64([5, 0, 3, 1]), img(9), i64([8, 2, 8, 6]), alpha(4)),
          ('real rows only', img(9), i64([7, 1, 8]), img(3), None, alpha(3)),
          ('fake rows only', img(3), None, img(9), i64([0, 8, 4]), alpha(3))]


# ---- expo_grad_penalty_fwd / _bwd -------------------------------------------------------------------------------------
PEN_ELEMS = (1, 3, 255, 256, 257, 12288, 17280)
PEN_NORMS = (0.0, 1 - 1e-3, 1 + 1e-3, 0.5, 3.0, 3.0, 1.7)  # row 0: the all-zero image
PEN_DTERM = (0.8, -1.3, 0.9, 0.4, -0.6, 0.0, 1.1)  # both signs and 0, on images of either side of the kink


def penalty_images(m, seed):
  """(g (7, m) float32, dterm): image k scaled so that sqrt(1e-6 + sum g^2) = PEN_NORMS[k] (row 0 all zero)."""
  rng = np.random.default_rng(seed)
  g = rng.standard_normal((len(PEN_NORMS), m))
  for k, target in enumerate(PEN_NORMS):
    g[k] *= np.sqrt(max(target**2 - 1e-6, 0.0) / (g[k]**2).sum())
  return g.astype(f32), np.array(PEN_DTERM, dtype=f32)


def penalty_fwd(g, dtype=f64, one_trip=False):
  """(norm, term) per image: norm = sqrt(1e-6 + sum g^2), term = max(norm - 1, 0)^2 (net.py:185-187;
  ``nets_np.critic_losses``).  float32: a thread's fmaf over elements t, t + 256, ..., the 256-wide LDS tree, sqrtf."""
  g = _in(g, f32 if np.dtype(dtype) == np.float32 else f64).reshape(len(g), -1)
  if np.dtype(dtype) == np.float32:
    cols = g.T[:256] if one_trip else g.T
    part = strided(cols, 256, f32, lambda s, v: fma(v, v, s, f32))
    norm = np.sqrt(f32(1e-6) + tree(part))
    over = np.maximum(norm - f32(1), f32(0))
    assert norm.dtype == f32
    return norm, over * over
  norm = np.sqrt(1e-6 + np.sum(g.astype(f64)**2, axis=1))
  return norm, np.maximum(norm - 1.0, 0.0)**2


def term_tol(norm, delta):
  """|d term| <= 2 max(norm - 1, 0) d + d^2 for |d norm| <= d."""
  return 2.0 * np.maximum(np.asarray(norm, f64) - 1.0, 0.0) * delta + np.asarray(delta, f64)**2


def penalty_coef(norm, factor=2.0):
  """d term / d g = coef g with coef = 2 max(norm - 1, 0) / norm:  term = o^2, o = max(nm - 1, 0), nm = sqrt(1e-6 + sum g^2);
  d nm / d g = g / nm, d o / d nm = [nm > 1]  ->  d term / d g = 2 o g / nm (0 below the kink, continuous across it)."""
  norm = np.asarray(norm, f64)
  return factor * np.maximum(norm - 1.0, 0.0) / norm


def coef_tol(norm, delta):
  """The largest |coef(norm') - coef(norm)| over |norm' - norm| <= delta (coef is monotone)."""
  norm = np.asarray(norm, f64)
  c = penalty_coef(norm)
  return np.maximum(penalty_coef(norm + delta) - c, c - penalty_coef(np.maximum(norm - delta, 1e-3)))


def penalty_bwd(g, norm, dterm, dtype=f64, with_norm=True, one_trip=False):
  """dg = dterm 2 max(norm - 1, 0) / norm g with ``norm`` the float32 the kernel is handed.  ``with_norm=False``: the mutant
  without the 1 / norm."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  g2 = np.asarray(g, dtype=f32).reshape(len(g), -1).astype(dt)
  nm, dterm = np.asarray(norm, dtype=f32).astype(dt), np.asarray(dterm, dtype=f32).astype(dt)
  c = dterm * dt(2) * np.maximum(nm - dt(1), dt(0))
  if with_norm:
    c = c / nm
  dg = g2 * c[:, None]
  if one_trip:
    dg[:, 64 * 256:] = np.nan
  assert dg.dtype == dt
  return dg.reshape(np.shape(g))


# ---- expo_planes_concat -----------------------------------------------------------------------------------------------
CONCAT_SHAPES = ((2, 1, 1), (2, 16, 12), (1, 15, 17), (2, 16, 16), (1, 257, 1), (1, 64, 64))  # pixels 1 .. 4096
CONCAT_VS = (0, 1, 3, 14, 29, 61)
CONCAT_BIG = (1, 513, 512)  # 262656 pixels: 1027 blocks capped to 1024, blocks 0 and 1 take a second trip (v = 1)


def planes_concat(images, vec, offset, one_trip=False):
  """out[n, p, c] = (c < 3 ? images[n, p, c] : vec[n, c - 3]) - offset rounded ONCE to float32 (the float64 difference of a
  float32 / float16 and 0.5 is exact): ``nets_np.enrich_image_input`` and the ``- 0.5`` of critics.py:64-76."""
  x = np.asarray(images).astype(f64)
  if vec is not None and np.shape(vec)[1] > 0:
    x = nets_np.enrich_image_input(dict(img_include_states=True), x, np.asarray(vec, dtype=f32).astype(f64))
  out = (x - float(f32(offset))).astype(f32)
  if one_trip:
    out.reshape(out.shape[0], -1, out.shape[-1])[:, 1024 * 256:] = np.nan
  return out


def concat_case(shape, v, np_dtype, seed):
  rng = np.random.default_rng(seed)
  img = rng.random(shape + (3,)).astype(np_dtype)
  return img, (rng.standard_normal((shape[0], v)).astype(f32) if v else None)


# ---- expo_generator_losses --------------------------------------------------------------------------------------------
GEN_NS = (1, 37, 255, 256, 257, 700)
GEN_CONSTS = np.array([0.3, 0.05, 0.98, 1.7, 7.0], dtype=f32)  # all_reward, mult, discount, plm, max_len


def gen_inputs(n, state_dim, seed, max_len=7):
  """Per-image scalars N(0, 1) (penalty |N|); new_states with stopped in {0, 1} and steps max_len - 1, max_len,
  max_len + 1 in turn (every combination with stopped from n = 6 on), random everywhere else."""
  rng = np.random.default_rng(seed)
  x = {k: rng.standard_normal(n).astype(f32) for k in ('fake_logit', 'fake_input_logit', 'new_value', 'old_value', 'surrogate')}
  x['penalty'] = np.abs(rng.standard_normal(n)).astype(f32)
  states = rng.standard_normal((n, state_dim)).astype(f32)
  states[:, 1] = (np.arange(n) // 3) % 2
  states[:, 2] = max_len - 1 + np.arange(n) % 3
  x['new_states'] = states
  return x


def generator_losses(x, consts, use_td, use_penalty, dtype=f64, keep_ge=False, gated=True, one_trip=False):
  """expo_generator_losses (net.py:92-160; ``nets_np.generator_losses`` from ``stopped`` on), per image i:
    nv = new_value [step <= max_len];  gate = a + (1 - a) stopped;  raw = gate (fake_logit - fake_input_logit) mult
    reward = raw - penalty;  cont = (1 - stopped) discount;  q = reward + cont nv;  adv = q - old_value
    TD: g_i = -q plm + surrogate w, w = stop_gradient(-adv);  otherwise g_i = -reward + surrogate w, w = stop_gradient(-reward)
    v_i = (stop_gradient(q) - old_value)^2;   g_loss = mean g_i, v_loss = mean v_i
  Hand gradients (coef rows, N = the batch), dq = d g_i / d q = -plm (TD) or d g_i / d reward = -1:
    0  d g_loss / d fake_logit = dq gate mult / N        (reward and q move one for one with raw)
    1  d g_loss / d new_value  = dq cont [step <= max_len] / N  (TD; without TD the loss does not see new_value: 0)
    2  d g_loss / d surrogate  = w / N
    3  d g_loss / d penalty    = -dq / N                 (reward = raw - penalty; 0 without the penalty)
    4  d v_loss / d old_value  = -2 adv / N
  Returns a dict; float64 adds ``scale`` (same keys): the absolute terms.  ``keep_ge`` (step >= max_len clears), ``gated``
  = False (reward without the gate) and ``one_trip`` (a thread's loop stops after its first image) are the mutants."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  a, mult, disc, plm, max_len = [dt(v) for v in np.asarray(consts, dtype=f32)]
  v = {k: _in(x[k], dt) for k in x}
  n = len(v['fake_logit'])
  one, inv_n = dt(1), dt(1) / dt(n)
  stopped, step = v['new_states'][:, 1], v['new_states'][:, 2]
  keep = np.where((step >= max_len) if keep_ge else (step > max_len), dt(0), one)
  nv = v['new_value'] * keep
  gate = a + (one - a) * stopped if gated else np.ones_like(stopped)
  raw = gate * (v['fake_logit'] - v['fake_input_logit']) * mult
  reward = raw - v['penalty'] if use_penalty else raw
  cont = (one - stopped) * disc
  q = reward + cont * nv
  adv = q - v['old_value']
  sur = v['surrogate']
  if use_td:
    routine, weight, dq = -q * plm, -adv, -plm
  else:
    routine, weight, dq = -reward, -reward, dt(-1)
  g_terms, v_terms = routine + sur * weight, adv * adv
  zero = np.zeros(n, dtype=dt)
  coef = np.stack([dq * gate * mult * inv_n, dq * cont * keep * inv_n if use_td else zero, weight * inv_n,
                   -dq * inv_n + zero if use_penalty else zero, dt(-2) * adv * inv_n])
  if dt is f32:
    if one_trip:
      g_terms, v_terms = g_terms[:256], v_terms[:256]
    losses = np.array([tree(strided(g_terms, 256, f32)) * inv_n, tree(strided(v_terms, 256, f32)) * inv_n])
  else:
    losses = np.array([g_terms.mean(), v_terms.mean()])
  out = dict(losses=losses, reward=reward, q=q, coef=coef)
  assert all(t.dtype == dt for t in out.values())
  if one_trip:
    for t in (reward, q, coef):
      t[..., 256:] = np.nan
  if dt is f64:
    a_r = np.abs(raw) + (np.abs(v['penalty']) if use_penalty else 0.0)
    a_q = a_r + np.abs(cont * nv)
    a_adv = a_q + np.abs(v['old_value'])
    a_w = a_adv if use_td else a_r
    a_routine = a_q * plm if use_td else a_r
    out['scale'] = dict(losses=np.array([(a_routine + np.abs(sur) * a_w).mean(), (a_adv**2).mean()]), reward=a_r, q=a_q,
                        coef=np.stack([np.abs(coef[0]), np.abs(coef[1]), a_w * inv_n, np.abs(coef[3]), 2 * a_adv * inv_n]))
    out['frozen'] = dict(q=q, weight=weight)
  return out


# ---- expo_critic_head_fwd / _bwd --------------------------------------------------------------------------------------
HEAD_HIDDEN = (1, 16, 63, 64, 65, 128, 200)
HEAD_ROWS = ((1, 1, 1), (3, 5, 0), (0, 0, 7), (5, 5, 5), (64, 64, 64), (96, 96, 96), (130, 130, 3))
HEAD_SLABS = (1, 2, 9, 17, 64)
TH_SLABS = (1, 9, 64)
PAIRED_NS = (1, 2, 3, 4, 5, 6, 8, 12, 64, 96, 128, 192)
MAX_FLOATS = 1 << 20  # no tensor of the GPU tests is larger than 4 MB
LEAK = f32(0.2)


def _fit(slabs, choices, per_slab):
  while slabs * per_slab > MAX_FLOATS:
    slabs = max(s for s in choices if s < slabs)
  return slabs


def head_cases(hidden):
  """(rows, slabs, th_slabs) for one width: every row case with one slab and no b1, and with a slab count > 1 that goes
  round (the largest that keeps the tensor under 4 MB); (5, 5, 5) with every slab count."""
  cases = []
  hi = HEAD_HIDDEN.index(hidden)
  for i, rows in enumerate(HEAD_ROWS):
    m = sum(rows)
    th = _fit(TH_SLABS[(i + hi) % 3], TH_SLABS, max(rows[2], 1) * hidden)
    cases.append((rows, 1, th))
    cases.append((rows, _fit(HEAD_SLABS[1 + (i + hi) % 4], HEAD_SLABS, m * hidden),
                  _fit(TH_SLABS[(i + hi + 1) % 3], TH_SLABS, max(rows[2], 1) * hidden)))
  for s in HEAD_SLABS[1:]:
    cases.append(((5, 5, 5), s, TH_SLABS[s % 3]))
  return cases


def head_inputs(rows, hidden, slabs, seed):
  """hpre (slabs, m, hidden) in multiples of 1 / 256 (every partial sum, b1 included, stays below 2^9 and is exact in float32
  and in float64: both see the same pre-activation and the same side of the kink); about one pre-activation in nine is
  exactly 0 -- slab 0 cancels the rest -- and 0.0 or -0.0 where there is one slab.  w2, b2 N(0, 1); b1 None for one slab."""
  rng = np.random.default_rng(seed)
  m = sum(rows)
  grid = lambda shape: (rng.integers(-1024, 1025, shape) / 256.0).astype(f32)
  hpre = grid((slabs, m, hidden))
  b1 = grid((hidden,)) if slabs > 1 else None
  zero = rng.random((m, hidden)) < 1.0 / 9
  if slabs == 1:
    hpre[0][zero] = np.where(rng.random((m, hidden)) < 0.5, f32(0.0), f32(-0.0))[zero]
  else:
    hpre[0][zero] = -(hpre[1:].astype(f64).sum(axis=0) + b1.astype(f64))[zero]
  return hpre, b1, rng.standard_normal(hidden).astype(f32), rng.standard_normal(1).astype(f32)


def slope(z, leak, dt):
  """The kernels' cs_slope: 1, leak, (1 + leak) / 2 at exactly 0 (TF's abs'(0) = 0) -- ``nets_np.lrelu_grad`` in float64."""
  if dt is f64:
    return nets_np.lrelu_grad(np.asarray(z, f64), float(leak))
  z = np.asarray(z, f32)
  return np.where(z > 0, f32(1), np.where(z < 0, f32(leak), f32(0.5) * (f32(1) + f32(leak)))).astype(f32)


def row_signs(rows, inv_n, dt):
  nr, nf, ni = rows
  inv = dt(f32(inv_n))
  return np.concatenate([np.full(nr, -inv, dt), np.full(nf, inv, dt), np.ones(ni, dt)]).astype(dt)


def head_fwd(hpre, b1, w2, b2, rows, inv_n, leak=LEAK, dtype=f64, slabs_read=None):
  """expo_critic_head_fwd: pre = sum_s hpre[s] + b1, h = lrelu(pre), logit_m = h_m . w2 + b2, and the gradient of
  L = sum_m dl_m logit_m (dl = -1/N real, +1/N fake, 1 interpolated) at the pre-activation:
    dh[m, j] = dL / d pre[m, j] = dl_m w2_j lrelu'(pre[m, j])       (lrelu'(0) = (1 + leak) / 2)
  float32: slabs in order, then b1; the dot by fmaf per lane over j = lane, lane + 64, ..., lanes by the xor tree.
  Returns dict(h, logits, dh) and, float64, ``logit_scale`` = sum |h w2| + |b2|.  ``slabs_read``: the mutant that adds only
  that many slabs."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  hp = np.asarray(hpre, dtype=f32).astype(dt)
  hp = hp[None] if hp.ndim == 2 else hp
  w, b, lk = np.asarray(w2, f32).astype(dt), dt(np.asarray(b2, f32).reshape(-1)[0]), dt(f32(leak))
  pre = hp[0].copy()
  for s in range(1, len(hp) if slabs_read is None else slabs_read):
    pre = pre + hp[s]
  if b1 is not None:
    pre = pre + np.asarray(b1, f32).astype(dt)
  dl = row_signs(rows, inv_n, dt)
  if dt is f64:
    h = np.where(pre > 0, pre, pre * lk)  # (``nets_np.lrelu``'s f1 x + f2 |x| up to rounding: held to it on the CPU)
    sl = nets_np.lrelu_grad(pre, float(lk))
    return dict(h=h, logits=h @ w + b, dh=dl[:, None] * w[None, :] * sl, logit_scale=np.abs(h) @ np.abs(w) + abs(b))
  h = np.where(pre > 0, pre, pre * lk).astype(f32)
  dh = (dl[:, None] * w[None, :]) * slope(h, lk, f32)
  lanes = np.zeros((64, h.shape[0]), f32)
  for start in range(0, h.shape[1], 64):
    k = min(64, h.shape[1] - start)
    lanes[:k] = fma(h.T[start:start + k], w[start:start + k, None], lanes[:k], f32)
  logits = tree(lanes) + b
  assert h.dtype == f32 and dh.dtype == f32 and logits.dtype == f32
  return dict(h=h, logits=logits, dh=dh)


def bwd_groups(n_real, n_fake):
  """The host's choice of row groups: 64, or the largest power of two <= 64 that divides equally long blocks."""
  groups = 64
  if n_real > 0 and n_real == n_fake:
    while groups > 1 and n_real % groups:
      groups >>= 1
  return groups


def head_bwd(dh, h, thpre, rows, inv_n, leak=LEAK, dtype=f64, order='kernel', th_read=None):
  """expo_critic_head_bwd, the gradients of L (``head_fwd``) plus the tangent's logit T = sum_m (t_m * lrelu'(h_m)) . w2 over
  the interpolated rows (t = sum_s thpre[s]) at fc1's bias, fc2's weight and fc2's bias:
    gb1[j] = sum_{loss rows} dh[m, j]                     (pre = x W1 + b1: d pre / d b1 = 1; the tangent has no bias)
    gw2[j] = sum_{loss rows} dl_m h[m, j] + sum_{interp} t[m, j] lrelu'(h[m, j])
    gb2    = sum_{loss rows} dl_m = (n_fake - n_real) / N
  Returns dict(gb1, gw2, gb2) and, float64, ``scale`` (the sums of the absolute terms).
  float32: a block's G row groups (``bwd_groups``), group g walking rows g, g + G, ... of the loss block and then of the
  interpolated block, the 64 group sums by the stride-32 tree.  ``order``: 'kernel' = what the kernel does now (equally
  long blocks: real row m and its fake partner are added to each other first, so a pair with equal slopes cancels before
  it meets anything else), 'parent' = a group's real rows first and its fake rows after, for every row count (the kernel
  before the pairing; the same additions in the same order when each group holds one row per side)."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  nr, nf, ni = rows
  nl = nr + nf
  dh, h = _in(dh, dt), _in(h, dt)
  hidden = h.shape[1]
  lk = dt(f32(leak))
  dl = row_signs(rows, inv_n, dt)
  t = None
  if ni:
    th = _in(thpre, dt)
    th = th[None] if th.ndim == 2 else th
    t = th[0].copy()
    for s in range(1, len(th) if th_read is None else th_read):
      t = t + th[s]
  if dt is f64:
    sl = nets_np.lrelu_grad(h[nl:], float(lk))
    gw2 = (dl[:nl, None] * h[:nl]).sum(axis=0) + ((t * sl).sum(axis=0) if ni else 0.0)
    a_t = (np.abs(np.asarray(thpre, f64).reshape(-1, ni, hidden)).sum(axis=0) * sl).sum(axis=0) if ni else 0.0
    inv = float(f32(inv_n))
    return dict(gb1=dh[:nl].sum(axis=0), gw2=gw2, gb2=np.array([dl[:nl].sum()]),
                scale=dict(gb1=np.abs(dh[:nl]).sum(axis=0), gw2=(np.abs(dl[:nl, None] * h[:nl])).sum(axis=0) + a_t,
                           gb2=np.array([(nr + nf) * inv])))
  groups = bwd_groups(nr, nf)
  paired = order == 'kernel' and nr > 0 and nr == nf
  p1, p2 = np.zeros((64, hidden), f32), np.zeros((64, hidden), f32)
  for g in range(groups):
    s1, s2 = np.zeros(hidden, f32), np.zeros(hidden, f32)
    for m in range(g, nl, groups):
      if not paired:
        s1 = s1 + dh[m]
      elif m < nr:
        s1 = s1 + (dh[m] + dh[nr + m])
      s2 = fma(dl[m], h[m], s2, f32)
    for m in range(g, ni, groups):
      s2 = fma(t[m], slope(h[nl + m], lk, f32), s2, f32)
    p1[g], p2[g] = s1, s2
  inv = f32(inv_n)
  return dict(gb1=tree(p1), gw2=tree(p2), gb2=np.array([f32(nf) * inv - f32(nr) * inv], dtype=f32))


def bwd_inputs(rows, hidden, th_slabs, seed):
  """dh, thpre N(0, 1), h N(0, 1) with one element in seven exactly 0."""
  rng = np.random.default_rng(seed)
  m = sum(rows)
  dh = rng.standard_normal((m, hidden)).astype(f32)
  h = rng.standard_normal((m, hidden)).astype(f32)
  h[rng.random((m, hidden)) < 1.0 / 7] = 0.0
  thpre = rng.standard_normal((th_slabs, rows[2], hidden)).astype(f32)
  return dh, h, (thpre[0] if th_slabs == 1 else thpre)


def paired_inputs(n, hidden, seed, odd_unit=None):
  """n real rows and n fake rows whose slopes (1, leak and the 0.6 of an exact zero, a third each) agree pair by pair:
  (dh, h) as ``head_fwd`` in float32 makes them, dh = (dl w2) slope -- a unit's real and fake entries are exact negatives of
  each other.  ``odd_unit``: in that column the first fake row takes the next slope round."""
  rng = np.random.default_rng(seed)
  kind = rng.integers(0, 3, (n, hidden))
  kinds = np.concatenate([kind, kind])
  if odd_unit is not None:
    kinds[n, odd_unit] = (kinds[n, odd_unit] + 1) % 3
  mag = (0.25 + rng.random((2 * n, hidden))).astype(f32)
  h = np.where(kinds == 0, mag, np.where(kinds == 1, -mag * LEAK, f32(0))).astype(f32)
  w2 = rng.standard_normal(hidden).astype(f32)
  w2[w2 == 0] = 1
  inv_n = 1.0 / n
  dh = (row_signs((n, n, 0), inv_n, f32)[:, None] * w2[None, :]) * slope(h, LEAK, f32)
  return dh.astype(f32), h, inv_n


# ---- expo_critic_report -----------------------------------------------------------------------------------------------
REPORT_ROWS = ((1, 1, 1), (3, 5, 0), (0, 0, 7), (5, 5, 5), (64, 64, 64), (65, 63, 64), (130, 130, 70))


def report_inputs(rows, seed):
  rng = np.random.default_rng(seed)
  return ((2.0 * rng.standard_normal(sum(rows))).astype(f32), (0.5 + rng.random(rows[2])).astype(f32),
          rng.random(rows[2]).astype(f32))


def critic_report(logits, norm, term, rows, lam, decay, ema, dtype=f64, one_trip=False):
  """expo_critic_report (net.py:165-168, 188-199; ``nets_np.critic_losses``): out = (c_loss, emd, mean gradient norm,
  gradient penalty, c_average) with mr / mf the mean real / fake logit, gp = lambda mean(term), c_loss = (mf - mr) + gp,
  emd = mr - mf, c_average = (mf + mr) / 2; the moving average ema + (1 - decay) (c_average - ema).  An empty block's mean
  is 0.  float32: lane sums over rows lane, lane + 64, ..., the xor tree.  Returns (out, new ema) and, float64, their
  absolute terms."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  nr, nf, ni = rows
  lg = _in(logits, dt)
  lam, decay, ema = dt(f32(lam)), dt(f32(decay)), dt(f32(ema))
  parts = [lg[:nr], lg[nr:nr + nf], _in(norm, dt), _in(term, dt)]
  if dt is f32:
    sums = [tree(strided(p[:64] if one_trip else p, 64, f32)) for p in parts]
  else:
    sums = [p.sum() for p in parts]
    asums = [np.abs(p).sum() for p in parts]
  mean = lambda s, k: s / dt(k) if k > 0 else dt(0)
  mr, mf = mean(sums[0], nr), mean(sums[1], nf)
  gp = lam * sums[3] / dt(ni) if ni > 0 else dt(0)
  ca = dt(0.5) * (mf + mr)
  out = np.array([(mf - mr) + gp, mr - mf, mean(sums[2], ni), gp, ca], dtype=dt)
  new_ema = ema + (dt(1) - decay) * (ca - ema)
  if dt is f32:
    return out, f32(new_ema)
  ar, af = mean(asums[0], nr), mean(asums[1], nf)
  agp = abs(lam) * asums[3] / ni if ni > 0 else 0.0
  scale = np.array([ar + af + agp, ar + af, mean(asums[2], ni), agp, 0.5 * (ar + af)])
  return out, new_ema, scale, abs(ema) + abs(1 - decay) * (scale[4] + abs(ema))


# ---- expo_plane_sums / expo_gp_direct ---------------------------------------------------------------------------------
SUM_PIXELS = ((1, 1), (7, 5), (33, 31), (32, 32), (41, 25), (80, 72))  # 1, 35, 1023, 1024, 1025, 5760
SUM_PLANES = (1, 3, 14, 16)


def block_reduce(acc):
  """The 1024 thread sums of a block: each of the 16 waves by the xor tree, the waves in index order."""
  total = tree(acc[:64])
  for w in range(1, 16):
    total = total + tree(acc[64 * w:64 * (w + 1)])
  return total


def block_sum(values, dt):
  """values (pixels, ...) summed as a 1024-thread block does: a thread over pixels t, t + 1024, ..., then ``block_reduce``."""
  if dt is f64:
    return np.asarray(values, f64).sum(axis=0)
  return block_reduce(strided(np.asarray(values, f32), 1024, f32))


def plane_sums(x, first, dtype=f64, one_trip=False):
  """sums[n, c - first] = sum over the pixels of x[n, ..., c]; float64 also the sums of |x|."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  x = np.asarray(x, f32)
  planes = x.reshape(x.shape[0], -1, x.shape[-1])[:, :, first:]
  if one_trip:
    planes = planes[:, :1024]
  if dt is f32:
    return np.stack([block_sum(p, f32) for p in planes])
  return planes.astype(f64).sum(axis=1), np.abs(planes.astype(f64)).sum(axis=1)


def gp_direct_inputs(shape, u_channels, seed):
  """u (n, h, w, u_channels), ds (n, h, w, 3) with g = u[..., :3] + ds scaled per image to PEN_NORMS (the all-zero image
  has u = -ds, not zeros: the sum cancels exactly)."""
  rng = np.random.default_rng(seed)
  n = len(PEN_NORMS)
  u = rng.standard_normal((n,) + shape + (u_channels,))
  ds = rng.standard_normal((n,) + shape + (3,))
  for k, target in enumerate(PEN_NORMS):
    g = u[k, ..., :3] + ds[k]
    s = np.sqrt(max(target**2 - 1e-6, 0.0) / (g**2).sum())
    u[k, ..., :3] *= s
    ds[k] *= s
  u, ds = u.astype(f32), ds.astype(f32)
  ds[0] = -u[0, ..., :3]
  return u, ds


def gp_direct(u, ds, scale, dtype=f64, at_norm=None, with_norm=True, one_trip=False):
  """expo_gp_direct: g = u[..., :3] + ds, (norm, term) as ``penalty_fwd``, v = scale d term / d g = scale coef g
  (``penalty_coef``).  float32: a thread's fmaf over its pixels' three channels, ``block_sum``'s order, then
  coef = scale 2 max(nm - 1, 0) / nm.  ``at_norm``: float64 only, v with coef taken at that norm (a restatement's own:
  what is left is v's element-wise rounding).  Returns dict(norm, term, v) and, float64, g_abs = |u| + |ds| and coef."""
  dt = f32 if np.dtype(dtype) == np.float32 else f64
  u3, d = np.asarray(u, f32)[..., :3].astype(dt), np.asarray(ds, f32).astype(dt)
  n = len(u3)
  g = (u3 + d).reshape(n, -1, 3)
  sc = dt(f32(scale))
  if dt is f32:
    sq = np.zeros(n, f32)
    for i in range(n):
      acc = np.zeros(1024, f32)
      pixels = g[i][:1024] if one_trip else g[i]
      for start in range(0, len(pixels), 1024):
        chunk = pixels[start:start + 1024]
        for c in range(3):
          acc[:len(chunk)] = fma(chunk[:, c], chunk[:, c], acc[:len(chunk)], f32)
      sq[i] = block_reduce(acc)
    norm = np.sqrt(f32(1e-6) + sq)
    over = np.maximum(norm - f32(1), f32(0))
    coef = sc * f32(2) * over
    coef = coef / norm if with_norm else coef
    v = g * coef[:, None, None]
    if one_trip:
      v[:, 1024:] = np.nan
    assert v.dtype == f32 and norm.dtype == f32
    return dict(norm=norm, term=over * over, v=v.reshape(d.shape))
  norm = np.sqrt(1e-6 + (g**2).sum(axis=(1, 2)))
  coef = sc * penalty_coef(norm if at_norm is None else np.asarray(at_norm, f64))
  g_abs = (np.abs(u3) + np.abs(d)).reshape(n, -1, 3)
  return dict(norm=norm, term=np.maximum(norm - 1.0, 0.0)**2, v=(g * coef[:, None, None]).reshape(d.shape), coef=coef,
              g_abs=g_abs.reshape(d.shape), norm_scale=np.sqrt(1e-6 + (g_abs**2).sum(axis=(1, 2))))


# ---- the comparisons of the GPU tests (tests/test_step_glue_host.py feeds them mutants) ------------------------------
def check_bit_equal(got, want, what):
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, what
  bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
  assert bad.size == 0, '%s: %d elements differ, the first at %d' % (what, bad.size, bad[0])


def check_interp(got, ref, scale, what):
  return assert_within(got, ref, C_INTERP * scale, what + ' interp')


def check_penalty_fwd(norm, term, ref_norm, ref_term, what):
  delta = C_NORM * np.abs(ref_norm)
  return dict(norm=assert_within(norm, ref_norm, delta, what + ' norm'),
              term=assert_within(term, ref_term, term_tol(ref_norm, delta), what + ' term'))


def check_dg(got, ref, what):
  return assert_within(got, ref, C_DG * np.abs(ref), what + ' dg')


def check_generator(got, ref, what):
  """reward, q, the five coef rows (a row whose reference is 0 has scale 0: it must be 0) and the two losses."""
  worst = {k: assert_within(got[k], ref[k], C_GEN_ROWS * ref['scale'][k], '%s %s' % (what, k)) for k in ('reward', 'q', 'coef')}
  worst['losses'] = assert_within(got['losses'], ref['losses'], C_GEN_LOSS * ref['scale']['losses'], what + ' losses')
  return worst


def check_head_fwd(got, ref, r32, what):
  assert np.array_equal(got['h'], r32['h']), what + ': h is not the float32 restatement bit for bit'
  return dict(logits=assert_within(got['logits'], ref['logits'], C_LOGIT * ref['logit_scale'], what + ' logits'),
              dh=assert_within(got['dh'], ref['dh'], C_DH * np.abs(ref['dh']), what + ' dh'))


def check_head_bwd(got, ref, r32, what):
  bad = np.flatnonzero(np.asarray(got['gb1']) != r32['gb1'])
  assert bad.size == 0 and np.isfinite(got['gb1']).all(), '%s: gb1 differs from the ordered float32 restatement in %d units' % (what, bad.size)
  return {k: assert_within(got[k], ref[k], c * ref['scale'][k], '%s %s' % (what, k))
          for k, c in (('gb1', C_GB1), ('gw2', C_GW2), ('gb2', C_GB2))}


def check_report(out, ema, ref, what):
  ref_out, ref_ema, scale, ema_scale = ref
  return dict(out=assert_within(out, ref_out, C_REPORT * scale, what + ' out'),
              ema=assert_within(ema, ref_ema, C_REPORT * ema_scale, what + ' ema'))


def check_plane_sums(got, ref, what):
  return assert_within(got, ref[0], C_PLANE * ref[1], what + ' plane sums')


def check_gp_direct(got, ref, scale, what):
  delta = C_GPNORM * ref['norm_scale']
  v_tol = ref['g_abs'] * (abs(float(f32(scale))) * coef_tol(ref['norm'], delta) + C_V * np.abs(ref['coef'])).reshape((-1,) + (1,) * (ref['v'].ndim - 1))
  return dict(norm=assert_within(got['norm'], ref['norm'], delta, what + ' norm'),
              term=assert_within(got['term'], ref['term'], term_tol(ref['norm'], delta), what + ' term'),
              v=assert_within(got['v'], ref['v'], v_tol, what + ' v'))
