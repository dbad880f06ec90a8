"""TEST-ONLY helpers of the per-image dispatch for any cfg.curve_steps (``expo_filter_dispatch_curves_*``,
``expo_heads_regress_curves_*``): the float64 references, step-count aware where ``tests/_agent_glue_ref.py`` is written
for 8 steps, the shared input cases, and oracle-backed CPU stand-ins for the four ``exposure_amd._cabi`` bindings layered
on ``tests/_fake_hip.fake_hip``."""
import contextlib
import functools
from unittest import mock

import numpy as np
import torch

from exposure_amd import synthetic
from oracle import filters_np as fnp
from oracle import filters_torch as ft
from tests import _agent_glue_ref as R
from tests._fake_hip import fake_hip

f32, f64 = np.float32, np.float64
WIDE = 48  # EXPO_MAX_PARAMS_CURVES
UNUSED = 1e30  # what lies behind a filter's parameters in the test rows: nothing may read it


def num_params(fid, steps):
  return steps if fid == 4 else 3 * steps if fid == 7 else fnp.NUM_PARAMS[fid]


# ---- dispatch -----------------------------------------------------------------------------------------------------------
def curve_row(rng, fid, steps):
  lo, hi = (0.5, 2.0) if fid == 4 else (0.9, 1.1)
  return rng.uniform(lo, hi, num_params(fid, steps)).astype(f32)


def make_inputs(seed, shape, np_dtype, steps):
  """x in about [-0.26, 1.5] (exact knots j / L written in where L is a power of two), dy ~ N(0, 1).  The lower end is
  where the images' many near-black pixels land, and is therefore no multiple of 1/5 or 1/12: -0.25 is -3/12, which
  would count a percent of the elements as lying on a knot of the 12-step curve."""
  rng = np.random.default_rng(seed)
  x = (synthetic.make_images(rng, shape, np_dtype).astype(f32) * f32(1.76) - f32(0.26)).astype(np_dtype)
  if steps in (8, 16):
    flat = x.reshape(-1)
    flat[::41] = (np.arange(flat[::41].size) % (steps + 1)).astype(f32) / steps
  dy = synthetic.make_grad(rng, shape, np_dtype)
  return x, dy


def make_rows(seed, ids, steps, hump_rows=()):
  """(N, 48) rows: the filter's parameters in front, UNUSED behind.  ``hump_rows``: Tone / Color rows given a curve that
  rises above 1 (outside the reference's ranges), so that the fused penalty is live for a curve image."""
  rng = np.random.default_rng(seed)
  rows = np.full((len(ids), WIDE), UNUSED, dtype=f32)
  for i, fid in enumerate(ids):
    if fid < 0:
      continue
    p = num_params(int(fid), steps)
    if fid in (4, 7):
      rows[i, :p] = curve_row(rng, int(fid), steps)
      if i in hump_rows and steps >= 2:
        hump = np.where(np.arange(steps) < (steps + 1) // 2, 2.0, -0.5).astype(f32)
        rows[i, :p] = np.tile(hump, p // steps)
    else:
      rows[i, :p] = synthetic.make_params(rng, int(fid), 1)[0]
  return rows


def on_knot_mask(x64, steps):
  """Elements within rounding of a knot of a step count that is no power of two: two equally valid sub-gradients
  (tests/test_curve_steps.py::check_generic_curve)."""
  if steps & (steps - 1) == 0:
    return np.zeros(x64.shape, bool)
  return np.abs(x64 * steps - np.round(x64 * steps)) < 1e-6


def dispatch_oracle(x, dy, ids, rows, steps, dpen=None):
  """float64, image by image -> y, penalty, dx, dparams (N, 48), A (N, 48): the sums of the absolute terms of dparams
  (``curve_grad_abs_pieces`` for one-step curves, whose every term is exactly 0)."""
  n = x.shape[0]
  x64, dy64 = x.astype(f64), dy.astype(f64)
  y, dx = np.zeros_like(x64), np.zeros_like(x64)
  dp, adp = np.zeros((n, WIDE)), np.zeros((n, WIDE))
  cnt = x.shape[1] * x.shape[2] * 3
  for i, fid in enumerate(ids):
    fid = int(fid)
    if fid < 0:
      continue
    p = num_params(fid, steps)
    prm = rows[i:i + 1, :p].astype(f64)
    y[i:i + 1] = fnp.process_packed(fid, x64[i:i + 1], prm)
    g = dy64[i:i + 1]
    if dpen is not None:
      g = g + 2.0 * np.maximum(y[i:i + 1] - 1, 0) * float(dpen[i]) / cnt
    gx, gp = fnp.backward_packed(fid, x64[i:i + 1], prm, g)
    dx[i:i + 1], dp[i, :p] = gx, gp[0]
    a_of = fnp.curve_grad_abs_pieces if (fid in (4, 7) and steps == 1) else fnp.param_grad_abs
    adp[i, :p] = a_of(fid, x64[i:i + 1], prm, g)[0]
  pen = np.mean(np.maximum(y - 1, 0)**2, axis=(1, 2, 3))
  return y, pen, dx, dp, adp


# ---- heads --------------------------------------------------------------------------------------------------------------
def heads_inputs(abi_ids, n, mask_features, seed, steps):
  """``tests/_agent_glue_ref.heads_inputs``'s recipe with heads as wide as the step count makes them and 48-wide dparams."""
  rng = np.random.default_rng(seed)
  raws = [(1.5 * rng.standard_normal((n, num_params(fid, steps) + mask_features))).astype(f32) for fid in abi_ids]
  h = len(abi_ids)
  selected = ((np.arange(n) + (0 if n > 1 else 3)) % (h + 1) - 1).astype(np.int32)
  special = (20.0, -20.0, 100.0, -100.0, 0.0)
  for r in range(n):
    block = r // (h + 1)
    if 1 <= block <= len(special):
      for raw in raws:
        raw[r] = special[block - 1]
  dparams = rng.standard_normal((n, WIDE)).astype(f32)
  return raws, selected, dparams


def _cfg_and_shift(fid, ranges, steps):
  cfg, shift = R._cfg_and_shift(fid, ranges)
  return dict(cfg, curve_steps=steps), shift


def heads_fwd(raws, abi_ids, ranges, selected, steps):
  """expo_heads_regress_curves_fwd in float64: (n, 48)."""
  ranges = np.asarray(ranges, dtype=f32).astype(f64)
  n = raws[0].shape[0]
  out = np.zeros((n, WIDE))
  for j, (raw, fid) in enumerate(zip(raws, abi_ids)):
    rows = np.flatnonzero(np.asarray(selected) == j)
    if len(rows) == 0:
      continue
    p = num_params(fid, steps)
    cfg, shift = _cfg_and_shift(fid, ranges, steps)
    f = np.asarray(raw)[rows, :p].astype(f64) + shift
    with np.errstate(over='ignore'):
      out[rows, :p] = fnp.regress_packed(fid, f, cfg)
  return out


def heads_bwd(raws, abi_ids, ranges, selected, dparams, steps):
  """expo_heads_regress_curves_bwd in float64: (d raw of every head, the sums of the absolute terms).  A curve head's line
  is element-wise (dp t01'(x + b) (hi - lo)) over its L or 3 L features; every other head is the 8-step reference's."""
  ranges64 = np.asarray(ranges, dtype=f32).astype(f64)
  _, _, tl, th, tb, cl, ch, cb, _ = ranges64
  selected = np.asarray(selected)
  dparams = np.asarray(dparams, dtype=f64)
  dt01 = lambda v: 0.5 * (1.0 - np.tanh(v)**2)
  adt01 = lambda v: 0.5 * (1.0 + np.tanh(v)**2)
  draws, scales = [], []
  for j, (raw, fid) in enumerate(zip(raws, abi_ids)):
    raw64 = np.asarray(raw, dtype=f64)
    if fid in (4, 7):
      g, a = np.zeros_like(raw64), np.zeros_like(raw64)
      rows = np.flatnonzero(selected == j)
      p = num_params(fid, steps)
      xs, dp = raw64[rows, :p], dparams[rows, :p]
      b, width = (tb, th - tl) if fid == 4 else (cb, ch - cl)
      g[rows, :p], a[rows, :p] = dp * dt01(xs + b) * width, np.abs(dp) * adt01(xs + b) * abs(width)
    else:
      only = np.where(selected == j, 0, -1)
      d, s = R.heads_bwd([raw], [fid], ranges, only, dparams[:, :R.MAX_PARAMS])
      g, a = d[0], s[0]
    draws.append(g)
    scales.append(a)
  return draws, scales


# ---- CPU stand-ins of the bindings --------------------------------------------------------------------------------------
def _dispatch_curves_fwd(calls, ids, x, y, params, curve_steps, penalty=None, workspace=None):
  calls['dispatch_fwd'] += 1
  for n in range(x.shape[0]):
    fid = int(ids[n])
    if fid < 0:
      y[n].zero_()
    else:
      p = params[n:n + 1, :num_params(fid, curve_steps)].contiguous()
      y[n:n + 1].copy_(ft.process_packed(fid, x[n:n + 1].double(), p.double()).to(y.dtype))
  if penalty is not None:
    penalty.copy_(((y.double() - 1).clamp_min(0)**2).mean(dim=(1, 2, 3)).float())


def _dispatch_curves_bwd(calls, ids, x, dy, dx, params, dparams, curve_steps, dpenalty=None, hsv_grad_mode=0, workspace=None):
  calls['dispatch_bwd'] += 1
  dparams.zero_()
  cnt = x.shape[1] * x.shape[2] * 3
  for n in range(x.shape[0]):
    fid = int(ids[n])
    if fid < 0:
      if dx is not None:
        dx[n].zero_()
      continue
    width = num_params(fid, curve_steps)
    p = params[n:n + 1, :width].contiguous().double()
    xi = x[n:n + 1].double()
    g = dy[n:n + 1].double()
    if dpenalty is not None:
      g = g + 2.0 * (ft.process_packed(fid, xi, p) - 1).clamp_min(0) * float(dpenalty[n]) / cnt
    with torch.enable_grad():
      gx, gp = ft.backward_packed(fid, xi, p, g, hsv_grad_mode)
    if dx is not None:
      dx[n:n + 1].copy_(gx.to(dx.dtype))
    dparams[n, :width] = gp[0].float()


def _heads_curves_fwd(calls, raws, abi_ids, ranges, selected, params, curve_steps):
  calls['heads_fwd'] += 1
  ref = heads_fwd([r.detach().numpy() for r in raws], abi_ids, ranges, selected.numpy(), curve_steps)
  params.copy_(torch.from_numpy(ref).float())


def _heads_curves_bwd(calls, raws, draws, abi_ids, ranges, selected, dparams, curve_steps):
  calls['heads_bwd'] += 1
  ref, _ = heads_bwd([r.detach().numpy() for r in raws], abi_ids, ranges, selected.numpy(), dparams.numpy(), curve_steps)
  for d, g in zip(draws, ref):
    d.copy_(torch.from_numpy(g).float())


@contextlib.contextmanager
def fake_hip_curves():
  """``fake_hip()`` plus the four bindings of the dispatch for any cfg.curve_steps; yields the call counts."""
  calls = dict(dispatch_fwd=0, dispatch_bwd=0, heads_fwd=0, heads_bwd=0)
  bind = lambda fn: functools.partial(fn, calls)
  with fake_hip(), mock.patch.multiple('exposure_amd._cabi', dispatch_curves_fwd=bind(_dispatch_curves_fwd),
                                       dispatch_curves_bwd=bind(_dispatch_curves_bwd),
                                       heads_regress_curves_fwd=bind(_heads_curves_fwd),
                                       heads_regress_curves_bwd=bind(_heads_curves_bwd)):
    yield calls
