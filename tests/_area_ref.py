"""Float64 restatement of OpenCV's INTER_AREA (computeResizeAreaTab) and NumPy stand-ins for the three library calls
``datasets.build_pack`` / ``PackProvider`` make (``_cabi.decode_ragged``, ``area_resize_ragged``, ``pack_recut``), so
the host logic runs without a GPU and the device results have something to be compared with."""
import math

import numpy as np
import torch


def axis_weights(d, scale, side):
  """[(source index, weight)] of output index ``d`` along one axis, in source order."""
  f1 = d * scale
  f2 = f1 + scale
  cell = min(scale, side - f1)
  s1, s2 = math.ceil(f1), math.floor(f2)
  s2 = min(s2, side - 1)
  s1 = min(s1, s2)
  out = []
  if s1 - f1 > 1e-3:
    out.append((s1 - 1, (s1 - f1) / cell))
  for s in range(s1, s2):
    out.append((s, 1.0 / cell))
  if f2 - s2 > 1e-3:
    out.append((s2, min(min(f2 - s2, 1.0), cell) / cell))
  return out


def area_matrix(side, S):
  """(S, side) float64: row d holds the weights of output index d."""
  assert side >= S
  scale = side / S
  a = np.zeros((S, side))
  for d in range(S):
    for s, w in axis_weights(d, scale, side):
      a[d, s] = w
  return a


def area_resize(img, S, cols=None):
  """(side, side, C) -> (S, S, C) float64.  ``cols``: another (S, side) matrix for the column pass (the mutants of
  tests/test_datasets_host.py)."""
  a = area_matrix(img.shape[0], S)
  img = np.asarray(img, dtype=np.float64)
  rows = np.tensordot(a, img, axes=(1, 0))                      # (S, side, C)
  return np.tensordot(rows, a if cols is None else cols, axes=(1, 1)).transpose(0, 2, 1)  # (S, C, S) -> (S, S, C)


BOUND = 4e-6  # |out - float64| of expo_area_resize_ragged's fp32 output on inputs in [0, 1]


def max_err(got, want):
  """The comparison of the device tests: the largest |got - want| and where it sits."""
  err = np.abs(np.asarray(got, dtype=np.float64) - want)
  return float(err.max()), tuple(int(i) for i in np.unravel_index(err.argmax(), err.shape))


def tile_plan(side, S, tile_cols=4096):
  """The column tiles of area_resize_kernel (csrc/datasets.hip: tile_out_cols and the loop over ox0) for one window:
  [(ox0, ox1, c0, c1)], output columns [ox0, ox1) read from the source columns [c0, c1) held in one LDS tile."""
  scale = side / S
  per = int((tile_cols - 2) / scale)
  assert per >= 1, 'side / S too large for one LDS tile: the entry point refuses the window'
  plan = []
  for ox0 in range(0, S, per):
    ox1 = min(ox0 + per, S)
    c0 = axis_weights(ox0, scale, side)[0][0]
    c1 = axis_weights(ox1 - 1, scale, side)[-1][0] + 1
    plan.append((ox0, ox1, c0, c1))
  return plan


# (S, side) -> output columns per tile: the windows of tests/test_hip_datasets.py::test_area_resize_across_tile_seams.
# 4094 is the last single-tile side at S = 64, 4095 the first with a second tile (of one column), 5120 an integer scale
# (every 1e-3 edge decision sits on an integer), 6000 a seam in the middle for both output sizes of the recipes, and
# 8191 three tiles (8188 is the smallest side that gives three for any S).
SEAM_PLANS = {(64, 4094): [64], (64, 4095): [63, 1], (64, 5120): [51, 13], (64, 6000): [43, 21], (80, 6000): [54, 26],
              (64, 8191): [31, 31, 2]}


# ---- stand-ins with the signatures of the _cabi calls (CPU tensors) --------------------------------------------------------
def decode_ragged(codes, table, normalize, outs, workspace=None):
  assert normalize == 0
  t = table.cpu().numpy()
  for c, o in zip(codes, outs):
    k = c.cpu().numpy()
    k = np.repeat(k, 3, axis=2) if k.shape[2] == 1 else k[:, :, :3]
    o.copy_(torch.from_numpy(t[k].astype(np.float32)).reshape(o.shape))


def area_resize_ragged(xs, windows, S, out):
  for k, (i, y0, x0, side) in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
    x = xs[i].reshape(xs[i].shape[-3:]).double().cpu().numpy()
    r = area_resize(x[y0:y0 + side, x0:x0 + side], S)
    out[k] = torch.from_numpy(r.astype(np.float32)).to(out.dtype)
  return out


def recut(master, rec):
  """NumPy: out[r] = flip_r(master[src][oy:oy + C, ox:ox + C]) for an (M, S, S, 3) array and (count, 5) records of
  (src, oy, ox, flip, C)."""
  rows = []
  for src, oy, ox, flip, c in rec:
    a = master[src, oy:oy + c, ox:ox + c]
    rows.append(a[:, ::-1] if flip else a)
  return np.stack(rows) if rows else np.zeros((0,) + master.shape[1:], master.dtype)


def pack_recut(master, records, out):
  c = out.shape[1]
  rec = [tuple(r) + (c,) for r in records.cpu().numpy().tolist()]
  out.copy_(torch.from_numpy(np.ascontiguousarray(recut(master.cpu().numpy(), rec))))
  return out


def patch(monkeypatch):
  """Route the module's three library calls to the stand-ins."""
  from exposure_amd import _cabi
  monkeypatch.setattr(_cabi, 'decode_ragged', decode_ragged)
  monkeypatch.setattr(_cabi, 'area_resize_ragged', area_resize_ragged)
  monkeypatch.setattr(_cabi, 'pack_recut', pack_recut)
