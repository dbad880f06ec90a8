"""Float64 NumPy restatement of the evaluation metric's device path: the patch statistics
(``expo_patch_stats``), the histograms (``expo_stat_hist``), the crops of ``metrics.patch_windows`` and the whole of
``metrics.set_statistics``; plus CPU stand-ins with the signatures of ``_cabi.patch_stats`` / ``_cabi.stat_hist``, so the
host logic runs without a GPU and the device results have something to be compared with."""
import numpy as np
import torch

from tests import _area_ref

STAT_BOUND = 2e-6  # |expo_patch_stats - float64| on every statistic (the derivation is in tests/test_hip_metric.py)


def statistics(patches, unbiased=False, weights=(0.27, 0.67, 0.06)):
  """(N, h, w, 3) -> (N, 3) float64 [mean lum, 2 std lum, mean HLS saturation] as ``metrics.get_statistics`` defines
  them.  ``unbiased`` / ``weights``: the mutants of the device test."""
  p = np.clip(np.asarray(patches, dtype=np.float64), 0.0, 1.0)
  n = p.shape[0]
  lum = (p[..., 0] * weights[0] + p[..., 1] * weights[1] + p[..., 2] * weights[2]).reshape(n, -1)
  mx, mn = p.max(axis=-1), p.min(axis=-1)
  d = mx - mn
  den = np.where((mx + mn) * 0.5 < 0.5, mx + mn, 2.0 - mx - mn)
  sat = np.where(d > 0, d / np.maximum(den, 1e-12), 0.0).reshape(n, -1)
  return np.stack([lum.mean(axis=1), 2.0 * lum.std(axis=1, ddof=1 if unbiased else 0), sat.mean(axis=1)], axis=1)


def crops(master, records, c):
  """master (M, S, S, 3) array, records [(src, oy, ox)] clamped as the kernel clamps them -> (count, c, c, 3)."""
  m, s = master.shape[0], master.shape[1]
  out = []
  for src, oy, ox in np.asarray(records).reshape(-1, 3).tolist():
    src, oy, ox = min(max(src, 0), m - 1), min(max(oy, 0), s - c), min(max(ox, 0), s - c)
    out.append(master[src, oy:oy + c, ox:ox + c])
  return np.stack(out) if out else np.zeros((0, c, c, 3), master.dtype)


def histogram(stats, bins):
  """(q, 3) -> (3, bins) int: np.histogram(range=(0, 1)) per statistic, NaN removed first."""
  st = np.asarray(stats, dtype=np.float32).reshape(-1, 3)
  return np.stack([np.histogram(st[:, k][~np.isnan(st[:, k])], bins=bins, range=(0, 1))[0] for k in range(3)])


def patches(seed, n=48, size=64):
  """The generator of the device tests: patch p = clip(base_p + amp_p (U - 0.5), 0, 1) with base_p ~ U(0, 1)^3 and
  amp_p ~ U(0, 0.5) -> (n, size, size, 3) float32."""
  rng = np.random.default_rng(seed)
  base = rng.random((n, 1, 1, 3))
  amp = rng.random((n, 1, 1, 1)) * 0.5
  u = rng.random((n, size, size, 3))
  return np.clip(base + amp * (u - 0.5), 0.0, 1.0).astype(np.float32)


def edge_distance(stats, bins=32):
  """The smallest distance of any statistic to a multiple of 1 / bins."""
  v = np.asarray(stats, dtype=np.float64) * bins
  return float(np.abs(v - np.rint(v)).min() / bins)


def set_statistics(images_u8, windows, records):
  """``metrics.set_statistics`` in float64 from uint8 arrays and ``metrics.patch_windows``' draws: / 255 as float32
  (the definition of the input), then ``_area_ref.area_resize`` to 80 x 80, the 64 x 64 crops and the statistics, all
  in float64 (the device's float32 master is within ``_area_ref.BOUND`` of this one)."""
  master = np.stack([_area_ref.area_resize((images_u8[i].astype(np.float64) / 255.0).astype(np.float32)
                                           [y0:y0 + e, x0:x0 + e], 80) for i, y0, x0, e in windows])
  return statistics(crops(master, records, 64))


# ---- stand-ins with the signatures of the _cabi calls (CPU tensors) --------------------------------------------------------
def patch_stats(master, records, C, stats):
  assert records.dtype == torch.int32 and tuple(stats.shape) == (records.shape[0], 3)
  st = statistics(crops(master.float().numpy(), records.numpy(), C))
  stats.copy_(torch.from_numpy(st.astype(np.float32)))
  return stats


def stat_hist(stats, bins, counts):
  assert tuple(counts.shape) == (3, bins) and counts.dtype == torch.int32
  counts.copy_(torch.from_numpy(histogram(stats.numpy(), bins).astype(np.int32)))
  return counts


def patch(monkeypatch):
  """Route the five library calls of the metric's device path to the stand-ins."""
  from exposure_amd import _cabi
  _area_ref.patch(monkeypatch)
  monkeypatch.setattr(_cabi, 'patch_stats', patch_stats)
  monkeypatch.setattr(_cabi, 'stat_hist', stat_hist)
