"""NumPy float32 restatement of ``expo_bilinear_resize_ragged`` (include/exposure_hip.h), operation for operation, a
float64 evaluation of the same interpolation, the derived bound against ``evaluate.make_low_res``, and a CPU stand-in
with ``_cabi.bilinear_resize_ragged``'s signature, so the host logic runs without a GPU and the device results have
something to be compared with bit for bit."""
import numpy as np
import torch

f32 = np.float32


def axis(side, S):
  """(i0, i1, l0, l1) of every output index along one axis: float32, every operation rounded on its own."""
  scale = f32(side) / f32(S)
  d = np.arange(S, dtype=np.float32)
  t = scale * (d + f32(0.5))             # the product is rounded,
  src = np.maximum(t - f32(0.5), f32(0))  # then the subtraction
  i0 = src.astype(np.int32)
  i1 = i0 + (i0 < side - 1)
  l1 = src - i0.astype(np.float32)
  l0 = f32(1) - l1
  assert src.dtype == l0.dtype == l1.dtype == np.float32 and i0.min() >= 0 and i1.max() <= side - 1
  return i0, i1, l0, l1


def bilinear_resize(win, S, out_dtype=np.float32):
  """(side, side, 3) float16 / float32 window -> (S, S, 3) ``out_dtype``: the kernel's definition."""
  assert win.shape[0] == win.shape[1]
  x = np.asarray(win).astype(np.float32)  # the taps are widened first
  i0, i1, hl0, hl1 = axis(x.shape[0], S)
  j0, j1, wl0, wl1 = axis(x.shape[0], S)
  hl0, hl1 = hl0[:, None, None], hl1[:, None, None]
  wl0, wl1 = wl0[None, :, None], wl1[None, :, None]
  a, b = x[i0][:, j0], x[i0][:, j1]
  c, d = x[i1][:, j0], x[i1][:, j1]
  top = wl0 * a + wl1 * b
  bot = wl0 * c + wl1 * d
  v = hl0 * top + hl1 * bot
  assert v.dtype == np.float32
  return v.astype(out_dtype)  # round to nearest even


def axis64(side, S):
  scale = side / S
  src = np.maximum(scale * (np.arange(S) + 0.5) - 0.5, 0.0)
  i0 = np.minimum(src.astype(np.int64), side - 1)
  i1 = i0 + (i0 < side - 1)
  l1 = src - i0
  return i0, i1, 1.0 - l1, l1


def bilinear_resize64(win, S):
  """The same interpolation evaluated in float64 (exact coordinates up to 2^-53)."""
  x = np.asarray(win).astype(np.float64)
  i0, i1, hl0, hl1 = axis64(x.shape[0], S)
  j0, j1, wl0, wl1 = i0, i1, hl0, hl1
  hl0, hl1 = hl0[:, None, None], hl1[:, None, None]
  wl0, wl1 = wl0[None, :, None], wl1[None, :, None]
  return hl0 * (wl0 * x[i0][:, j0] + wl1 * x[i0][:, j1]) + hl1 * (wl0 * x[i1][:, j0] + wl1 * x[i1][:, j1])


def parity_bound(win, S, out_dtype):
  """(S, S, 3) bound on |restatement - another float32 evaluation of the same bilinear form| (torch's, or float64):
  a compiler may contract ``scale * (d + 0.5) - 0.5`` into one fma, so a source coordinate differs by at most
  2 ulp_f32(side) per axis; the form is continuous and piecewise linear in each coordinate with slope at most R (max
  minus min of the four taps), so the value moves by at most (dh + dw) R; the float32 evaluation of the form itself adds
  at most 8 * 2^-24 * M (M the taps' largest magnitude); one ulp of the storage type when the output is fp16."""
  x = np.asarray(win).astype(np.float64)
  side = x.shape[0]
  i0, i1, _, _ = axis(side, S)
  taps = np.stack([x[r][:, c] for r in (i0, i1) for c in (i0, i1)])
  R = taps.max(0) - taps.min(0)
  M = np.abs(taps).max(0)
  delta = 2.0 * float(np.spacing(f32(side)))
  bound = 2.0 * delta * R + 8.0 * 2.0**-24 * M
  if np.dtype(out_dtype) == np.float16:
    bound = bound + np.spacing(np.abs(bilinear_resize64(win, S)).astype(np.float16)).astype(np.float64)
  return bound


# ---- stand-in with the signature of the _cabi call (CPU tensors) -----------------------------------------------------------
def bilinear_resize_ragged(xs, windows, S, out):
  np_dt = np.float16 if out.dtype == torch.float16 else np.float32
  for k, (i, y0, x0, side) in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
    x = xs[i].reshape(xs[i].shape[-3:]).cpu().numpy()
    out[k] = torch.from_numpy(bilinear_resize(x[y0:y0 + side, x0:x0 + side], S, np_dt))
  return out


def patch(monkeypatch):
  """Route the module's library call to the stand-in."""
  from exposure_amd import _cabi
  monkeypatch.setattr(_cabi, 'bilinear_resize_ragged', bilinear_resize_ragged)
