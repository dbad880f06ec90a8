"""Timing of the masked fused inference pass at 16x512x512 and 64x512x512, fp16, 5 steps, with
sharp = 1.0, min_strength = 0.3, seeded filter ids in 0..7, parameters from synthetic.make_params and squashed mask rows
5 tanh(N(0,1)).  Three ways through the same images, timed with device events around `--reps` calls after warm-up,
alternating round by round, median of `--rounds`:
  masked_fused   one expo_chain_fused_masked_fwd_ragged call (the images as a list of views)
  five_launches  the schedule without it: five expo_filter_apply_dispatch_fwd launches, two buffers swapping roles
  unmasked_fused expo_chain_fused_fwd_ragged on the same ids and parameters, for scale (other results: no masks)
The C entry points are called through ctypes with the argument arrays built once, so the windows hold device work and
not the binding's per-image checks.  Also reports the largest difference between the first two's outputs (one fp16
rounding per step against one at the end).
usage: python tools/bench_masked_chain.py [--rounds 7] [--reps 200] [--out profiles/masked_chain.md]"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import _cabi, synthetic  # noqa: E402

STEPS, H, W = 5, 512, 512
SHARP, MIN_STRENGTH = 1.0, 0.3


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) * 1e3 / reps  # us


def case(n, rounds, reps, dev):
  lib = _cabi.load()
  rng = np.random.default_rng(n)
  x = torch.from_numpy(synthetic.make_images(rng, (n, H, W, 3), np.float16)).to(dev)
  ids_np = rng.integers(0, 8, (n, STEPS)).astype(np.int32)
  prm_np = np.zeros((n, STEPS, 24), dtype=np.float32)
  for i in range(n):
    for k in range(STEPS):
      fid = int(ids_np[i, k])
      prm_np[i, k, :synthetic.NUM_PARAMS[fid]] = synthetic.make_params(rng, fid, 1)[0]
  mp_np = (5.0 * np.tanh(rng.standard_normal((n, STEPS, 6)))).astype(np.float32)
  ids, prm, mp = (torch.from_numpy(a).to(dev) for a in (ids_np, prm_np, mp_np))
  # per-step rows of the five launches
  ids_k = [ids[:, k].contiguous() for k in range(STEPS)]
  prm_k = [prm[:, k].contiguous() for k in range(STEPS)]
  mp_k = [mp[:, k].contiguous() for k in range(STEPS)]
  y_fused, y_plain, a, b = (torch.empty_like(x) for _ in range(4))
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())
  xs = _cabi._ptr_array(list(x.unbind(0)))
  ys = _cabi._ptr_array(list(y_fused.unbind(0)))
  yp = _cabi._ptr_array(list(y_plain.unbind(0)))
  hs, ws = (ctypes.c_int * n)(*[H] * n), (ctypes.c_int * n)(*[W] * n)

  def masked_fused():
    rc = lib.expo_chain_fused_masked_fwd_ragged(ptr(ids), ptr(prm), ptr(mp), STEPS, SHARP, MIN_STRENGTH, xs, ys, hs, ws,
                                                n, _cabi.EXPO_F16, 0, _cabi.EXPO_TAP_STORAGE, None, stream)
    assert rc == 0, lib.expo_last_error()

  def five_launches():
    src, dst = x, a
    for k in range(STEPS):
      rc = lib.expo_filter_apply_dispatch_fwd(ptr(ids_k[k]), ptr(src), ptr(dst), ptr(prm_k[k]), ptr(mp_k[k]), SHARP,
                                              MIN_STRENGTH, n, H, W, _cabi.EXPO_F16, stream)
      assert rc == 0, lib.expo_last_error()
      src, dst = dst, (b if dst is a else a)

  def unmasked_fused():
    rc = lib.expo_chain_fused_fwd_ragged(ptr(ids), ptr(prm), STEPS, xs, yp, hs, ws, n, _cabi.EXPO_F16, stream)
    assert rc == 0, lib.expo_last_error()

  fns = dict(masked_fused=masked_fused, five_launches=five_launches, unmasked_fused=unmasked_fused)
  for fn in fns.values():  # warm-up: code objects, clocks
    for _ in range(20):
      fn()
  torch.cuda.synchronize()
  stepwise = a if STEPS % 2 else b  # the buffer the last of the five launches wrote
  diff = float((y_fused.float() - stepwise.float()).abs().max())
  scale = float(stepwise.float().abs().max())
  ts = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      ts[k].append(timed(fn, reps))
  res = {k: dict(us=statistics.median(v), us_min=min(v), us_max=max(v)) for k, v in ts.items()}
  res['shape'] = '%dx%dx%d' % (n, H, W)
  res['max_abs_diff_fused_vs_five'] = diff
  res['max_abs_value'] = scale
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=200)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'masked_chain.md'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_masked_chain needs a ROCm GPU'
  dev = torch.device('cuda:0')
  rows = [case(n, args.rounds, args.reps, dev) for n in (16, 64)]
  px_bytes = lambda n: n * H * W * 3 * 2
  lines = ['# Masked fused chain: fp16, %d steps, median of %d rounds x %d calls (us; min .. max)' % (STEPS, args.rounds,
                                                                                                   args.reps),
           '', 'Device: %s' % torch.cuda.get_device_name(0), '',
           '| shape | masked fused | five launches | unmasked fused | five / fused | fused GB/s (12 B/px) | max abs diff fused vs five |',
           '|---|---|---|---|---|---|---|']
  for n, r in zip((16, 64), rows):
    cell = lambda k: '%.1f (%.1f .. %.1f)' % (r[k]['us'], r[k]['us_min'], r[k]['us_max'])
    lines.append('| %s | %s | %s | %s | %.2f | %.0f | %.3e (values up to %.3g) |' % (
        r['shape'], cell('masked_fused'), cell('five_launches'), cell('unmasked_fused'),
        r['five_launches']['us'] / r['masked_fused']['us'], 2 * px_bytes(n) / (r['masked_fused']['us'] * 1e-6) / 1e9,
        r['max_abs_diff_fused_vs_five'], r['max_abs_value']))
  text = '\n'.join(lines) + '\n'
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)
  print(text)


if __name__ == '__main__':
  main()
