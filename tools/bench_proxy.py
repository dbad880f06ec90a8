"""Timing of the agent's 64x64 proxies of a ragged batch, on the same device tensors:
  (a) the loop of retouch_batch's default path: torch.cat([make_low_res(im, 64) for im in images]) (torch's
      interpolate on an fp32 copy of every centre square);
  (b) make_low_res_batch(images, 64): one expo_bilinear_resize_ragged launch.
Shapes: 16 x 6000x4000 and 16 x 512x512, fp16 and fp32.  HIP events around `--reps` calls after warm-up, the two
alternating inside every round; median and range over `--rounds`.  Also end to end: retouch_batch with proxy='torch'
and proxy='device' on the same images, agent, z and dropout masks (host clock around a call that ends in a device
synchronise).  `--launch-counts` instead counts the device kernels of one call of (a) and (b) with torch's profiler
(a run of its own: tracing slows the host), or null where the profiler is not available.
usage: python tools/bench_proxy.py [--rounds 7] [--reps 10] [--out profiles/proxy_bench.json]
       python tools/bench_proxy.py --launch-counts"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import evaluate  # noqa: E402
from exposure_amd.agent import Agent  # noqa: E402
from exposure_amd.config import make_cfg  # noqa: E402

SHAPES = (('16x6000x4000', [(6000, 4000)] * 16), ('16x512x512', [(512, 512)] * 16))
SIZE = 64


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def sync_time(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3


def stats(ts):
  return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def kernel_launches(fn):
  """device kernels of one call, as torch's profiler sees them"""
  try:
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
      fn()
      torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
    return n or None
  except Exception:  # no profiler in this build: not measured
    return None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--launch-counts', action='store_true')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  if args.rounds < 5:
    ap.error('--rounds must be at least 5')
  dev = torch.device('cuda:0')
  cfg = make_cfg()
  torch.manual_seed(4)
  agent = Agent(cfg).to(dev)
  res = dict(proxies=[], end_to_end=[])
  for name, sizes in SHAPES:
    for dtype, dname in ((torch.float16, 'f16'), (torch.float32, 'f32')):
      torch.manual_seed(len(sizes))
      images = [(torch.rand((1, h, w, 3), device=dev)**2.2).to(dtype) for h, w in sizes]
      loop = lambda: torch.cat([evaluate.make_low_res(im, SIZE) for im in images])
      batch = lambda: evaluate.make_low_res_batch(images, SIZE)
      if args.launch_counts:
        r = dict(shape=name, dtype=dname, images=len(sizes), torch_loop_launches=kernel_launches(loop),
                 device_batch_launches=kernel_launches(batch))
        print(json.dumps(r), flush=True)
        res.setdefault('launches', []).append(r)
        continue
      for _ in range(3):
        loop(), batch()
      torch.cuda.synchronize()
      ta, tb = [], []
      for _ in range(args.rounds):
        ta.append(timed(loop, args.reps))
        tb.append(timed(batch, args.reps))
      centre = sum(min(h, w)**2 for h, w in sizes) * 3
      r = dict(shape=name, dtype=dname, torch_loop=stats(ta), device_batch=stats(tb),
               speedup=statistics.median(ta) / statistics.median(tb),
               # bytes by count: (a) reads the centre squares and writes their fp32 copies; (b) reads 4 taps per output
               torch_loop_copy_bytes=centre * (images[0].element_size() + 4),
               device_batch_tap_bytes=len(sizes) * SIZE * SIZE * 4 * 3 * images[0].element_size(),
               worst_abs_difference=float((loop().double() - batch().double()).abs().max()))
      print(json.dumps(r), flush=True)
      res['proxies'].append(r)
      # end to end on the same images: fixed z and dropout masks, so both paths run the same schedule
      g = torch.Generator().manual_seed(7)
      z = torch.rand(len(sizes), cfg.z_dim, generator=g).to(dev)
      masks = [[(torch.rand(len(sizes), 4096, generator=g) < 0.5).float().to(dev) for _ in range(2)]
               for _ in range(cfg.test_steps)]
      run = {p: (lambda p=p: evaluate.retouch_batch(agent, images, z=z, dropout_masks=masks, proxy=p))
             for p in evaluate.PROXIES}
      for p in run:
        run[p]()
      te = {p: [] for p in run}
      for _ in range(args.rounds):
        for p in run:
          te[p].append(sync_time(run[p]))
      r = dict(shape=name, dtype=dname, retouch_batch_torch=stats(te['torch']), retouch_batch_device=stats(te['device']),
               speedup=statistics.median(te['torch']) / statistics.median(te['device']))
      print(json.dumps(r), flush=True)
      res['end_to_end'].append(r)
      del images, run, loop, batch
      torch.cuda.empty_cache()
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
