"""A / B timing of the ragged fused chain (expo_chain_fused_fwd_ragged) and of evaluate.retouch_batch.

  (a) 16 fp16 images of mixed sizes (512x768 / 768x512 alternating, three of 1.3-1.9 MP): ONE ragged call against
      the 16 per-image expo_chain_fused_fwd launches;
  (b) 16 x 512x512 fp16 (BASELINE config 5's pixels) as a list through the ragged entry against ONE
      expo_chain_fused_fwd on the (16, 512, 512, 3) tensor;
  (c) retouch_batch on the 16 images of (a) against 16 retouch calls, in ms per image (agent on the 64x64 proxies +
      the full-resolution chain; random-init agent).

Device events around `--reps` calls, after warm-up, A and B alternating in one process for `--rounds` rounds; the
median over the rounds is reported.  (a) and (b) also report the device work alone (the same `--reps` calls captured
as one graph and replayed, A / B alternating) and the host time per call (enqueue): a call is bound by the larger.
Before timing, (a) and (b) check that A and B give bit-identical outputs.
usage: python tools/bench_ragged_infer.py [--rounds 7] [--reps 20] [--steps 8] [--out profiles/x.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import _cabi, evaluate, synthetic  # noqa: E402
from exposure_amd import agent as xagent  # noqa: E402
from exposure_amd.config import make_cfg  # noqa: E402

MIXED = [(512, 768), (768, 512)] * 6 + [(512, 768), (1024, 1280), (1200, 1600), (1536, 1024)]


def timed(fn, reps):
  """ms per call of fn over reps calls, device events on the current stream"""
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def ab(fa, fb, rounds, reps, warmup):
  for _ in range(warmup):
    fa()
    fb()
  torch.cuda.synchronize()
  ta, tb = [], []
  for r in range(rounds):
    first, second = (fa, fb) if r % 2 == 0 else (fb, fa)  # alternate which goes first
    t1, t2 = timed(first, reps), timed(second, reps)
    ta.append(t1 if r % 2 == 0 else t2)
    tb.append(t2 if r % 2 == 0 else t1)
  return dict(a_ms=statistics.median(ta), b_ms=statistics.median(tb), a_all=ta, b_all=tb)


def graphed(fn, reps):
  """reps calls of fn captured as one graph: its replay times the device work alone, without the host's share"""
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(reps):
      fn()
  torch.cuda.synchronize()
  return g


def device_ab(fa, fb, rounds, reps, warmup):
  ga, gb = graphed(fa, reps), graphed(fb, reps)
  r = ab(ga.replay, gb.replay, rounds, 1, warmup)
  return dict(a_ms=r['a_ms'] / reps, b_ms=r['b_ms'] / reps)


def host_us(fn, reps):
  """host time per call of fn (enqueue only; the device work drains after the clock stops)"""
  torch.cuda.synchronize()
  t = time.perf_counter()
  for _ in range(reps):
    fn()
  dt = time.perf_counter() - t
  torch.cuda.synchronize()
  return dt / reps * 1e6


def sequences(rng, n, steps, dev):
  ids = np.array([[(i + st) % 8 for st in range(steps)] for i in range(n)], dtype=np.int32).reshape(n, steps)
  p = np.zeros((n, steps, 24), dtype=np.float32)
  for i in range(n):
    for st in range(steps):
      fid = int(ids[i, st])
      p[i, st, :_cabi.NUM_PARAMS[fid]] = synthetic.make_params(rng, fid, 1)[0]
  return torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev)


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--steps', type=int, default=8, help='filter steps of (a) / (b) (config 5: 8)')
  ap.add_argument('--retouch-reps', type=int, default=3)
  ap.add_argument('--out', default=None, help='also write the JSON result here')
  args = ap.parse_args(argv)
  assert torch.cuda.is_available(), 'bench_ragged_infer needs a ROCm GPU'
  dev = torch.device('cuda:0')
  rng = np.random.default_rng(1)
  res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, rounds=args.rounds, reps=args.reps)

  # (a) mixed sizes
  xs = [torch.from_numpy(synthetic.make_images(rng, (1, h, w, 3), np.float16)).to(dev) for h, w in MIXED]
  ys_a, ys_b = [torch.empty_like(x) for x in xs], [torch.empty_like(x) for x in xs]
  ids, p = sequences(rng, len(xs), args.steps, dev)
  rows = [(ids[i:i + 1].contiguous(), p[i:i + 1].contiguous()) for i in range(len(xs))]

  def ragged_a():
    _cabi.chain_fused_fwd_ragged(ids, p, xs, ys_a)

  def per_image_a():
    for (ri, rp), x, y in zip(rows, xs, ys_b):
      _cabi.chain_fused_fwd(ri, rp, x, y)

  ragged_a()
  per_image_a()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(ys_a, ys_b)), '(a): ragged and per-image outputs differ'
  px = sum(h * w for h, w in MIXED)
  r = ab(ragged_a, per_image_a, args.rounds, args.reps, args.warmup)
  d = device_ab(ragged_a, per_image_a, args.rounds, args.reps, args.warmup)
  ha, hb = host_us(ragged_a, args.reps), host_us(per_image_a, args.reps)
  res['a_mixed'] = dict(images=len(MIXED), megapixels=px / 1e6, ragged_ms=r['a_ms'], per_image_ms=r['b_ms'],
                        ratio=r['a_ms'] / r['b_ms'], ragged_all=r['a_all'], per_image_all=r['b_all'],
                        device_ragged_ms=d['a_ms'], device_per_image_ms=d['b_ms'], device_ratio=d['a_ms'] / d['b_ms'],
                        host_ragged_us=ha, host_per_image_us=hb)
  print('(a) 16 mixed fp16 images (%.1f MP), %d steps: one ragged call %.4f ms, 16 per-image launches %.4f ms '
        '(ragged / per-image %.3f); device only (graph replay) %.4f / %.4f ms (%.3f); host per call %.1f / %.1f us'
        % (px / 1e6, args.steps, r['a_ms'], r['b_ms'], r['a_ms'] / r['b_ms'], d['a_ms'], d['b_ms'],
           d['a_ms'] / d['b_ms'], ha, hb))

  # (b) same size: the list through the ragged entry against the one-tensor launch
  x16 = torch.from_numpy(synthetic.make_images(rng, (16, 512, 512, 3), np.float16)).to(dev)
  y16, y16r = torch.empty_like(x16), torch.empty_like(x16)
  ids16, p16 = sequences(rng, 16, args.steps, dev)
  xl, yl = [x16[i] for i in range(16)], [y16r[i] for i in range(16)]

  def ragged_b():
    _cabi.chain_fused_fwd_ragged(ids16, p16, xl, yl)

  def dense_b():
    _cabi.chain_fused_fwd(ids16, p16, x16, y16)

  ragged_b()
  dense_b()
  torch.cuda.synchronize()
  assert torch.equal(y16, y16r), '(b): ragged and one-tensor outputs differ'
  r = ab(ragged_b, dense_b, args.rounds, args.reps, args.warmup)
  d = device_ab(ragged_b, dense_b, args.rounds, args.reps, args.warmup)
  ha, hb = host_us(ragged_b, args.reps), host_us(dense_b, args.reps)
  res['b_same_size'] = dict(shape=[16, 512, 512, 3], ragged_ms=r['a_ms'], tensor_ms=r['b_ms'],
                            ratio=r['a_ms'] / r['b_ms'], ragged_all=r['a_all'], tensor_all=r['b_all'],
                            device_ragged_ms=d['a_ms'], device_tensor_ms=d['b_ms'], device_ratio=d['a_ms'] / d['b_ms'],
                            host_ragged_us=ha, host_tensor_us=hb)
  print('(b) 16x512x512 fp16, %d steps: ragged list %.4f ms, one (16, 512, 512, 3) launch %.4f ms '
        '(ragged / tensor %.3f); device only (graph replay) %.4f / %.4f ms (%.3f); host per call %.1f / %.1f us'
        % (args.steps, r['a_ms'], r['b_ms'], r['a_ms'] / r['b_ms'], d['a_ms'], d['b_ms'], d['a_ms'] / d['b_ms'],
           ha, hb))

  # (c) the inference loop: retouch_batch on the 16 images against 16 retouch calls
  torch.manual_seed(0)
  ag = xagent.Agent(make_cfg()).to(dev)

  def batch_c():
    evaluate.retouch_batch(ag, xs)

  def single_c():
    for x in xs:
      evaluate.retouch(ag, x)

  r = ab(batch_c, single_c, args.rounds, args.retouch_reps, args.warmup)
  n = len(xs)
  res['c_retouch'] = dict(images=n, batch_ms_per_image=r['a_ms'] / n, single_ms_per_image=r['b_ms'] / n,
                          speedup=r['b_ms'] / r['a_ms'], batch_all=r['a_all'], single_all=r['b_all'])
  print('(c) retouch_batch on 16 mixed images %.3f ms / image, 16 retouch calls %.3f ms / image (speed-up %.2fx)'
        % (r['a_ms'] / n, r['b_ms'] / n, r['b_ms'] / r['a_ms']))
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
      fh.write(line + '\n')


if __name__ == '__main__':
  main()
