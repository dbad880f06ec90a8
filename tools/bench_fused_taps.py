"""Timing of the tap kernels (expo_chain_fused_fwd_taps): the fused inference pass that also writes the image after
chosen steps.  16 x 512x512 fp16, the 8-step sequence of bench.py's chain (one filter of each kind), cases:

  (a) no taps (expo_chain_fused_fwd);                     (b) 7 U8 taps + y;
  (c) 7 U8 taps, y NULL;                                  (d) 7 storage (fp16) taps + y;
  (e) today's way to the same pictures: 8 per-step expo_filter_fwd launches, each followed by the torch u8 encode;
  (f) one 24 MP image (4000x6000), 5 steps, 4 U8 taps + y, against the same call without taps;
  (g) 7 U16 taps + y;                                     (h) the picture only: a U16 tap of the last step + y;
  (i) the picture only as a storage tap + y (what (h) is compared with, as (g) with (d));
  (j) - (m) fp32 storage, 16 x 512x512, against the fp32 call without taps: 7 U16 taps + y, 7 fp32 storage taps + y,
      the U16 picture + y, the fp32 storage picture + y.

Device events around `--reps` calls after warm-up; every case is timed against (a) in the same process, A and B
alternating for `--rounds` rounds; medians.  Each case is reported against its algorithmic bytes (12 B/px + 3 B/px per
U8 tap, + 6 B/px per fp16 or U16 tap, fp32 storage: 24 B/px + 12 B/px per fp32 tap), as effective TB/s.  Also the CLI: `evaluate --step-by-step --batch 16` on 16 PNGs of
mixed sizes against `--step-by-step --stepwise`, wall time per image (one run each, after a warm-up run).
usage: python tools/bench_fused_taps.py [--rounds 7] [--reps 20] [--out profiles/x.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import _cabi, evaluate, synthetic  # noqa: E402

SEQ = [0, 1, 2, 3, 4, 5, 6, 7]  # E, G, W, S+, T, Ct, BW, C
MIXED = [(512, 768), (768, 512)] * 6 + [(512, 768), (1024, 1280), (1200, 1600), (1536, 1024)]


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def ab(fa, fb, rounds, reps, warmup=3):
  for _ in range(warmup):
    fa()
    fb()
  torch.cuda.synchronize()
  ta, tb = [], []
  for r in range(rounds):
    first, second = (fa, fb) if r % 2 == 0 else (fb, fa)
    t1, t2 = timed(first, reps), timed(second, reps)
    ta.append(t1 if r % 2 == 0 else t2)
    tb.append(t2 if r % 2 == 0 else t1)
  return statistics.median(ta), statistics.median(tb)


def sequence(rng, n, steps, dev):
  ids = np.array([SEQ[:steps]] * n, dtype=np.int32)
  p = np.zeros((n, steps, 24), dtype=np.float32)
  for i in range(n):
    for st in range(steps):
      fid = int(ids[i, st])
      p[i, st, :_cabi.NUM_PARAMS[fid]] = synthetic.make_params(rng, fid, 1)[0]
  return torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev)


def case(name, ms_a, ms_b, px, extra_bpp, base_bpp=12):
  b = px * (base_bpp + extra_bpp)
  return dict(case=name, a_ms=ms_a, b_ms=ms_b, ratio=ms_b / ms_a, bytes=b, tbps=b / (ms_b * 1e-3) / 1e12,
              a_tbps=px * base_bpp / (ms_a * 1e-3) / 1e12)


def cli_wall(paths, extra, out):
  t0 = time.perf_counter()
  evaluate.main(['--seed', '1', '--step-by-step', '--out', out, *extra, *paths])
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3 / len(paths)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  rng = np.random.default_rng(0)
  res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, cases=[])
  n, h, w, steps = 16, 512, 512, 8
  x = torch.from_numpy(synthetic.make_images(rng, (n, h, w, 3), np.float16)).to(dev)
  y = torch.empty_like(x)
  ids, p = sequence(rng, n, steps, dev)
  px = n * h * w
  m7 = (1 << 7) - 1  # every step but the last (the shipped agent's intermediates)
  u8 = torch.empty((7, n, h, w, 3), dtype=torch.uint8, device=dev)
  st = torch.empty((7, n, h, w, 3), dtype=torch.float16, device=dev)
  # correctness guard before timing: y of the tap call is the plain call's
  y0 = torch.empty_like(x)
  _cabi.chain_fused_fwd(ids, p, x, y0)
  _cabi.chain_fused_fwd_taps(ids, p, x, y, m7, u8)
  assert torch.equal(y.view(torch.int16), y0.view(torch.int16))

  def fa():
    _cabi.chain_fused_fwd(ids, p, x, y)

  def fb():
    _cabi.chain_fused_fwd_taps(ids, p, x, y, m7, u8)

  def fc():
    _cabi.chain_fused_fwd_taps(ids, p, x, None, m7, u8)

  def fd():
    _cabi.chain_fused_fwd_taps(ids, p, x, y, m7, st)

  bufs = [torch.empty_like(x) for _ in range(2)]
  prow = [p[:, k, :_cabi.NUM_PARAMS[SEQ[k]]].contiguous() for k in range(steps)]

  def fe():  # the per-step schedule: one launch per step, then the torch encode of each picture but the last
    cur = x
    for k in range(steps):
      nxt = bufs[k % 2]
      _cabi.filter_fwd(SEQ[k], cur, nxt, prow[k])
      if k < steps - 1:
        u8[k].copy_(evaluate.encode_u8(nxt))
      cur = nxt

  for name, fn, extra in (('b_7u8_y', fb, 21), ('c_7u8_noy', fc, 21 - 6), ('d_7f16_y', fd, 42),
                          ('e_per_step_torch_encode', fe, 21)):
    a, b = ab(fa, fn, args.rounds, args.reps)
    res['cases'].append(case(name, a, b, px, extra))
    print(json.dumps(res['cases'][-1]), flush=True)
  # (f) one 24 MP image, 5 steps, 4 U8 taps
  big = torch.from_numpy(synthetic.make_images(rng, (1, 4000, 6000, 3), np.float16)).to(dev)
  yb = torch.empty_like(big)
  idb, pb = sequence(rng, 1, 5, dev)
  tb = torch.empty((4, 1, 4000, 6000, 3), dtype=torch.uint8, device=dev)
  a, b = ab(lambda: _cabi.chain_fused_fwd(idb, pb, big, yb), lambda: _cabi.chain_fused_fwd_taps(idb, pb, big, yb, 15, tb),
            args.rounds, max(2, args.reps // 4))
  res['cases'].append(case('f_24mp_5steps_4u8_y', a, b, 4000 * 6000, 12))
  print(json.dumps(res['cases'][-1]), flush=True)
  del big, yb, tb
  # (g) - (i) U16 taps, fp16 storage: the tap planes are the storage taps' bytes
  last = 1 << (steps - 1)
  u16 = torch.empty((7, n, h, w, 3), dtype=torch.uint16, device=dev)
  _cabi.chain_fused_fwd_taps(ids, p, x, y, m7, u16)
  assert torch.equal(y.view(torch.int16), y0.view(torch.int16))
  _cabi.chain_fused_fwd_taps(ids, p, x, y, last, st[:1])
  assert torch.equal(evaluate.encode_u16(st[0]).view(torch.int16), evaluate.encode_u16(y0).view(torch.int16))
  for name, fn, extra in (('g_7u16_y', lambda: _cabi.chain_fused_fwd_taps(ids, p, x, y, m7, u16), 42),
                          ('h_u16_picture_y', lambda: _cabi.chain_fused_fwd_taps(ids, p, x, y, last, u16[:1]), 6),
                          ('i_f16_picture_y', lambda: _cabi.chain_fused_fwd_taps(ids, p, x, y, last, st[:1]), 6)):
    a, b = ab(fa, fn, args.rounds, args.reps)
    res['cases'].append(case(name, a, b, px, extra))
    print(json.dumps(res['cases'][-1]), flush=True)
  # (j) - (m) the same with fp32 storage: the U16 planes go through the per-wave LDS stage
  x32 = x.float()
  y32 = torch.empty_like(x32)
  st32 = torch.empty((7, n, h, w, 3), dtype=torch.float32, device=dev)

  def fa32():
    _cabi.chain_fused_fwd(ids, p, x32, y32)

  for name, fn, extra in (('j_f32_7u16_y', lambda: _cabi.chain_fused_fwd_taps(ids, p, x32, y32, m7, u16), 42),
                          ('k_f32_7f32_y', lambda: _cabi.chain_fused_fwd_taps(ids, p, x32, y32, m7, st32), 84),
                          ('l_f32_u16_picture_y', lambda: _cabi.chain_fused_fwd_taps(ids, p, x32, y32, last, u16[:1]), 6),
                          ('m_f32_f32_picture_y', lambda: _cabi.chain_fused_fwd_taps(ids, p, x32, y32, last, st32[:1]), 12)):
    a, b = ab(fa32, fn, args.rounds, args.reps)
    res['cases'].append(case(name, a, b, px, extra, 24))
    print(json.dumps(res['cases'][-1]), flush=True)
  # the CLI on 16 mixed-size PNGs
  from PIL import Image
  with tempfile.TemporaryDirectory() as tmp:
    paths = []
    for i, (hh, ww) in enumerate(MIXED):
      pth = os.path.join(tmp, 'im%02d.png' % i)
      Image.fromarray(rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8), 'RGB').save(pth)
      paths.append(pth)
    out = os.path.join(tmp, 'out') + os.sep
    cli_wall(paths[:2], ['--batch', '2'], out)  # warm-up (agent build, kernels, PIL)
    batch = cli_wall(paths, ['--batch', '16'], out)
    stepwise = cli_wall(paths, ['--stepwise'], out)
    res['cli'] = dict(images=len(paths), batch16_ms_per_image=batch, stepwise_ms_per_image=stepwise,
                      ratio=batch / stepwise)
    print(json.dumps(res['cli']), flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
