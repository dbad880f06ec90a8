"""Timing and peak memory of retouching straight from integer codes against the path it replaces,
both in this process, alternating round by round, warmed, timed with device events around `--reps` calls.

  parent  decode_ragged + bilinear_resize_ragged + chain_fused_fwd_ragged_taps      (the float input is written and read)
  codes   decode_tables + bilinear_resize_ragged_codes + chain_fused_fwd_ragged_codes
Each with the float outputs and with ys = None (pictures only).  The sequence is 8 steps, all eight filters, with a tap
of the last step: uint8 for srgb8 codes, uint16 for prophoto16.  Shapes: 16 x 512x512 and `--big` x 4000x6000.  Codes:
uniformly random (what profiles/decode.md used), and a smooth seeded gradient with noise (neighbouring pixels of a
photo hold neighbouring codes).  Every buffer is allocated before the clock starts; the peak memory of a path is
torch.cuda.max_memory_allocated over one call that allocates what the path needs (the codes excluded: both hold them).
The two paths' outputs and taps are compared bit for bit before anything is timed.
usage: python tools/bench_fused_decode.py [--rounds 5] [--reps 5] [--big 16] [--out profiles/fused_decode_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import _cabi, evaluate, synthetic  # noqa: E402

STEPS = 8
S = 64


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def make_codes(sizes, kind, how, dev, seed):
  hi, ct = (256, torch.uint8) if kind == 'srgb8' else (65536, torch.uint16)
  g = torch.Generator(device=dev).manual_seed(seed)
  out = []
  for h, w in sizes:
    if how == 'random':
      c = torch.randint(0, hi, (h, w, 3), dtype=torch.int32, device=dev, generator=g)
    else:  # a diagonal ramp per channel plus noise of 1 % of the range
      yy = torch.linspace(0.05, 0.6, h, device=dev)[:, None, None]
      xx = torch.linspace(0.0, 0.35, w, device=dev)[None, :, None]
      ch = torch.tensor([0.0, 0.03, -0.02], device=dev)[None, None, :]
      v = yy + xx + ch + 0.01 * torch.randn((h, w, 3), device=dev, generator=g)
      c = (v.clamp_(0, 1) * (hi - 1)).round_().to(torch.int32)
    out.append(c.to(ct))
    del c
  return out


def sequence(n, dev):
  """ids 0..7 in order for every image, parameters seeded per image"""
  rng = np.random.default_rng(8)
  ids = np.tile(np.arange(STEPS, dtype=np.int32), (n, 1))
  p = np.zeros((n, STEPS, 24), dtype=np.float32)
  for i in range(n):
    for st in range(STEPS):
      p[i, st, :_cabi.NUM_PARAMS[st]] = synthetic.make_params(rng, st, 1)[0]
  return torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev)


def case(name, sizes, kind, dtype, how, rounds, reps, dev):
  n = len(sizes)
  codes = make_codes(sizes, kind, how, dev, 100 + n)
  table, norm = evaluate.decode_table(kind, dev), evaluate.DECODE_NORMALIZE[kind]
  tap_dt = torch.uint8 if kind == 'srgb8' else torch.uint16
  ids, prm = sequence(n, dev)
  mask = 1 << (STEPS - 1)
  windows = evaluate.center_windows(sizes)

  def buffers(float_in, outputs):
    b = dict(low=torch.empty((n, S, S, 3), dtype=dtype, device=dev),
             taps=[torch.empty((1, h, w, 3), dtype=tap_dt, device=dev) for h, w in sizes])
    b['xs'] = [torch.empty((1, h, w, 3), dtype=dtype, device=dev) for h, w in sizes] if float_in else None
    b['ys'] = [torch.empty((1, h, w, 3), dtype=dtype, device=dev) for h, w in sizes] if outputs else None
    return b

  def parent(b):
    _cabi.decode_ragged(codes, table, norm, b['xs'])
    _cabi.bilinear_resize_ragged(b['xs'], windows, S, b['low'])
    _cabi.chain_fused_fwd_ragged_taps(ids, prm, b['xs'], b['ys'], mask, b['taps'])

  def fused(b):
    tables, stride = _cabi.decode_tables(codes, table, norm, dtype)
    _cabi.bilinear_resize_ragged_codes(codes, tables, stride, windows, S, b['low'])
    _cabi.chain_fused_fwd_ragged_codes(ids, prm, codes, tables, stride, b['ys'], mask, b['taps'])

  paths = {'parent': (parent, True, True), 'parent_pictures_only': (parent, True, False),
           'codes': (fused, False, True), 'codes_pictures_only': (fused, False, False)}
  for key in ('parent', 'codes'):  # the shared workspace grows to its size here, outside the measurements
    b = buffers(paths[key][1], True)
    paths[key][0](b)
    del b
  # peak memory of one call that allocates what it needs, over the resident codes
  peak = {}
  for key, (fn, float_in, outputs) in paths.items():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    b = buffers(float_in, outputs)
    fn(b)
    torch.cuda.synchronize()
    peak[key] = torch.cuda.max_memory_allocated() - base
    if key == 'parent':
      ref = b
    elif key == 'codes':  # the same bits before anything is timed
      for a, c in zip(ref['ys'] + ref['taps'] + [ref['low']], b['ys'] + b['taps'] + [b['low']]):
        assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)), name
      del ref
    del b
  bufs = {key: buffers(float_in, outputs) for key, (_fn, float_in, outputs) in paths.items()}
  for key, (fn, _i, _o) in paths.items():
    for _ in range(2):
      fn(bufs[key])
  torch.cuda.synchronize()
  ms = {key: [] for key in paths}
  for _ in range(rounds):  # alternating
    for key, (fn, _i, _o) in paths.items():
      ms[key].append(timed(lambda: fn(bufs[key]), reps))
  row = dict(case=name, images=n, pixels=sum(h * w for h, w in sizes), kind=kind, codes=how,
             dtype='f16' if dtype is torch.float16 else 'f32', tap=str(tap_dt).split('.')[-1])
  for key in paths:
    row[key + '_ms'] = statistics.median(ms[key])
    row[key + '_ms_min_max'] = [min(ms[key]), max(ms[key])]
    row[key + '_peak_bytes'] = peak[key]
  row['codes_over_parent'] = row['codes_ms'] / row['parent_ms']
  row['pictures_only_codes_over_parent'] = row['codes_pictures_only_ms'] / row['parent_pictures_only_ms']
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--big', type=int, default=16, help='number of 4000x6000 images of the large case')
  ap.add_argument('--only', default=None, help='run the cases whose name contains this')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  rows = []
  for name, sizes in (('16x512x512', [(512, 512)] * 16), ('%dx24MP' % args.big, [(4000, 6000)] * args.big)):
    for kind in ('srgb8', 'prophoto16'):
      for dtype in (torch.float16, torch.float32):
        for how in ('random', 'gradient'):
          if args.only and args.only not in name:
            continue
          r = case(name, sizes, kind, dtype, how, args.rounds, args.reps, dev)
          print(json.dumps(r), flush=True)
          rows.append(r)
          torch.cuda.empty_cache()
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(rows, f, indent=1)


if __name__ == '__main__':
  main()
