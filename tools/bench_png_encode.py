"""Timing and file sizes of the device PNG encoder, by the method of tools/bench_input_pictures.py.

Inputs: EXPO_TAP_U8 pictures (evaluate.retouch_batch(..., picture=True)) of exposure_amd.synthetic images retouched by a
seeded, randomly initialised agent: 16 x 512x512, 1 x 4000x6000, 16 x 4000x6000.  synthetic's images are independent
noise per pixel, which no PNG coder compresses much; `--smooth` adds the same shapes made from synthetic images of 1/8
the size, enlarged bilinearly, as a stand-in for a photograph's local smoothness (reported apart, never mixed in).
Per shape and filter (adaptive, paeth):
  device ms per expo_png_encode_ragged call from events (warm-up, --reps calls, median / min / max of --rounds), as a
    multiple of a 1-byte-per-channel read-and-write copy of the pictures (torch's device copy of the same bytes, timed
    the same way); the same with the download to host bytes (evaluate.encode_png_batch), host clock around it;
  the parent's path in the same process, alternating with the device path: pic.cpu().numpy() + save_png_u8 into a
    BytesIO at PIL's default level and at compress_level=1, host clock;
  bytes: device files against PIL level 6 and level 1.
usage: python tools/bench_png_encode.py [--rounds 7] [--reps 50] [--host-reps 1] [--shapes small,one,many] [--smooth]
       [--out FILE.json] [--md FILE.md]"""
import argparse
import io
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
from exposure_amd.agent import Agent  # noqa: E402
from exposure_amd.config import make_cfg  # noqa: E402

SHAPES = {'small': (16, 512, 512), 'one': (1, 4000, 6000), 'many': (16, 4000, 6000)}


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def rounds_ms(fn, rounds, reps):
  for _ in range(2):
    fn()
  torch.cuda.synchronize()
  t = [timed(fn, reps) for _ in range(rounds)]
  return dict(median=statistics.median(t), min=min(t), max=max(t))


def pictures(agent, n, h, w, smooth, dev):
  rng = np.random.default_rng(n * 1000003 + h)
  pics = []
  for _ in range(n):  # one image at a time: the float inputs of 16 x 24 MP need not be resident together
    if smooth:
      lo = torch.from_numpy(synthetic.make_images(rng, (1, h // 8, w // 8, 3), np.float32)).to(dev).permute(0, 3, 1, 2)
      x = torch.nn.functional.interpolate(lo, size=(h, w), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
      x = x.contiguous().half()
    else:
      x = torch.from_numpy(synthetic.make_images(rng, (1, h, w, 3), np.float16)).to(dev)
    torch.manual_seed(11)
    pics.append(evaluate.retouch_batch(agent, [x], picture=True)[-1][0].contiguous())
  return pics


def pil_bytes(pic_host, level):
  from PIL import Image
  buf = io.BytesIO()
  kw = {} if level is None else dict(compress_level=level)
  Image.fromarray(pic_host, 'RGB').save(buf, format='PNG', **kw)
  return buf.getbuffer().nbytes


def case(name, pics, filt, args):
  raw = sum(p.numel() for p in pics)
  outs, sizes = _cabi.png_encode_ragged(pics, filt)
  dev_bytes = int(sizes.sum().item())
  enc = rounds_ms(lambda: _cabi.png_encode_ragged(pics, filt, outs=outs), args.rounds, args.reps)
  copies = [torch.empty_like(p) for p in pics]

  def copy():
    for a, b in zip(copies, pics):
      a.copy_(b)

  cp = rounds_ms(copy, args.rounds, args.reps)
  dl, host6, host1, b6, b1 = [], [], [], 0, 0
  for _ in range(args.host_reps):  # alternating: device path, level 6, level 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    files = evaluate.encode_png_batch(pics, filt)
    torch.cuda.synchronize()
    dl.append((time.perf_counter() - t0) * 1e3)
    assert sum(len(f) for f in files) == dev_bytes
    for level, acc in ((None, host6), (1, host1)):
      t0 = time.perf_counter()
      total = sum(pil_bytes(p.cpu().numpy(), level) for p in pics)
      acc.append((time.perf_counter() - t0) * 1e3)
      if level is None:
        b6 = total
      else:
        b1 = total
  row = dict(case=name, filter=filt, images=len(pics), raw_bytes=raw, device_ms=enc, copy_ms=cp,
             of_copy=enc['median'] / cp['median'], device_with_download_ms=statistics.median(dl),
             pil6_ms=statistics.median(host6), pil1_ms=statistics.median(host1),
             speedup_vs_pil6=statistics.median(host6) / statistics.median(dl),
             speedup_vs_pil1=statistics.median(host1) / statistics.median(dl), device_bytes=dev_bytes, pil6_bytes=b6,
             pil1_bytes=b1, of_raw=dev_bytes / raw, size_vs_pil6=dev_bytes / b6, size_vs_pil1=dev_bytes / b1)
  print(json.dumps(row), flush=True)
  return row


def markdown(rows):
  out = ['| pictures | filter | device ms (min - max) | x copy | with download ms | PIL 6 ms | PIL 1 ms | vs PIL 6 | vs PIL 1 | '
         'bytes / raw | bytes / PIL 6 | bytes / PIL 1 |', '|---|---|---|---|---|---|---|---|---|---|---|---|']
  for r in rows:
    d = r['device_ms']
    out.append('| %s | %s | %.3f (%.3f - %.3f) | %.1f | %.1f | %.1f | %.1f | %.1fx | %.1fx | %.3f | %.2f | %.2f |' %
               (r['case'], r['filter'], d['median'], d['min'], d['max'], r['of_copy'], r['device_with_download_ms'],
                r['pil6_ms'], r['pil1_ms'], r['speedup_vs_pil6'], r['speedup_vs_pil1'], r['of_raw'], r['size_vs_pil6'],
                r['size_vs_pil1']))
  return '\n'.join(out) + '\n'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--host-reps', type=int, default=1)
  ap.add_argument('--shapes', default='small,one,many')
  ap.add_argument('--smooth', action='store_true')
  ap.add_argument('--out', default=None)
  ap.add_argument('--md', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  torch.manual_seed(7)
  agent = Agent(make_cfg()).to(dev)
  rows = []
  for key in args.shapes.split(','):
    n, h, w = SHAPES[key]
    for smooth in ((False, True) if args.smooth else (False,)):
      pics = pictures(agent, n, h, w, smooth, dev)
      for filt in ('adaptive', 'paeth'):
        rows.append(case('%d x %dx%d%s' % (n, h, w, ' smooth' if smooth else ''), pics, filt, args))
      del pics
      torch.cuda.empty_cache()
  if args.out:
    with open(args.out, 'w') as fh:
      json.dump(rows, fh, indent=1)
  if args.md:
    with open(args.md, 'w') as fh:
      fh.write(markdown(rows))


if __name__ == '__main__':
  main()
