"""Timing and file sizes of the device JPEG encoder, by the method of tools/bench_png_encode.py.

Inputs: EXPO_TAP_U8 pictures (evaluate.retouch_batch(..., picture=True)) of exposure_amd.synthetic images retouched by a
seeded, randomly initialised agent: 16 x 512x512, 1 x 4000x6000, 16 x 4000x6000.  synthetic's images are independent
noise per pixel, the worst case of a transform coder; `--smooth` adds the same shapes made from synthetic images of 1/8
the size, enlarged bilinearly, as a stand-in for a photograph's local smoothness (reported apart, never mixed in).
Both kinds are synthetic pictures, not photographs.  Per shape and sampling (420, 444) at --quality:
  device ms per expo_jpeg_encode_ragged call from events (warm-up, --reps calls, median / min / max of --rounds), as a
    multiple of a 1-byte-per-channel read-and-write copy of the pictures (torch's device copy of the same bytes, timed
    the same way); the same with the download to host bytes (evaluate.encode_jpeg_batch), host clock around it;
  the same pictures through evaluate.encode_png_batch (adaptive filter) in the same process, to host bytes;
  PIL's save(..., 'JPEG', quality, subsampling) of the downloaded picture into a BytesIO, alternating with the device
    path in the same process, host clock;
  bytes: device files against raw and against PIL's.
usage: python tools/bench_jpeg_encode.py [--rounds 7] [--reps 50] [--host-reps 1] [--shapes small,one,many] [--smooth]
       [--quality 90] [--out FILE.json] [--md FILE.md]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import _cabi, evaluate  # noqa: E402
from exposure_amd.agent import Agent  # noqa: E402
from exposure_amd.config import make_cfg  # noqa: E402
from tools.bench_png_encode import SHAPES, pictures, rounds_ms  # noqa: E402


def pil_bytes(pic_host, quality, sub):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(pic_host, 'RGB').save(buf, format='JPEG', quality=quality, subsampling={'444': 0, '420': 2}[sub])
  return buf.getbuffer().nbytes


def case(name, pics, sub, args):
  raw = sum(p.numel() for p in pics)
  caps = [_cabi.jpeg_encode_bound(p.shape[0], p.shape[1], sub) if args.bound else 629 + p.numel() for p in pics]
  outs, sizes = _cabi.jpeg_encode_ragged(pics, args.quality, sub, capacity=caps)
  sizes = sizes.cpu().tolist()
  dev_bytes = sum(sizes)
  written = all(n <= o.numel() for n, o in zip(sizes, outs))
  enc = rounds_ms(lambda: _cabi.jpeg_encode_ragged(pics, args.quality, sub, outs=outs), args.rounds, args.reps)
  copies = [torch.empty_like(p) for p in pics]

  def copy():
    for a, b in zip(copies, pics):
      a.copy_(b)

  cp = rounds_ms(copy, args.rounds, args.reps)
  del copies, outs
  dl, png, pil, pil_total, png_total = [], [], [], 0, 0
  for _ in range(args.host_reps):  # alternating: device JPEG, device PNG, PIL's JPEG
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    files = evaluate.encode_jpeg_batch(pics, args.quality, sub)
    torch.cuda.synchronize()
    dl.append((time.perf_counter() - t0) * 1e3)
    assert sum(len(f) for f in files) == dev_bytes
    del files
    t0 = time.perf_counter()
    files = evaluate.encode_png_batch(pics, 'adaptive')
    torch.cuda.synchronize()
    png.append((time.perf_counter() - t0) * 1e3)
    png_total = sum(len(f) for f in files)
    del files
    t0 = time.perf_counter()
    pil_total = sum(pil_bytes(p.cpu().numpy(), args.quality, sub) for p in pics)
    pil.append((time.perf_counter() - t0) * 1e3)
  row = dict(case=name, subsampling=sub, quality=args.quality, images=len(pics), raw_bytes=raw, device_ms=enc, copy_ms=cp,
             of_copy=enc['median'] / cp['median'], all_written_in_first_call=written,
             device_with_download_ms=statistics.median(dl), png_with_download_ms=statistics.median(png),
             pil_ms=statistics.median(pil), speedup_vs_pil=statistics.median(pil) / statistics.median(dl),
             speedup_vs_png=statistics.median(png) / statistics.median(dl), device_bytes=dev_bytes, png_bytes=png_total,
             pil_bytes=pil_total, of_raw=dev_bytes / raw, size_vs_pil=dev_bytes / pil_total)
  print(json.dumps(row), flush=True)
  return row


def markdown(rows):
  out = ['| pictures | sampling | device ms (min - max) | x copy | to host bytes ms | device PNG to host bytes ms | PIL JPEG ms | '
         'vs PIL | vs device PNG | bytes / raw | bytes / PIL |', '|---|---|---|---|---|---|---|---|---|---|---|']
  for r in rows:
    d = r['device_ms']
    out.append('| %s | %s | %.3f (%.3f - %.3f) | %.1f | %.1f | %.1f | %.1f | %.1fx | %.1fx | %.3f | %.3f |' %
               (r['case'], r['subsampling'], d['median'], d['min'], d['max'], r['of_copy'], r['device_with_download_ms'],
                r['png_with_download_ms'], r['pil_ms'], r['speedup_vs_pil'], r['speedup_vs_png'], r['of_raw'],
                r['size_vs_pil']))
  return '\n'.join(out) + '\n'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--host-reps', type=int, default=1)
  ap.add_argument('--shapes', default='small,one,many')
  ap.add_argument('--smooth', action='store_true')
  ap.add_argument('--quality', type=int, default=90)
  ap.add_argument('--bound', action='store_true', help='time with buffers of expo_jpeg_encode_bound instead of 629 + 3 h w')
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
      for sub in ('420', '444'):
        rows.append(case('%d x %dx%d%s' % (n, h, w, ' smooth' if smooth else ''), pics, sub, args))
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
