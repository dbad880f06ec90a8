"""Timing of expo_decode_ragged (the input images' decode on the device).

Device (events around `--reps` calls after warm-up, median of `--rounds`):
  (a) 16 x 4000x6000 8-bit RGB -> fp16, normalised (srgb8);  (b) the same with 16-bit codes (srgb16);
  (c) a mixed-size ragged set of 16 8-bit images -> fp16.
Algorithmic bytes: codes read twice plus the output written (normalised); the rate is reported against the 12-byte
copy rate of profiles/r06_final_membench.txt (c12bufx4, 5.78 TB/s).
Host, per image, on seeded 24 MP files (an 8-bit PNG and a 16-bit TIFF): PIL's / the TIFF reader's decode alone,
load_image + upload + cast, and load_raw + upload + decode_ragged, each ending in a device synchronise.
usage: python tools/bench_decode.py [--rounds 5] [--reps 10] [--host-reps 3] [--out profiles/decode_bench.json]"""
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

from exposure_amd import _cabi, evaluate  # noqa: E402
from exposure_amd.tiff16 import read_tiff, write_tiff  # noqa: E402

COPY12_TBS = 5.7756  # c12bufx4, grid 2048, profiles/r06_final_membench.txt
MIXED = [(512, 768), (768, 512)] * 6 + [(512, 768), (1024, 1280), (1200, 1600), (1536, 1024)]


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def device_case(name, sizes, kind, rounds, reps, dev):
  hi, ct = (256, torch.uint8) if kind == 'srgb8' else (65536, torch.uint16)
  torch.manual_seed(len(sizes))
  codes = [torch.randint(0, hi, (h, w, 3), dtype=torch.int32, device=dev).to(ct) for h, w in sizes]
  outs = [torch.empty((h, w, 3), dtype=torch.float16, device=dev) for h, w in sizes]
  table = evaluate.decode_table(kind, dev)
  norm = evaluate.DECODE_NORMALIZE[kind]
  fn = lambda: _cabi.decode_ragged(codes, table, norm, outs)
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  ms = statistics.median(timed(fn, reps) for _ in range(rounds))
  px = sum(h * w for h, w in sizes)
  nbytes = px * 3 * ct.itemsize * (2 if norm else 1) + px * 3 * 2
  tbs = nbytes / (ms * 1e-3) / 1e12
  return dict(case=name, images=len(sizes), pixels=px, kind=kind, dtype='f16', ms=ms, algorithmic_bytes=nbytes,
              tb_per_s=tbs, of_copy12=tbs / COPY12_TBS)


def host_case(path, reps, dev):
  def sync_time(fn):
    ts = []
    for _ in range(reps):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3

  tif = path.endswith('.tif')
  if tif:
    file_decode = lambda: read_tiff(path)
  else:
    from PIL import Image
    file_decode = lambda: np.asarray(Image.open(path).convert('RGB'))
  host = lambda: torch.from_numpy(np.ascontiguousarray(evaluate.load_image(path))).to(dev).to(torch.float16)[None]
  device = lambda: evaluate.decode_images([evaluate.load_raw(path)], torch.float16, dev)
  a, b = host(), device()[0]
  torch.cuda.synchronize()
  assert torch.equal(a.view(torch.int16), b.view(torch.int16)), path
  return dict(file=os.path.basename(path), file_decode_ms=sync_time(file_decode), load_image_upload_cast_ms=sync_time(host),
              load_raw_upload_decode_ms=sync_time(device))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--host-reps', type=int, default=3)
  ap.add_argument('--skip-host', action='store_true')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  res = dict(device=[], host=[])
  for name, sizes, kind in (('16x24MP_8bit', [(4000, 6000)] * 16, 'srgb8'),
                            ('16x24MP_16bit', [(4000, 6000)] * 16, 'srgb16'),
                            ('mixed16_8bit', MIXED, 'srgb8')):
    r = device_case(name, sizes, kind, args.rounds, args.reps, dev)
    print(json.dumps(r), flush=True)
    res['device'].append(r)
  if not args.skip_host:
    from PIL import Image
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
      png, tif = os.path.join(tmp, 'a.png'), os.path.join(tmp, 'a.tif')
      Image.fromarray(rng.integers(0, 256, (4000, 6000, 3), dtype=np.uint8), 'RGB').save(png, compress_level=1)
      write_tiff(tif, rng.integers(0, 65536, (4000, 6000, 3), dtype=np.uint16))
      for p in (png, tif):
        r = host_case(p, args.host_reps, dev)
        print(json.dumps(r), flush=True)
        res['host'].append(r)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
