"""Timing of the evaluation metric for `--images` synthetic 8-bit pictures of 4000x6000.

Host: `metrics.read_images` + `metrics.get_statistics` over `--host-files` PNG files written to a temporary directory
(wall clock; reported per file and scaled to `--images`, the work being the same for every file), split into reading
the files (PIL decode + the float32 conversion) and the rest (crops, pooling, statistics).
Device: `metrics.set_statistics` from resident codes (host clock around calls that end in a synchronise, median of
`--rounds`), and its three stages on their own (events around `--reps` calls after warm-up, median of `--rounds`):
  decode_ragged       one chunk of the set (the images of 4 GiB of float32): bytes = codes read + floats written
  area_resize_ragged  the chunk's 4 windows per image to 80x80: bytes = window pixels x 12 + the output
  patch_stats         the whole set's 16 F records on its (4 F, 80, 80, 3) master: bytes = 16 F x 64 x 64 x 12
and `stat_hist` of the (16 F, 3) statistics.  Rates are against the 12-byte copy rate of
profiles/r06_final_membench.txt (c12bufx4, 5.78 TB/s).
usage: python tools/bench_metric.py [--images 64] [--host-files 2] [--rounds 5] [--reps 10] [--out profiles/metric.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import _cabi, datasets, metrics  # noqa: E402

COPY12_TBS = 5.7756  # c12bufx4, grid 2048, profiles/r06_final_membench.txt
H, W = 4000, 6000


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def device_ms(fn, rounds, reps):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  return statistics.median(timed(fn, reps) for _ in range(rounds))


def rate(nbytes, ms):
  tbs = nbytes / (ms * 1e-3) / 1e12
  return dict(ms=ms, algorithmic_bytes=nbytes, tb_per_s=tbs, of_copy12=tbs / COPY12_TBS)


def host_case(files, images):
  from PIL import Image
  rng = np.random.default_rng(0)
  with tempfile.TemporaryDirectory() as tmp:
    for k in range(files):
      # smooth content plus noise (the file size of a photo, not of noise alone)
      y, x = np.mgrid[0:H, 0:W]
      base = (np.sin(x / (97.0 + k)) * np.cos(y / 61.0) + 1) / 2
      img = np.stack([base, base**1.5, 1 - base], axis=2) * 235 + rng.integers(0, 20, (H, W, 3))
      Image.fromarray(img.astype(np.uint8), 'RGB').save(os.path.join(tmp, 'f%02d.png' % k), compress_level=1)
      print('host: wrote file %d of %d' % (k + 1, files), flush=True)
    t0 = time.perf_counter()
    for f in sorted(os.listdir(tmp)):
      np.asarray(Image.open(os.path.join(tmp, f)).convert('RGB'), dtype=np.float32) / 255.0
    read = time.perf_counter() - t0
    t0 = time.perf_counter()
    patches = metrics.read_images(tmp, rng=random.Random(0))
    stats = metrics.get_statistics(patches)
    wall = time.perf_counter() - t0
  assert stats.shape == (16 * files, 3)
  per = wall * 1e3 / files
  return dict(files=files, ms_per_file=per, read_ms_per_file=read * 1e3 / files,
              rest_ms_per_file=(wall - read) * 1e3 / files, ms_scaled_to_set=per * images, images=images)


def device_cases(images, rounds, reps, dev):
  g = torch.Generator(device=dev).manual_seed(0)
  codes = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(images)]
  res = {}
  # the whole call, from resident codes
  def whole():
    st = metrics.set_statistics(codes, random.Random(0))
    torch.cuda.synchronize()
    return st
  whole()
  ts = []
  for _ in range(rounds):
    t0 = time.perf_counter()
    stats = whole()
    ts.append((time.perf_counter() - t0) * 1e3)
  res['set_statistics'] = dict(images=images, ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts),
                               ms_per_image=statistics.median(ts) / images)
  print('device: set_statistics %s' % res['set_statistics'], flush=True)
  # the stages
  lo, hi = datasets.plan_chunks([H * W * 12] * images)[0]
  n = hi - lo
  table = metrics._code_table(dev)
  lin = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in range(n)]
  ms = device_ms(lambda: _cabi.decode_ragged(codes[lo:hi], table, 0, lin), rounds, reps)
  res['decode_ragged'] = dict(images=n, **rate(n * H * W * 3 * (1 + 4), ms))
  windows, records = metrics.patch_windows([(H, W)] * images, random.Random(0))
  wins = np.array(windows[:4 * n], dtype=np.int32)
  master = torch.empty((4 * n, 80, 80, 3), dtype=torch.float32, device=dev)
  ms = device_ms(lambda: _cabi.area_resize_ragged(lin, wins, 80, master), rounds, reps)
  res['area_resize_ragged'] = dict(windows=4 * n, side=H, **rate(4 * n * (H * H * 12 + 80 * 80 * 12), ms))
  del lin
  full = torch.rand((4 * images, 80, 80, 3), device=dev, generator=g)
  rec = torch.from_numpy(np.array(records, dtype=np.int32)).to(dev)
  out = torch.empty((len(records), 3), dtype=torch.float32, device=dev)
  ms = device_ms(lambda: _cabi.patch_stats(full, rec, 64, out), rounds, reps)
  res['patch_stats'] = dict(records=len(records), **rate(len(records) * 64 * 64 * 12, ms))
  counts = torch.empty((3, 32), dtype=torch.int32, device=dev)
  ms = device_ms(lambda: _cabi.stat_hist(stats, 32, counts), rounds, reps)
  res['stat_hist'] = dict(values=3 * stats.shape[0], ms=ms)
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--images', type=int, default=64)
  ap.add_argument('--host-files', type=int, default=2)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metric.json'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  res = dict(device=torch.cuda.get_device_name(0), copy12_tb_per_s=COPY12_TBS, picture='%dx%d' % (H, W))
  res.update(device_cases(args.images, args.rounds, args.reps, dev))
  torch.cuda.empty_cache()
  res['host'] = host_case(args.host_files, args.images)
  res['host_over_device'] = res['host']['ms_scaled_to_set'] / res['set_statistics']['ms']
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res, indent=1))


if __name__ == '__main__':
  main()
