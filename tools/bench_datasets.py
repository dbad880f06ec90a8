"""Timing of the photo training sets: expo_area_resize_ragged, expo_pack_recut, build_pack per file,
and the training iteration over PackProviders against ResidentProviders.

Device (events around `--reps` calls after warm-up, median of `--rounds`):
  (a) INTER_AREA of 16 x 4000x6000 fp32 to 80x80: 4 `fivek` windows (side 4000) per image, and 1 centre (`folder`)
      window per image.  Algorithmic bytes: window pixels x 12 + the output; rate against the 12-byte copy rate of
      profiles/r06_final_membench.txt (c12bufx4, 5.78 TB/s).  Host: the float64 NumPy restatement of one window,
      times the windows of the case.
  (b) expo_pack_recut of 8 000 x 80^2 -> 64^2 fp32 (bytes: the crops read + written).
Host: build_pack wall time per 24 MP 16-bit TIFF (`fivek`) and per 24 MP 8-bit JPEG (`folder`), split into file decode
and the rest (upload, device decode, resize, synchronise).
Training: ms per iteration of GAN.train_iteration (graph path) over 8 000-row packs against 4 096-row ResidentProviders,
`--iters` iterations after warm-up (several epoch wraps of the real set at 384 rows per iteration).
usage: python tools/bench_datasets.py [--rounds 5] [--reps 10] [--iters 200] [--out profiles/datasets.json]"""
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

from exposure_amd import _cabi, datasets  # noqa: E402
from exposure_amd.tiff16 import write_tiff  # noqa: E402
from tests import _area_ref  # noqa: E402

COPY12_TBS = 5.7756  # c12bufx4, grid 2048, profiles/r06_final_membench.txt


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


def resize_cases(rounds, reps, dev):
  h, w, n, S = 4000, 6000, 16, 80
  g = torch.Generator(device=dev).manual_seed(0)
  xs = [torch.rand((h, w, 3), device=dev, generator=g) for _ in range(n)]
  rng = np.random.default_rng(0)
  fivek = [(i, 0, int(rng.integers(0, w - h + 1)), h) for i in range(n) for _ in range(4)]
  folder = [(i, 0, (w - h) // 2, h) for i in range(n)]
  host_one = None
  out = []
  for name, wins in (('fivek: 4 windows per image', fivek), ('folder: 1 centre window per image', folder)):
    o = torch.empty((len(wins), S, S, 3), device=dev)
    ms = device_ms(lambda: _cabi.area_resize_ragged(xs, wins, S, o), rounds, reps)
    nbytes = len(wins) * (h * h * 12 + S * S * 12)
    if host_one is None:
      win = xs[0][:, fivek[0][2]:fivek[0][2] + h].double().cpu().numpy()
      t0 = time.perf_counter()
      _area_ref.area_resize(win, S)
      host_one = time.perf_counter() - t0
    tbs = nbytes / (ms * 1e-3) / 1e12
    out.append(dict(case=name, windows=len(wins), side=h, S=S, ms=ms, algorithmic_bytes=nbytes, tb_per_s=tbs,
                    of_copy12=tbs / COPY12_TBS, host_numpy_ms=host_one * 1e3 * len(wins)))
  return out


def recut_case(rounds, reps, dev):
  m, S, C = 8000, 80, 64
  master = torch.rand((m, S, S, 3), device=dev)
  rng = np.random.default_rng(1)
  rec = torch.from_numpy(np.stack([rng.permutation(m), rng.integers(0, S - C + 1, m), rng.integers(0, S - C + 1, m),
                                   rng.random(m) < 0.5], 1).astype(np.int32)).to(dev)
  out = torch.empty((m, C, C, 3), device=dev)
  ms = device_ms(lambda: _cabi.pack_recut(master, rec, out), rounds, reps)
  nbytes = 2 * m * C * C * 12
  tbs = nbytes / (ms * 1e-3) / 1e12
  return dict(case='8000 x 80^2 -> 64^2 fp32', ms=ms, algorithmic_bytes=nbytes, tb_per_s=tbs, of_copy12=tbs / COPY12_TBS)


def build_cases(dev, files=2):
  from PIL import Image
  rng = np.random.default_rng(2)
  out = []
  with tempfile.TemporaryDirectory() as tmp:
    for recipe, ext in (('fivek', 'tif'), ('folder', 'jpg')):
      d = os.path.join(tmp, recipe)
      os.makedirs(d)
      for k in range(files):
        # smooth content (JPEG sizes of a photo, not of noise)
        y, x = np.mgrid[0:4000, 0:6000]
        base = (np.sin(x / (97.0 + k)) * np.cos(y / 61.0) + 1) / 2
        img = np.stack([base, base**1.5, 1 - base], axis=2)
        if recipe == 'fivek':
          write_tiff(os.path.join(d, 'f%02d.tif' % k), (img * 65535).astype(np.uint16))
        else:
          Image.fromarray((img * 255).astype(np.uint8)).save(os.path.join(d, 'f%02d.jpg' % k), quality=92)
      paths = datasets.list_files(d)
      datasets.build_pack(paths[:1], recipe, torch.float32, dev, seed=0)  # warm-up
      tm = {}
      t0 = time.perf_counter()
      datasets.build_pack(paths, recipe, torch.float32, dev, seed=0, timings=tm)
      wall = time.perf_counter() - t0
      out.append(dict(recipe=recipe, file='24 MP %s' % ('16-bit TIFF' if recipe == 'fivek' else '8-bit JPEG'),
                      files=files, ms_per_file=wall * 1e3 / files, read_ms_per_file=tm['read'] * 1e3 / files,
                      rest_ms_per_file=(wall - tm['read']) * 1e3 / files))
  return out


def training_cases(dev, iters):
  from exposure_amd.config import make_cfg
  from exposure_amd.gan import GAN
  from exposure_amd.replay_memory import ReplayMemory, ResidentProvider
  cfg = make_cfg()
  res = []
  for name in ('ResidentProvider', 'PackProvider'):
    torch.manual_seed(0)
    gan = GAN(cfg, device=dev, use_graphs=True, seed=0)
    if name == 'PackProvider':
      g = torch.Generator(device=dev).manual_seed(3)
      fd = datasets.PackProvider(torch.rand((8000, 80, 80, 3), device=dev, generator=g)**2.2 * 0.35, seed=1)
      rd = datasets.PackProvider(torch.rand((8000, 64, 64, 3), device=dev, generator=g)**1.2 * 0.9, seed=2)
    else:
      fd = ResidentProvider(dev, gamma=2.2, scale=0.35, seed=1)
      rd = ResidentProvider(dev, gamma=1.2, scale=0.9, seed=2)
    mem = ReplayMemory(cfg, fd, rd, seed=0)
    for _ in range(20):  # roll-out: terminated records for the critic
      feed, feats = mem.get_feed_dict_and_states(cfg.batch_size, lazy=True)
      out = gan.generator_step(feed['fake_input'], feed['z'], feed['states'], 0.0, it=0)
      mem.replace_memory(out['fake_output'], out['new_states'], feats, advanced=True)
    for it in range(1, 11):
      gan.train_iteration(mem, it)
    torch.cuda.synchronize()
    e0 = getattr(rd, 'epochs', 0)
    t0 = time.perf_counter()
    for it in range(11, 11 + iters):
      gan.train_iteration(mem, it)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    res.append(dict(provider=name, iterations=iters, ms_per_iteration=ms, real_epoch_wraps=getattr(rd, 'epochs', 0) - e0,
                    graph_captured=any(k[0] == 'it' and isinstance(v, tuple) for k, v in gan._graphs.items())))
  res[1]['vs_resident'] = res[1]['ms_per_iteration'] / res[0]['ms_per_iteration']
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'datasets.json'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  res = dict(device=torch.cuda.get_device_name(0), copy12_tb_per_s=COPY12_TBS)
  res['area_resize'] = resize_cases(args.rounds, args.reps, dev)
  torch.cuda.empty_cache()
  res['pack_recut'] = recut_case(args.rounds, args.reps, dev)
  torch.cuda.empty_cache()
  res['build'] = build_cases(dev)
  res['training'] = training_cases(dev, args.iters)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res, indent=1))


if __name__ == '__main__':
  main()
