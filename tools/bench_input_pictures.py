"""Timing of the input pictures from integer codes, by the method of tools/bench_decode.py: device
events around `--reps` calls after warm-up, median of `--rounds`; the C entry point is called through ctypes with the
argument arrays built once.

(a) expo_codes_lut_ragged, 16 x 4000x6000 and 16 x 512x512, RGB codes -> uint8 pictures: 8-bit codes, and 16-bit codes
    with the table read through the caches and staged in LDS (EXPO_CODES_LUT_LDS16 = 0 / 1).  Bytes: codes in + picture
    out; the rate is reported against the 12-byte copy rate of profiles/r06_final_membench.txt (5.78 TB/s).
(b) per 24 MP image (8-bit RGB codes, fp16 storage), wall time ending in a device synchronise: today's --show-input
    path (download of the float input + tone_mapped_input + save_png's encode) against evaluate.input_pictures_raw
    (tone-mapped picture only, codes already uploaded + download of the picture), each with and without the PNG write.
usage: python tools/bench_input_pictures.py [--rounds 5] [--reps 10] [--skip-host] [--out FILE.json]"""
import argparse
import ctypes
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

COPY12_TBS = 5.7756  # c12bufx4, grid 2048, profiles/r06_final_membench.txt


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / reps


def median_ms(fn, rounds, reps):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  return statistics.median(timed(fn, reps) for _ in range(rounds))


def lut_case(name, sizes, bits, lds16, rounds, reps, dev):
  lib = _cabi.load()
  ct = torch.uint8 if bits == 8 else torch.uint16
  torch.manual_seed(len(sizes) + bits)
  n = len(sizes)
  codes = [torch.randint(0, 1 << bits, (h, w, 3), dtype=torch.int32, device=dev).to(ct) for h, w in sizes]
  outs = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for h, w in sizes]
  luts = torch.randint(0, 256, (n, 1 << bits), dtype=torch.int32, device=dev).to(torch.uint8)
  cp, op = _cabi._ptr_array(codes), _cabi._ptr_array(outs)
  hs, ws = (ctypes.c_int * n)(*[h for h, _w in sizes]), (ctypes.c_int * n)(*[w for _h, w in sizes])
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  os.environ['EXPO_CODES_LUT_LDS16'] = '1' if lds16 else '0'

  def fn():
    rc = lib.expo_codes_lut_ragged(cp, hs, ws, n, 3, bits, ctypes.c_void_p(luts.data_ptr()), 1 << bits, 8, op, stream)
    assert rc == 0, lib.expo_last_error()

  ms = median_ms(fn, rounds, reps)
  px = sum(h * w for h, w in sizes)
  nbytes = px * 3 * (bits // 8) + px * 3
  tbs = nbytes / (ms * 1e-3) / 1e12
  return dict(case=name, images=n, pixels=px, code_bits=bits, table='lds' if (lds16 or bits == 8) else 'caches', ms=ms,
              bytes=nbytes, tb_per_s=tbs, of_copy12=tbs / COPY12_TBS)


def host_case(reps, dev, tmp):
  rng = np.random.default_rng(7)
  raws = [(rng.integers(0, 256, (4000, 6000, 3), dtype=np.uint8), 'srgb8')]
  hi = evaluate.decode_images(raws, torch.float16, dev)[0]
  staged = list(evaluate.stage_raws(raws, torch.float16, dev))
  png = os.path.join(tmp, 'p.png')

  def sync_time(fn):
    ts = []
    for _ in range(reps):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3

  def host_picture():
    a = evaluate.tone_mapped_input(hi[0].float().cpu().numpy())
    return np.clip(np.rint(np.asarray(a, dtype=np.float32) * 255.0), 0, 255).astype(np.uint8)

  def device_picture():
    return evaluate.input_pictures_raw(raws, torch.float16, dev, linear=False, staged=staged)[0][0].cpu().numpy()

  assert np.array_equal(host_picture(), device_picture())
  return dict(image='24MP srgb8 fp16', host_ms=sync_time(host_picture), device_ms=sync_time(device_picture),
              host_with_png_ms=sync_time(lambda: evaluate.save_png_u8(png, host_picture())),
              device_with_png_ms=sync_time(lambda: evaluate.save_png_u8(png, device_picture())))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--host-reps', type=int, default=3)
  ap.add_argument('--skip-host', action='store_true')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_input_pictures needs a ROCm GPU'
  dev = torch.device('cuda:0')
  res = dict(device=torch.cuda.get_device_name(0), lut=[], host=[])
  for name, sizes in (('16x24MP', [(4000, 6000)] * 16), ('16x512x512', [(512, 512)] * 16)):
    small = sizes[0][0] == 512
    for bits, lds16 in ((8, False), (16, False), (16, True)):
      r = lut_case(name, sizes, bits, lds16, args.rounds, args.reps * (20 if small else 1), dev)
      print(json.dumps(r), flush=True)
      res['lut'].append(r)
  os.environ.pop('EXPO_CODES_LUT_LDS16', None)
  if not args.skip_host:
    with tempfile.TemporaryDirectory() as tmp:
      r = host_case(args.host_reps, dev, tmp)
      print(json.dumps(r), flush=True)
      res['host'].append(r)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
