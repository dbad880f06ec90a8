"""Timing of the device JPEG decoder, by the method of tools/bench_jpeg_encode.py.

Pictures: synthetic uint8 pictures made on the host, independent noise per pixel (the worst case of a transform coder)
and "smooth" (noise of 1/8 the size enlarged bilinearly, a stand-in for a photograph's local smoothness); neither is a
photograph, and the tree holds none: "smooth" is the most photograph-like picture there is and stands in for them.  16 x 512x512 (sixteen pictures), 1 x 4000x6000 and 16 x 4000x6000 (one picture's file sixteen times).  Each
picture at --quality in 4:2:0 and 4:4:4, as two files:
  own   this project's device encoder (expo_jpeg_encode_ragged): restart intervals of 8 / 16 MCUs, a lane per interval
  pil   PIL's save(..., 'JPEG'): no restart markers.  These rows go through expo_jpeg_decode_sync_ragged (§3.36: a lane
        per subsequence of jpeg_decode.SUB_BYTES bytes, jpeg_decode.GRID_ROUNDS further settle launches) and carry the
        info words (how many pictures went which way), the one-lane walk of expo_jpeg_decode_ragged on the same files
        (what --jpeg-serial-entropy runs; measured once when it takes more than --slow-ms), and the sweep of sub_bytes
        over 64, 128, 256 and 512
Per case:
  device ms per expo_jpeg_decode_ragged call from events (warm-up, --reps calls, median / min / max of --rounds; a call
    of more than --slow-ms is measured once, and the row says so), as a multiple of a device copy of the output bytes;
    the kernels' shares (settle, scan, emit, serial or entropy, idct, rgb) from torch.profiler, one profiled call
    (where the profiler is available);
  file bytes -> device codes: jpeg_decode.decode_jpeg_batch (parse, one upload, the call), host clock around a
    synchronise;
  PIL: Image.open + convert('RGB') + upload of the same files, alternating in the same process, host clock.
--pack N: datasets.build_pack of N small JPEGs (the folder recipe) both ways, with its timings.
usage: python tools/bench_jpeg_decode.py [--rounds 7] [--reps 50] [--host-reps 3] [--shapes small,one,many]
       [--quality 90] [--slow-ms 1000] [--pack 256] [--out FILE.json] [--md FILE.md]"""
import argparse
import io
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

from exposure_amd import _cabi, datasets, jpeg_decode  # noqa: E402
from tools.bench_png_encode import SHAPES, rounds_ms, timed  # noqa: E402

SUBS = {'420': 2, '444': 0}


def picture(rng, h, w, smooth):
  from PIL import Image
  if not smooth:
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
  lo = Image.fromarray(rng.integers(0, 256, (h // 8, w // 8, 3), dtype=np.uint8), 'RGB')
  return np.asarray(lo.resize((w, h), Image.BILINEAR))


def pil_file(pic, quality, sub):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(pic, 'RGB').save(buf, format='JPEG', quality=quality, subsampling=SUBS[sub])
  return buf.getvalue()


def own_file(pic, quality, sub, dev):
  t = torch.from_numpy(np.ascontiguousarray(pic)).to(dev)
  cap = _cabi.jpeg_encode_bound(pic.shape[0], pic.shape[1], sub)
  outs, sizes = _cabi.jpeg_encode_ragged([t], quality, sub, capacity=[cap])
  return outs[0][:int(sizes[0])].cpu().numpy().tobytes()


def pil_decode_upload(datas, dev):
  from PIL import Image
  return [torch.from_numpy(np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))).to(dev) for d in datas]


def kernel_shares(fn):
  """{kernel: ms} of one profiled call, or None where the profiler gives nothing"""
  try:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
      fn()
      torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
      for k in ('sync_settle', 'sync_scan', 'sync_emit', 'sync_serial', 'entropy', 'idct', 'rgb'):
        if 'jpeg_%s_kernel' % k in e.key:
          out[k] = out.get(k, 0.0) + getattr(e, 'device_time_total', getattr(e, 'cuda_time_total', 0.0)) / 1e3
    return out or None
  except Exception:  # the profiler is optional: the totals stand without it
    return None


def case(name, kind, sub, datas, args, dev):
  """one row; a 'pil' row is the §3.36 entry with the one-lane path, the info words and the sweep beside it"""
  plans = [jpeg_decode.parse(d) for d in datas]
  files = [torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev) for d in datas]
  blobs = [torch.from_numpy(p.blob).to(dev) for p in plans]
  outs = [torch.empty((p.h, p.w, 3), dtype=torch.uint8, device=dev) for p in plans]
  status = torch.empty((len(datas),), dtype=torch.int32, device=dev)
  geo = ([p.h for p in plans], [p.w for p in plans], [p.sampling for p in plans], [p.ncomp for p in plans], [p.nsegs for p in plans])
  serial_call = lambda: _cabi.jpeg_decode_ragged(files, blobs, *geo, outs, status)
  info = torch.zeros((len(datas),), dtype=torch.int32, device=dev)
  sync_call = lambda b: _cabi.jpeg_decode_sync_ragged(files, blobs, *geo, [p.nsubs(b) for p in plans], b, jpeg_decode.GRID_ROUNDS,
                                                      outs, status, info)
  sync = kind == 'pil'
  call = (lambda: sync_call(jpeg_decode.SUB_BYTES)) if sync else serial_call
  _cabi.reserve_workspace(dev, max(jpeg_decode.workspace_bytes(plans), jpeg_decode.workspace_bytes(plans, 64)))  # (the first call allocates nothing)
  torch.cuda.synchronize()
  first = timed(call, 1)
  assert status.cpu().tolist() == [0] * len(datas)
  words = info.cpu().tolist()
  extra = {}
  if sync:
    keep = [o.clone() for o in outs]
    once = timed(serial_call, 1)  # the parent's one-lane path on the same files, in the same process
    print('  %s %s parallel %.1f ms, one lane %.1f ms' % (name, sub, first, once), file=sys.stderr, flush=True)
    assert all(torch.equal(a, b) for a, b in zip(keep, outs))
    reps = max(1, min(args.reps, int(args.slow_ms / max(once, 1e-3))))
    extra['serial_ms'] = dict(median=once, min=once, max=once) if once > args.slow_ms else rounds_ms(serial_call, args.rounds, reps)
    extra['serial_measured'] = 'once' if once > args.slow_ms else '%d x %d' % (args.rounds, reps)
    extra['info'] = {str(v): words.count(v) for v in (0, 1, 2)}
    sweep = {}
    for b in (64, 128, 256, 512):
      t = timed(lambda: sync_call(b), 1)
      print('  %s %s sub_bytes %d: %.1f ms' % (name, sub, b, t), file=sys.stderr, flush=True)  # (a slow row stays audible)
      got = info.cpu().tolist()
      assert all(torch.equal(a, c) for a, c in zip(keep, outs))
      reps = max(1, min(args.reps, int(args.slow_ms / max(t, 1e-3))))
      ms = dict(median=t, min=t, max=t) if t > args.slow_ms else rounds_ms(lambda: sync_call(b), args.rounds, reps)
      sweep[str(b)] = dict(ms=ms['median'], info={str(v): got.count(v) for v in (0, 1, 2)})
    extra['sweep'] = sweep
    del keep
  if first > args.slow_ms:  # seconds per call: this one call is the measurement
    dec, measured = dict(median=first, min=first, max=first), 'once'
  else:
    reps = max(1, min(args.reps, int(args.slow_ms / max(first, 1e-3))))
    dec, measured = rounds_ms(call, args.rounds, reps), '%d x %d' % (args.rounds, reps)
  shares = kernel_shares(call) if first <= args.slow_ms else None
  copies = [torch.empty_like(o) for o in outs]

  def copy():
    for a, b in zip(copies, outs):
      a.copy_(b)

  cp = rounds_ms(copy, args.rounds, args.reps)
  del copies
  host_reps = 1 if first > args.slow_ms else args.host_reps
  e2e, pil = [], []
  for _ in range(host_reps):  # alternating: the device path from file bytes, PIL's decode and upload
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, _ = jpeg_decode.decode_jpeg_batch(datas, dev)
    torch.cuda.synchronize()
    e2e.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    ref = pil_decode_upload(datas, dev)
    torch.cuda.synchronize()
    pil.append((time.perf_counter() - t0) * 1e3)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))  # bit for bit, as everywhere
    del got, ref
  row = dict(case=name, files=kind, subsampling=sub, images=len(datas), file_bytes=sum(len(d) for d in datas),
             out_bytes=sum(o.numel() for o in outs), segments=sum(p.nsegs for p in plans), device_ms=dec, measured=measured,
             kernels_ms=shares, copy_ms=cp, of_copy=dec['median'] / cp['median'], from_file_bytes_ms=statistics.median(e2e),
             pil_ms=statistics.median(pil), speedup_vs_pil=statistics.median(pil) / statistics.median(e2e), **extra)
  print(json.dumps(row), flush=True)
  return row


def pack_case(n, args, dev):
  rng = np.random.default_rng(99)
  with tempfile.TemporaryDirectory() as d:
    paths = []
    for i in range(n):
      paths.append(os.path.join(d, '%04d.jpg' % i))
      with open(paths[-1], 'wb') as f:
        f.write(pil_file(picture(rng, 96 + 8 * (i % 5), 128 + 8 * (i % 7), True), args.quality, '420'))
    out = {}
    for label, on in (('host', False), ('device', True), ('host2', False), ('device2', True)):  # alternating
      t = {}
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      pack = datasets.build_pack(paths, 'folder', torch.float16, dev, seed=1, timings=t, device_jpeg=on)
      torch.cuda.synchronize()
      out[label] = dict(total_ms=(time.perf_counter() - t0) * 1e3, read_ms=t['read'] * 1e3, device_ms=t['device'] * 1e3)
      if on:
        assert torch.equal(pack, keep)
      keep = pack
  row = dict(case='build_pack of %d small JPEGs (folder recipe, f16)' % n, **out)
  print(json.dumps(row), flush=True)
  return row


def markdown(rows, pack):
  out = ['| pictures | files | sampling | segments | device ms (min - max) | measured | settle / scan / emit / serial (entropy) / idct / rgb ms | x copy | '
         'file bytes to device codes ms | PIL open + convert + upload ms | vs PIL |', '|---|---|---|---|---|---|---|---|---|---|---|']
  for r in rows:
    d, k = r['device_ms'], r['kernels_ms']
    shares = 'not measured'
    if k:
      shares = ' / '.join('%.3f' % k.get(key, 0) for key in ('sync_settle', 'sync_scan', 'sync_emit')) + \
          ' / %.3f / %.3f / %.3f' % (k.get('sync_serial', 0) + k.get('entropy', 0), k.get('idct', 0), k.get('rgb', 0))
    out.append('| %s | %s | %s | %d | %.3f (%.3f - %.3f) | %s | %s | %.1f | %.1f | %.1f | %.2fx |' %
               (r['case'], r['files'], r['subsampling'], r['segments'], d['median'], d['min'], d['max'], r['measured'], shares,
                r['of_copy'], r['from_file_bytes_ms'], r['pil_ms'], r['speedup_vs_pil']))
  sync = [r for r in rows if 'sweep' in r]
  if sync:
    out += ['', 'Files without restart markers (DESIGN.md §3.36): the parallel walk at the default sub_bytes against the one-lane walk '
            '(`--jpeg-serial-entropy`) on the same files in the same process, the info words (pictures by 0 a lane per segment / 1 verified '
            'subsequences / 2 serial fallback) and the sweep of sub_bytes (device ms, info 1 / 2).', '',
            '| pictures | sampling | device ms | one-lane ms | measured | one-lane / parallel | info 0 / 1 / 2 | ' +
            ' | '.join('sub_bytes %d' % b for b in (64, 128, 256, 512)) + ' |', '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in sync:
      cells = ['%.3f (%d / %d)' % (r['sweep'][str(b)]['ms'], r['sweep'][str(b)]['info']['1'], r['sweep'][str(b)]['info']['2']) for b in (64, 128, 256, 512)]
      out.append('| %s | %s | %.3f | %.3f | %s | %.2fx | %d / %d / %d | %s |' %
                 (r['case'], r['subsampling'], r['device_ms']['median'], r['serial_ms']['median'], r['serial_measured'],
                  r['serial_ms']['median'] / r['device_ms']['median'], r['info']['0'], r['info']['1'], r['info']['2'], ' | '.join(cells)))
  text = '\n'.join(out) + '\n'
  if pack:
    text += '\n| %s | total ms | read ms | device ms |\n|---|---|---|---|\n' % pack['case']
    for label in ('host', 'device', 'host2', 'device2'):
      text += '| %s | %.1f | %.1f | %.1f |\n' % (label, pack[label]['total_ms'], pack[label]['read_ms'], pack[label]['device_ms'])
  return text


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--host-reps', type=int, default=3)
  ap.add_argument('--shapes', default='small,one,many')
  ap.add_argument('--quality', type=int, default=90)
  ap.add_argument('--slow-ms', type=float, default=1000.0)
  ap.add_argument('--kinds', default='own,pil')
  ap.add_argument('--pack', type=int, default=0)
  ap.add_argument('--out', default=None)
  ap.add_argument('--md', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  rows, pack = [], None

  def save():
    if args.out:
      with open(args.out, 'w') as fh:
        json.dump(dict(rows=rows, pack=pack), fh, indent=1)
    if args.md:
      with open(args.md, 'w') as fh:
        fh.write(markdown(rows, pack))

  if args.pack:
    pack = pack_case(args.pack, args, dev)
    save()
  for key in [k for k in args.shapes.split(',') if k]:
    n, h, w = SHAPES[key]
    rng = np.random.default_rng(n * 1000003 + h)
    for smooth in (True, False):
      pics = [picture(rng, h, w, smooth) for _ in range(n if key == 'small' else 1)]
      for sub in ('420', '444'):
        for kind in args.kinds.split(','):
          datas = [own_file(p, args.quality, sub, dev) if kind == 'own' else pil_file(p, args.quality, sub) for p in pics]
          datas = datas * (n // len(datas))
          rows.append(case('%d x %dx%d%s' % (n, h, w, ' smooth' if smooth else ''), kind, sub, datas, args, dev))
          save()  # (a row at a time: a run that ends early leaves what it measured)
          torch.cuda.empty_cache()
  save()


if __name__ == '__main__':
  main()
