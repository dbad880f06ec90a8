"""Timing and peak memory of retouching straight from integer codes with a generic agent (cfg.curve_steps = L, DESIGN.md
§3.27) against the path it replaces, both in this process, alternating round by round, warmed, timed with device events
around `--reps` calls:

  parent               retouch_batch(agent, decode_images(raws, ...), proxy='device', curves='fused', picture='u8')
  codes                retouch_batch_raw(agent, raws, ..., curves='fused', picture='u8')
  codes_pictures_only  the same with outputs=False

The agent has random seeded weights; z and the dropout masks are fixed, so every call takes the same steps.  The codes
are made on the device and staged once (`stage_raws`' records: codes and tables), so no host upload is inside the clock
and both paths read the same resident codes; the parent's own decode (its maximum, its division and the float tensors
it writes) is inside.  Codes: a smooth seeded gradient with noise (tools/bench_fused_decode.py's), or `--codes random`.
Peak memory is torch.cuda.max_memory_allocated over one call, above what is resident before it (codes, tables, agent).
The two paths' outputs and pictures are compared bit for bit before anything is timed.
A call is launch-bound by the agent's 64x64 steps; `--curve-dispatch` runs them on the per-image dispatch kernels
(§3.26), which shortens that part and leaves more of the full-resolution work visible.
usage: python tools/bench_curves_codes.py [--L 16] [--rounds 7] [--reps 3] [--big 16] [--curve-dispatch]
       [--out FILE.json] [--md FILE.md]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, 'tools')):
  if path not in sys.path:
    sys.path.insert(0, path)

from bench_fused_decode import make_codes, timed  # noqa: E402
from exposure_amd import _cabi, evaluate  # noqa: E402
from exposure_amd.agent import Agent  # noqa: E402
from exposure_amd.config import make_cfg  # noqa: E402


def case(name, sizes, kind, dtype, how, L, rounds, reps, dev, dispatch=False):
  n = len(sizes)
  cfg = make_cfg()
  cfg.curve_steps = L
  torch.manual_seed(16)
  agent = Agent(cfg).to(dev)
  agent.curve_dispatch = dispatch  # §3.26: the agent's own 64x64 step on the per-image dispatch kernels
  z = torch.rand((n, cfg.z_dim), device=dev)
  drops = [[(torch.rand(n, 4096, device=dev) < 0.5).float() for _ in range(2)] for _ in range(cfg.test_steps)]
  codes = make_codes(sizes, kind, how, dev, 100 + n)
  tables, stride = _cabi.decode_tables(codes, evaluate.decode_table(kind, dev), evaluate.DECODE_NORMALIZE[kind], dtype)
  staged = [(list(range(n)), codes, tables, stride, kind)]  # one group: what list(stage_raws(...)) holds
  raws = [(None, kind)] * n  # the host copies are never read once the codes are staged
  kw = dict(z=z, dropout_masks=drops, picture='u8')

  def parent():
    return evaluate.retouch_batch(agent, evaluate.decode_images(raws, dtype, dev, staged), proxy='device', curves='fused',
                                  **kw)

  def fused(outputs=True):
    return evaluate.retouch_batch_raw(agent, raws, dtype, dev, curves='fused', outputs=outputs, staged=staged, **kw)

  paths = {'parent': parent, 'codes': fused, 'codes_pictures_only': lambda: fused(False)}
  ref = parent()  # (the shared workspace grows to its size here, outside the measurements)
  got, bare = fused(), fused(False)
  for a, b, c in zip(ref[0], got[0], bare[0]):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and c is None, name
  for a, b, c in zip(ref[-1], got[-1], bare[-1]):
    assert torch.equal(a, b) and torch.equal(a, c), name
  assert torch.equal(ref[1], got[1]) and torch.equal(ref[2], got[2])
  del ref, got, bare
  peak = {}
  for key, fn in paths.items():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = fn()
    torch.cuda.synchronize()
    peak[key] = torch.cuda.max_memory_allocated() - base
    del res
  for fn in paths.values():
    for _ in range(2):
      fn()
  torch.cuda.synchronize()
  ms = {key: [] for key in paths}
  for _ in range(rounds):  # alternating
    for key, fn in paths.items():
      ms[key].append(timed(fn, reps))
  row = dict(case=name, images=n, pixels=sum(h * w for h, w in sizes), kind=kind, codes=how, L=L, curve_dispatch=dispatch,
             dtype='f16' if dtype is torch.float16 else 'f32')
  for key in paths:
    row[key + '_ms'] = statistics.median(ms[key])
    row[key + '_ms_min_max'] = [min(ms[key]), max(ms[key])]
    row[key + '_peak_bytes'] = peak[key]
  row['codes_over_parent'] = row['codes_ms'] / row['parent_ms']
  row['pictures_only_over_parent'] = row['codes_pictures_only_ms'] / row['parent_ms']
  return row


def markdown(rows):
  cell = lambda r, k: '%.2f (%.2f .. %.2f)' % ((r[k + '_ms'],) + tuple(r[k + '_ms_min_max']))
  mb = lambda r, k: '%.0f' % (r[k + '_peak_bytes'] / 1e6)
  out = ['| shape | kind | dtype | L | parent ms | codes ms | codes / parent | codes, pictures only ms | / parent | '
         'peak MB parent | codes | pictures only |', '|---|---|---|---|---|---|---|---|---|---|---|---|']
  for r in rows:
    out.append('| %s | %s | %s | %d | %s | %s | %.3f | %s | %.3f | %s | %s | %s |' % (
        r['case'], r['kind'], r['dtype'], r['L'], cell(r, 'parent'), cell(r, 'codes'), r['codes_over_parent'],
        cell(r, 'codes_pictures_only'), r['pictures_only_over_parent'], mb(r, 'parent'), mb(r, 'codes'),
        mb(r, 'codes_pictures_only')))
  return '\n'.join(out) + '\n'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--L', type=int, default=16)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--big', type=int, default=16, help='number of 4000x6000 images of the large case')
  ap.add_argument('--codes', default='gradient', choices=('gradient', 'random'))
  ap.add_argument('--dtype', default='f16', choices=('f16', 'f32'))
  ap.add_argument('--curve-dispatch', action='store_true', help='Agent.curve_dispatch: the shorter agent step')
  ap.add_argument('--only', default=None, help='run the cases whose name contains this')
  ap.add_argument('--out', default=None, help='write the rows as JSON')
  ap.add_argument('--md', default=None, help='write the table as markdown')
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  dtype = torch.float16 if args.dtype == 'f16' else torch.float32
  rows = []
  for name, sizes in (('16x512x512', [(512, 512)] * 16), ('%dx24MP' % args.big, [(4000, 6000)] * args.big)):
    for kind in ('srgb8', 'prophoto16'):
      if args.only and args.only not in name:
        continue
      r = case(name, sizes, kind, dtype, args.codes, args.L, args.rounds, args.reps, dev, args.curve_dispatch)
      print(json.dumps(r), flush=True)
      rows.append(r)
      torch.cuda.empty_cache()
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(rows, f, indent=1)
  if args.md:
    with open(args.md, 'w') as f:
      f.write(markdown(rows))


if __name__ == '__main__':
  main()
