"""Timing of the fused inference pass for any cfg.curve_steps, fp16, 5 steps, seeded filter ids in
0..7, parameters from the oracle's regressors on seeded features.

Kernel level, at 16x512x512 and 64x512x512: three ways through the same images, timed with device events around
`--reps` calls after warm-up, alternating round by round, median of `--rounds` (min .. max):
  tuned_L8    expo_chain_fused_fwd_ragged, the pass built for 8-step curves, 24-wide rows
  curves_L8   expo_chain_fused_curves_fwd_ragged at L = 8 on the same ids and parameters (48-wide rows): what a runtime
              L costs against the tuned pass
  curves_L16  the same entry at L = 16 (the same ids; curve rows regressed for 16 knots)
The C entry points are called through ctypes with the argument arrays built once, so the windows hold device work and
not the binding's per-image checks.

End to end, 16x512x512 fp16, cfg.curve_steps = 16, a random-init agent, fixed z and dropout masks:
  stepwise    retouch(agent, x, curves='stepwise'): the schedule without the new pass (every filter's kernel on the
              full-resolution tensor at every step)
  fused       retouch(agent, x, curves='fused')
Wall time with a device synchronise around each call (the agent's host loop is part of it), `--e2e-reps` calls per
round, the two alternating, median of `--rounds`.

usage: python tools/bench_curves_chain.py [--rounds 7] [--reps 200] [--e2e-reps 5] [--out profiles/curves_chain.md]
                                          [--json profiles/curves_chain_bench.json]"""
import argparse
import ctypes
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
from exposure_amd import agent as xagent  # noqa: E402
from exposure_amd.config import make_cfg  # noqa: E402
from oracle import filters_np as fnp  # noqa: E402

STEPS, H, W = 5, 512, 512


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) * 1e3 / reps  # us


def rows(ids, feats, L, width):
  """(n, STEPS, width) packed rows from per-(image, step) features (48 standard normals each); zero-padded"""
  cfg = dict(fnp.DEFAULT_CFG, curve_steps=L)
  n = ids.shape[0]
  p = np.zeros((n, STEPS, width), dtype=np.float32)
  for i in range(n):
    for k in range(STEPS):
      fid = int(ids[i, k])
      m = L if fid == 4 else 3 * L if fid == 7 else fnp.NUM_PARAMS[fid]
      p[i, k, :m] = fnp.regress_packed(fid, feats[i, k:k + 1, :m], cfg)[0]
  return p


def summary(v):
  return dict(us=statistics.median(v), us_min=min(v), us_max=max(v))


def kernel_case(n, rounds, reps, dev):
  lib = _cabi.load()
  rng = np.random.default_rng(n)
  x = torch.from_numpy(synthetic.make_images(rng, (n, H, W, 3), np.float16)).to(dev)
  ids_np = rng.integers(0, 8, (n, STEPS)).astype(np.int32)
  feats = rng.standard_normal((n, STEPS, 48))
  ids = torch.from_numpy(ids_np).to(dev)
  p24 = torch.from_numpy(rows(ids_np, feats, 8, 24)).to(dev)
  p48_8 = torch.from_numpy(rows(ids_np, feats, 8, 48)).to(dev)
  p48_16 = torch.from_numpy(rows(ids_np, feats, 16, 48)).to(dev)
  y_tuned, y_8, y_16 = (torch.empty_like(x) for _ in range(3))
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())
  xs = _cabi._ptr_array(list(x.unbind(0)))
  ya, yb, yc = (_cabi._ptr_array(list(y.unbind(0))) for y in (y_tuned, y_8, y_16))
  hs, ws = (ctypes.c_int * n)(*[H] * n), (ctypes.c_int * n)(*[W] * n)

  def tuned_L8():
    rc = lib.expo_chain_fused_fwd_ragged(ptr(ids), ptr(p24), STEPS, xs, ya, hs, ws, n, _cabi.EXPO_F16, stream)
    assert rc == 0, lib.expo_last_error()

  def curves(prm, L, ys):
    rc = lib.expo_chain_fused_curves_fwd_ragged(ptr(ids), ptr(prm), STEPS, L, xs, ys, hs, ws, n, _cabi.EXPO_F16, 0,
                                                _cabi.EXPO_TAP_STORAGE, None, stream)
    assert rc == 0, lib.expo_last_error()

  fns = dict(tuned_L8=tuned_L8, curves_L8=lambda: curves(p48_8, 8, yb), curves_L16=lambda: curves(p48_16, 16, yc))
  for fn in fns.values():  # warm-up: code objects, clocks
    for _ in range(20):
      fn()
  torch.cuda.synchronize()
  diff = float((y_tuned.float() - y_8.float()).abs().max())
  ts = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      ts[k].append(timed(fn, reps))
  res = {k: summary(v) for k, v in ts.items()}
  res['shape'] = '%dx%dx%d' % (n, H, W)
  res['max_abs_diff_curves_L8_vs_tuned'] = diff
  res['curve_steps_in_ids'] = int(((ids_np == 4) | (ids_np == 7)).sum())
  res['bytes_moved'] = 2 * n * H * W * 3 * 2
  return res


def end_to_end(rounds, reps, dev):
  n, L = 16, 16
  cfg = make_cfg()
  cfg.curve_steps = L
  torch.manual_seed(0)
  ag = xagent.Agent(cfg).to(dev)
  rng = np.random.default_rng(5)
  x = torch.from_numpy(synthetic.make_images(rng, (n, H, W, 3), np.float16)).to(dev)
  g = torch.Generator(device='cpu').manual_seed(1)
  z = torch.rand((n, cfg.z_dim), generator=g).to(dev)
  masks = [[(torch.rand((n, 4096), generator=g) < 0.5).float().to(dev) for _ in range(2)] for _ in range(cfg.test_steps)]

  def call(curves):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate.retouch(ag, x, z=z, dropout_masks=masks, return_trace=True, curves=curves)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out

  outs = {}
  for c in ('stepwise', 'fused'):
    for _ in range(3):
      _, outs[c] = call(c)
  same = bool(torch.equal(outs['stepwise'][3], outs['fused'][3]))
  diff = float((outs['stepwise'][0].float() - outs['fused'][0].float()).abs().max())
  scale = float(outs['stepwise'][0].float().abs().max())
  ts = dict(stepwise=[], fused=[])
  for _ in range(rounds):
    for c in ts:
      ts[c].append(statistics.mean(call(c)[0] for _ in range(reps)))
  res = {c: summary(v) for c, v in ts.items()}
  res.update(shape='%dx%dx%d' % (n, H, W), curve_steps=L, same_filters=same, max_abs_diff=diff, max_abs_value=scale,
             filters=[ag.filters[int(j)].get_short_name() for j in outs['fused'][3][0]])
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=200)
  ap.add_argument('--e2e-reps', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'curves_chain.md'))
  ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'curves_chain_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_curves_chain needs a ROCm GPU'
  dev = torch.device('cuda:0')
  kern = [kernel_case(n, args.rounds, args.reps, dev) for n in (16, 64)]
  e2e = end_to_end(args.rounds, args.e2e_reps, dev)
  cell = lambda r, k: '%.1f (%.1f .. %.1f)' % (r[k]['us'], r[k]['us_min'], r[k]['us_max'])
  lines = ['# Fused chain for any cfg.curve_steps: fp16, %d steps' % STEPS, '', 'Device: %s' % torch.cuda.get_device_name(0),
           '', '## Kernel level: median of %d rounds x %d calls, device events (us; min .. max)' % (args.rounds, args.reps),
           '',
           '| shape | tuned pass (L = 8) | new entry, L = 8 | new entry, L = 16 | L8 new / tuned | L16 new / tuned | new L = 8 GB/s (12 B/px) | max abs diff new L = 8 vs tuned |',
           '|---|---|---|---|---|---|---|---|']
  for r in kern:
    lines.append('| %s | %s | %s | %s | %.3f | %.3f | %.0f | %.3e |' % (
        r['shape'], cell(r, 'tuned_L8'), cell(r, 'curves_L8'), cell(r, 'curves_L16'),
        r['curves_L8']['us'] / r['tuned_L8']['us'], r['curves_L16']['us'] / r['tuned_L8']['us'],
        r['bytes_moved'] / (r['curves_L8']['us'] * 1e-6) / 1e9, r['max_abs_diff_curves_L8_vs_tuned']))
  lines += ['', '(%s of the %s (image, step) pairs are curve steps at 16 images, %s of %s at 64.)' % (
      kern[0]['curve_steps_in_ids'], 16 * STEPS, kern[1]['curve_steps_in_ids'], 64 * STEPS), '',
            '## End to end: retouch, %s fp16, cfg.curve_steps = %d, wall time with a device synchronise around each call, '
            'median of %d rounds x %d calls (us; min .. max)' % (e2e['shape'], e2e['curve_steps'], args.rounds, args.e2e_reps),
            '', '| curves=\'stepwise\' | curves=\'fused\' | stepwise / fused | same filters | max abs diff (values up to) |',
            '|---|---|---|---|---|',
            '| %s | %s | %.2f | %s | %.3e (%.3g) |' % (cell(e2e, 'stepwise'), cell(e2e, 'fused'),
                                                      e2e['stepwise']['us'] / e2e['fused']['us'], e2e['same_filters'],
                                                      e2e['max_abs_diff'], e2e['max_abs_value']),
            '', 'Filters of image 0: %s.' % ' '.join(e2e['filters']), '',
            'Not measured: the tap variants, fp32 storage, retouch_batch on mixed sizes, the CLI.']
  text = '\n'.join(lines) + '\n'
  for path in (args.out, args.json):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)
  with open(args.json, 'w') as f:
    json.dump(dict(device=torch.cuda.get_device_name(0), steps=STEPS, rounds=args.rounds, reps=args.reps,
                   e2e_reps=args.e2e_reps, kernel=kern, end_to_end=e2e), f, indent=1, sort_keys=True)
    f.write('\n')
  print(text)


if __name__ == '__main__':
  main()
