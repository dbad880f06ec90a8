"""Timing of the agent's per-image dispatch step for any cfg.curve_steps: every variant against the
code path it replaces -- `Agent.curve_dispatch` off in the same build -- alternating round by round after warm-up, device
events around `reps` calls, median of `--rounds` (min .. max).

Kernel level, 64x64x64 fp16, seeded filter ids in 0..7, parameters from the oracle's regressors, forward (with the fused
penalty) and backward (dx, dparams, dpenalty):
  new_L8 / new_L16   expo_filter_dispatch_curves_fwd / _bwd
  tuned_L8           expo_filter_dispatch_fwd / _bwd on the same ids (24-wide rows)
  stack_L16          the eight whole-batch launches of the stack-and-select step: expo_filter_fwd / _bwd of the six light
                     filters, expo_curve_fwd / _bwd of Tone and Color (kernels only: the one-hot products, sums and the
                     penalty of that path are torch launches on top)
Training, cfg.curve_steps = 16, batch 64, step graphs on: `generator_step` and `train_iteration`, switch off / on, the
8-step iteration beside them as the floor; kernel launches of one eager generator step counted with the profiler.
Inference: `retouch` at 16x512x512 fp16, cfg.curve_steps = 16, curves='fused', switch off / on (wall time with a device
synchronise around each call: the agent's host loop is part of it).

usage: python tools/bench_curve_dispatch.py [--rounds 7] [--reps 200] [--step-reps 20] [--it-reps 5] [--e2e-reps 5]
                                            [--out profiles/curve_dispatch.md] [--json profiles/curve_dispatch_bench.json]"""
import argparse
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
from exposure_amd.gan import GAN  # noqa: E402
from oracle import filters_np as fnp  # noqa: E402


def timed(fn, reps):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) * 1e3 / reps  # us


def summary(v):
  return dict(us=statistics.median(v), us_min=min(v), us_max=max(v))


def alternate(fns, rounds, reps, warm=3):
  for fn in fns.values():
    for _ in range(warm):
      fn()
  torch.cuda.synchronize()
  ts = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      ts[k].append(timed(fn, reps))
  return {k: summary(v) for k, v in ts.items()}


def num_params(fid, L):
  return L if fid == 4 else 3 * L if fid == 7 else fnp.NUM_PARAMS[fid]


def kernel_level(rounds, reps, dev):
  n, shape = 64, (64, 64, 64, 3)
  rng = np.random.default_rng(64)
  x = torch.from_numpy(synthetic.make_images(rng, shape, np.float16) * np.float16(1.3)).to(dev)
  dy = torch.from_numpy(synthetic.make_grad(rng, shape, np.float16)).to(dev)
  ids_np = rng.integers(0, 8, n).astype(np.int32)
  feats = rng.standard_normal((n, 48))
  ids = torch.from_numpy(ids_np).to(dev)
  dpen = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)

  def rows(L, width):
    cfg = dict(fnp.DEFAULT_CFG, curve_steps=L)
    p = np.zeros((n, width), dtype=np.float32)
    for i, fid in enumerate(ids_np):
      m = num_params(int(fid), L)
      p[i, :m] = fnp.regress_packed(int(fid), feats[i:i + 1, :m], cfg)[0]
    return torch.from_numpy(p).to(dev)

  p24, p48_8, p48_16 = rows(8, 24), rows(8, 48), rows(16, 48)
  y, dx, pen = torch.empty_like(x), torch.empty_like(x), torch.empty(n, device=dev)
  d24, d48 = torch.empty_like(p24), torch.empty_like(p48_16)
  cfg16 = dict(fnp.DEFAULT_CFG, curve_steps=16)
  whole = {fid: torch.from_numpy(fnp.regress_packed(fid, rng.standard_normal((n, num_params(fid, 16))), cfg16).astype(np.float32)).to(dev)
           for fid in range(8)}
  dwhole = {fid: torch.empty_like(p) for fid, p in whole.items()}

  def stack_fwd():
    for fid in range(8):
      if fid in (4, 7):
        _cabi.curve_fwd(x, y, whole[fid], 1 if fid == 4 else 3, 16)
      else:
        _cabi.filter_fwd(fid, x, y, whole[fid])

  def stack_bwd():
    for fid in range(8):
      if fid in (4, 7):
        _cabi.curve_bwd(x, dy, dx, whole[fid], dwhole[fid], 1 if fid == 4 else 3, 16)
      else:
        _cabi.filter_bwd(fid, x, dy, dx, whole[fid], dwhole[fid])

  fwd = dict(new_L8=lambda: _cabi.dispatch_curves_fwd(ids, x, y, p48_8, 8, pen),
             new_L16=lambda: _cabi.dispatch_curves_fwd(ids, x, y, p48_16, 16, pen),
             tuned_L8=lambda: _cabi.dispatch_fwd(ids, x, y, p24, pen), stack_L16=stack_fwd)
  bwd = dict(new_L8=lambda: _cabi.dispatch_curves_bwd(ids, x, dy, dx, p48_8, d48, 8, dpen),
             new_L16=lambda: _cabi.dispatch_curves_bwd(ids, x, dy, dx, p48_16, d48, 16, dpen),
             tuned_L8=lambda: _cabi.dispatch_bwd(ids, x, dy, dx, p24, d24, dpen), stack_L16=stack_bwd)
  return dict(shape='64x64x64', curve_images=int(((ids_np == 4) | (ids_np == 7)).sum()),
              forward=alternate(fwd, rounds, reps, warm=20), backward=alternate(bwd, rounds, reps, warm=20))


def make_memory(cfg, dev):
  from exposure_amd.replay_memory import ReplayMemory, ResidentProvider
  return ReplayMemory(cfg, ResidentProvider(dev, dtype=torch.float16, seed=1, count=512),
                      ResidentProvider(dev, gamma=1.0, dtype=torch.float16, seed=2, count=512), seed=0)


def count_launches(cfg, switch, dev, feed):
  """kernel launches of ONE eager generator step (forward, backward, optimiser), from the profiler; None if it has no
  device activity to show"""
  try:
    from torch.profiler import ProfilerActivity, profile
    torch.manual_seed(0)
    gan = GAN(cfg, device=dev, use_graphs=False, seed=4, curve_dispatch=switch)
    for it in (1, 2):
      gan.generator_step(feed['fake_input'], feed['z'], feed['states'], 0.1, it=it)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
      gan.generator_step(feed['fake_input'], feed['z'], feed['states'], 0.1, it=3)
      torch.cuda.synchronize()
    count = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA and
                'Memcpy' not in e.key and 'Memset' not in e.key)
    return int(count) or None
  except Exception as e:  # the profiler is a convenience here, not the measurement
    print('launch count not available: %s' % e, file=sys.stderr)
    return None


def training(rounds, step_reps, it_reps, dev):
  variants = {'L16_off': (16, False), 'L16_on': (16, True), 'L8': (8, False)}
  gans, mems, feeds, launches = {}, {}, {}, {}
  for name, (L, switch) in variants.items():
    cfg = make_cfg()
    cfg.curve_steps = L
    torch.manual_seed(0)
    gan = GAN(cfg, device=dev, use_graphs=True, seed=4, curve_dispatch=switch)
    mem = make_memory(cfg, dev)
    for _ in range(8):  # iteration 0's roll-out, shortened: terminated records for the critic
      feed, feats = mem.get_feed_dict_and_states(cfg.batch_size, lazy=False)
      feed = {k: v.clone() for k, v in feed.items() if torch.is_tensor(v)}  # (the last one: the timed step's fixed batch)
      g = gan.generator_step(feed['fake_input'], feed['z'], feed['states'], 0.0, it=0)
      mem.replace_memory(g['fake_output'], g['new_states'], feats, advanced=True)
    gans[name], mems[name], feeds[name] = gan, mem, feed
    launches[name] = count_launches(cfg, switch, dev, feed)
  its = {k: 1 for k in variants}

  def step(k):
    def run():
      gans[k].generator_step(feeds[k]['fake_input'], feeds[k]['z'], feeds[k]['states'], 0.1, it=5)
    return run

  def iteration(k):
    def run():
      gans[k].train_iteration(mems[k], its[k])
      its[k] += 1
    return run

  res = dict(batch=int(gans['L8'].cfg.batch_size), citers=int(gans['L8'].cfg.citers), launches_per_generator_step=launches,
             generator_step=alternate({k: step(k) for k in variants}, rounds, step_reps),
             train_iteration=alternate({k: iteration(k) for k in variants}, rounds, it_reps))
  return res


def inference(rounds, reps, dev):
  n, L, H, W = 16, 16, 512, 512
  cfg = make_cfg()
  cfg.curve_steps = L
  torch.manual_seed(0)
  ag = xagent.Agent(cfg).to(dev)
  rng = np.random.default_rng(5)
  x = torch.from_numpy(synthetic.make_images(rng, (n, H, W, 3), np.float16)).to(dev)
  g = torch.Generator(device='cpu').manual_seed(1)
  z = torch.rand((n, cfg.z_dim), generator=g).to(dev)
  masks = [[(torch.rand((n, 4096), generator=g) < 0.5).float().to(dev) for _ in range(2)] for _ in range(cfg.test_steps)]

  def call(switch):
    ag.curve_dispatch = switch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate.retouch(ag, x, z=z, dropout_masks=masks, return_trace=True, curves='fused')
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out

  outs = {}
  for s in (False, True):
    for _ in range(3):
      _, outs[s] = call(s)
  ts = {False: [], True: []}
  for _ in range(rounds):
    for s in ts:
      ts[s].append(statistics.mean(call(s)[0] for _ in range(reps)))
  return dict(shape='%dx%dx%d' % (n, H, W), curve_steps=L, off=summary(ts[False]), on=summary(ts[True]),
              same_filters=bool(torch.equal(outs[False][3], outs[True][3])),
              max_abs_diff=float((outs[False][0].float() - outs[True][0].float()).abs().max()))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--reps', type=int, default=200)
  ap.add_argument('--step-reps', type=int, default=20)
  ap.add_argument('--it-reps', type=int, default=5)
  ap.add_argument('--e2e-reps', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'curve_dispatch.md'))
  ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'curve_dispatch_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_curve_dispatch needs a ROCm GPU'
  dev = torch.device('cuda:0')
  kern = kernel_level(args.rounds, args.reps, dev)
  train = training(args.rounds, args.step_reps, args.it_reps, dev)
  infer = inference(args.rounds, args.e2e_reps, dev)
  cell = lambda r: '%.1f (%.1f .. %.1f)' % (r['us'], r['us_min'], r['us_max'])
  ms = lambda r: '%.3f (%.3f .. %.3f)' % (r['us'] / 1e3, r['us_min'] / 1e3, r['us_max'] / 1e3)
  apart = lambda a, b: 'yes' if a['us_max'] < b['us_min'] else 'no'
  lines = ['# Per-image dispatch step for any cfg.curve_steps', '', 'Device: %s' % torch.cuda.get_device_name(0), '',
           '## Kernel level: %s fp16, %d of 64 images select a curve; median of %d rounds x %d calls, device events '
           '(us; min .. max)' % (kern['shape'], kern['curve_images'], args.rounds, args.reps), '',
           '| direction | new entry, L = 8 | new entry, L = 16 | tuned dispatch (L = 8) | eight whole-batch launches (L = 16) |',
           '|---|---|---|---|---|']
  for d in ('forward', 'backward'):
    r = kern[d]
    lines.append('| %s | %s | %s | %s | %s |' % (d, cell(r['new_L8']), cell(r['new_L16']), cell(r['tuned_L8']), cell(r['stack_L16'])))
  lines += ['', '## Training: batch %d, step graphs on, %d critic steps per iteration; median of %d rounds, device events '
            '(ms; min .. max)' % (train['batch'], train['citers'], args.rounds), '',
            '| | L = 16, switch off | L = 16, switch on | off / on | ranges apart | L = 8 (floor) |', '|---|---|---|---|---|---|']
  for key, reps in (('generator_step', args.step_reps), ('train_iteration', args.it_reps)):
    r = train[key]
    lines.append('| %s (x %d calls) | %s | %s | %.2f | %s | %s |' % (key, reps, ms(r['L16_off']), ms(r['L16_on']),
                                                                  r['L16_off']['us'] / r['L16_on']['us'],
                                                                  apart(r['L16_on'], r['L16_off']), ms(r['L8'])))
  la = train['launches_per_generator_step']
  lines += ['', 'Kernel launches of one eager generator step (profiler): L = 16 off %s, on %s; L = 8 %s.' % (
      la['L16_off'], la['L16_on'], la['L8']), '',
            '## Inference: retouch, %s fp16, cfg.curve_steps = %d, curves=\'fused\', wall time with a device synchronise '
            'around each call, median of %d rounds x %d calls (ms; min .. max)' % (infer['shape'], infer['curve_steps'],
                                                                                  args.rounds, args.e2e_reps), '',
            '| switch off | switch on | off / on | ranges apart | same filters | max abs diff |', '|---|---|---|---|---|---|',
            '| %s | %s | %.2f | %s | %s | %.3e |' % (ms(infer['off']), ms(infer['on']), infer['off']['us'] / infer['on']['us'],
                                                    apart(infer['on'], infer['off']), infer['same_filters'], infer['max_abs_diff']),
            '', 'Not measured: fp32 storage, other batch sizes, the high_res op-by-op path, multi-GPU training, the CLIs.']
  text = '\n'.join(lines) + '\n'
  for path in (args.out, args.json):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)
  with open(args.json, 'w') as f:
    json.dump(dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, step_reps=args.step_reps,
                   it_reps=args.it_reps, e2e_reps=args.e2e_reps, kernel=kern, training=train, inference=infer), f, indent=1,
              sort_keys=True)
    f.write('\n')
  print(text)


if __name__ == '__main__':
  main()
