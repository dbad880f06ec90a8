"""``python -m exposure_amd.train [--iters N]`` -- the tensor part of the reference's
``train.py:9-14`` / ``GAN.train`` (``net.py:298-403``) on synthetic FiveK-shaped data: the G/V and
critic alternation with the device-resident replay memory, one hipGraph replay per optimisation
step.  ``--fake-dir`` / ``--real-dir`` train on folders of photos instead (``datasets.py``: the reference's FiveK and
folder recipes, master packs built on the device, re-cut every epoch; ``--pack-cache`` keeps the packs).  TensorBoard,
PNG dashboards and checkpoints of the reference are out of scope; ``--save`` writes weights + optimiser state with ``torch.save`` (``--resume`` reads it), ``--save-tf`` a TF-1 checkpoint
(``checkpoint.py``, ``tf_bundle.py``).

Note on the numbers it prints: with random-init weights the policy can chain Exposure (x11) and
Gamma (power 3) steps, so pixel values -- and with them the over-exposure penalty, the critic logits
and the value targets -- occasionally overflow float32 in the first iterations.  That is the
reference's arithmetic (``filters.py:181-182, 205-206`` have no clamp; ``cfg.clamp`` is off), not
a kernel artefact; ``--clamp`` turns on the reference's own ``clip_by_value(net, 0, 5)``
(``agent.py:240-241``)."""
import argparse
import os
import time

import torch

from .config import make_cfg
from .gan import GAN
from .replay_memory import ReplayMemory, ResidentProvider


def parse_args(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=20, help='training iterations to run (the reference runs 20000)')
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--log-every', type=int, default=10)
  ap.add_argument('--no-graphs', action='store_true')
  ap.add_argument('--save', default=None, help="torch.save of {'model': state_dict, 'optim': Adam slots, step counters, "
                  "learning rates and the logit centre's average} -- what the reference's tf.train.Saver keeps (net.py:271)")
  ap.add_argument('--resume', default=None, help='a file written by --save: weights and optimiser state are restored in place')
  ap.add_argument('--save-tf', default=None, metavar='MODEL_DIR',
                  help="also write MODEL_DIR/model.ckpt-<iters> in TensorFlow's checkpoint format, variable names and "
                  "layouts as the reference's graph declares them (net.py:380-384)")
  ap.add_argument('--clamp', action='store_true', help='cfg.clamp = True (agent.py:240-241)')
  ap.add_argument('--curve-steps', type=int, default=None, metavar='L',
                  help='cfg.curve_steps, 1..16 (default 8): the knots of the Tone and Color curves (L != 8 trains on '
                  'the generic curve kernels)')
  ap.add_argument('--curve-dispatch', action='store_true',
                  help='with --curve-steps other than 8: the agent\'s step on the per-image dispatch kernels for any step '
                  'count (one selection, one regress-and-gather and one dispatch launch each way) instead of running '
                  'every filter on the whole batch')
  ap.add_argument('--dtype', default='f32', choices=['f32', 'f16'], help='storage type of the image pool')
  ap.add_argument('--fake-dir', default=None, help='folder of input photos (with --real-dir; default: synthetic data)')
  ap.add_argument('--real-dir', default=None, help='folder of target photos (with --fake-dir)')
  ap.add_argument('--fake-recipe', default='fivek', choices=['fivek', 'folder'], help='preprocessing of --fake-dir')
  ap.add_argument('--real-recipe', default='folder', choices=['fivek', 'folder'], help='preprocessing of --real-dir')
  ap.add_argument('--fake-list', default=None, help='fold file selecting --fake-dir files (1-based indices)')
  ap.add_argument('--real-list', default=None, help='fold file selecting --real-dir files (1-based indices)')
  ap.add_argument('--read-limit', type=int, default=-1, help='read at most this many files of each folder')
  ap.add_argument('--pack-cache', default=None, metavar='DIR', help='keep the built packs under DIR/fake and DIR/real')
  ap.add_argument('--device-jpeg-decode', action='store_true',
                  help="decode the folder recipe's baseline JPEG files on the device from their bytes (DESIGN.md 3.35): "
                  'the same pack, bit for bit; other files go through PIL as before')
  ap.add_argument('--jpeg-serial-entropy', action='store_true',
                  help='with --device-jpeg-decode: walk a file without restart markers with one lane instead of a lane per '
                  'subsequence (DESIGN.md 3.36), for comparison runs; the same pack')
  args = ap.parse_args(argv)
  if args.curve_steps is not None and not 1 <= args.curve_steps <= 16:
    ap.error('--curve-steps must be in 1..16')
  if (args.fake_dir is None) != (args.real_dir is None):
    ap.error('--fake-dir and --real-dir go together')
  if args.fake_dir is None:
    for flag in ('fake_list', 'real_list', 'pack_cache'):
      if getattr(args, flag) is not None:
        ap.error('--%s needs --fake-dir and --real-dir' % flag.replace('_', '-'))
    if args.read_limit != -1:
      ap.error('--read-limit needs --fake-dir and --real-dir')
  for d in (args.fake_dir, args.real_dir):
    if d is not None and not os.path.isdir(d):
      ap.error('%s is not a directory' % d)
  for f in (args.fake_list, args.real_list):
    if f is not None and not os.path.isfile(f):
      ap.error('%s is not a file' % f)
  return args


def photo_providers(args, cfg, dev, dt):
  """The two PackProviders of --fake-dir / --real-dir (packs from --pack-cache when they match)."""
  from .datasets import PackProvider, cached_pack
  provs = []
  for role, k in (('fake', 1), ('real', 2)):
    folder, recipe, fold = getattr(args, role + '_dir'), getattr(args, role + '_recipe'), getattr(args, role + '_list')
    cache = os.path.join(args.pack_cache, role) if args.pack_cache else None
    t0 = time.time()
    master, hit = cached_pack(folder, recipe, dt, dev, args.seed + k, fold=fold, read_limit=args.read_limit, cache=cache,
                              device_jpeg=args.device_jpeg_decode, jpeg_sync=False if args.jpeg_serial_entropy else 'auto')
    print('%s pack: %d rows of %d x %d from %s (%s recipe, %s, %.1f s)' %
          (role, master.shape[0], master.shape[1], master.shape[2], folder, recipe,
           'cache hit' if hit else 'built', time.time() - t0))
    if master.shape[0] < cfg.batch_size:
      raise SystemExit('%s pack has %d rows, fewer than one batch (%d): add photos' %
                       (role, master.shape[0], cfg.batch_size))
    provs.append(PackProvider(master, crop_size=64, seed=args.seed + k))
  return provs


def main(argv=None):
  args = parse_args(argv)
  dev = torch.device('cuda:0')
  torch.manual_seed(args.seed)
  cfg = make_cfg()
  cfg.clamp = bool(args.clamp)
  if args.curve_steps is not None:
    cfg.curve_steps = args.curve_steps
  gan = GAN(cfg, device=dev, use_graphs=not args.no_graphs, seed=args.seed, curve_dispatch=args.curve_dispatch)  # (--seed also drives dropout / alpha)
  dt = torch.float32 if args.dtype == 'f32' else torch.float16
  if args.fake_dir is not None:
    fake, real = photo_providers(args, cfg, dev, dt)
  else:
    # toy task with the statistics of the real one: dark linear-RAW-like inputs, brighter targets
    # (both synthetic data sets resident in HBM: 4 096 images each, served as views)
    fake = ResidentProvider(dev, gamma=2.2, scale=0.35, dtype=dt, seed=args.seed + 1)
    real = ResidentProvider(dev, gamma=1.2, scale=0.9, dtype=dt, seed=args.seed + 2)
  memory = ReplayMemory(cfg, fake, real, seed=args.seed)
  if args.resume:
    ckpt = torch.load(args.resume, map_location=dev)
    gan.load_state_dict(ckpt['model'] if 'model' in ckpt else ckpt)
    if 'optim' in ckpt:
      gan.load_optimizer_state_dict(ckpt['optim'])
  t0 = time.time()
  hist = gan.train(memory, max_iter_step=args.iters, log_every=args.log_every)
  torch.cuda.synchronize()
  dt = time.time() - t0
  print('%d iterations in %.1f s (iteration 0 = 100 warm-up generator steps + 100 critic steps, net.py:314-323)' %
        (len(hist), dt))
  if args.save:
    torch.save({'model': gan.state_dict(), 'optim': gan.optimizer_state_dict()}, args.save)
  if args.save_tf:
    from . import checkpoint
    print('wrote', checkpoint.save(gan, args.save_tf, args.iters))
  return hist


if __name__ == '__main__':
  main()
