"""The paper's evaluation metric (``/root/reference/histogram_intersection.py``): histogram
intersection of per-image luminance mean, contrast (2 x luminance std) and HLS saturation between a
set of retouched images and a set of target images.  The statistics are tensor-in / number-out and run on
whatever device the images live on; ``read_images`` and ``python -m exposure_amd.metrics OUT_DIR TARGET_DIR``
restate the script's file side (``histogram_intersection.py:36-76``: every file -> 4 random square crops ->
80x80 by area averaging -> 4 random 64x64 patches each) with PIL instead of cv2.

The device path computes the same number from 8-bit pictures that are already on the GPU:
``set_statistics`` (decode, exact INTER_AREA, ``expo_patch_stats``) gives a set's (16 F, 3) statistics, ``score`` the
intersections of two sets' histograms (``expo_stat_hist``); ``read_statistics`` is the file side and
``python -m exposure_amd.metrics --device OUT_DIR TARGET_DIR`` the script."""
import os
import random

import torch

HIST_BINS = 32  # histogram_intersection.py:8
MAIN_SIZE, PATCH_SIZE = 80, 64  # histogram_intersection.py:48-56: the resized crop and the patches cut from it


def hls_saturation(img):
  """S channel of cv2.cvtColor(img, COLOR_RGB2HLS) for float images in [0,1] (NHWC):
  L = (max+min)/2;  S = (max-min)/(max+min) if L < 0.5 else (max-min)/(2-max-min);  0 if max == min."""
  mx = img.amax(dim=-1)
  mn = img.amin(dim=-1)
  d = mx - mn
  l = (mx + mn) * 0.5
  den = torch.where(l < 0.5, mx + mn, 2.0 - mx - mn)
  return torch.where(d > 0, d / den.clamp_min(1e-12), torch.zeros_like(d))


def get_statistics(images):
  """histogram_intersection.py:15-20 for a batch (N,H,W,3) -> (N,3) [lum mean, 2*lum std, mean sat]."""
  img = images.float().clamp(0.0, 1.0)
  lum = img[..., 0] * 0.27 + img[..., 1] * 0.67 + img[..., 2] * 0.06
  sat = hls_saturation(img).mean(dim=(1, 2))
  return torch.stack([lum.mean(dim=(1, 2)), lum.std(dim=(1, 2), unbiased=False) * 2, sat], dim=1)


def calc_hist(arr, nbins=HIST_BINS, xrange=(0.0, 1.0)):
  """histogram_intersection.py:23-25 (np.histogram semantics: values outside the range are dropped,
  the right edge is inclusive)."""
  arr = arr.float()
  inside = (arr >= xrange[0]) & (arr <= xrange[1])
  h = torch.histc(arr[inside], bins=nbins, min=xrange[0], max=xrange[1])
  return h / float(arr.numel())


def hist_intersection(a, b):
  """histogram_intersection.py:11-12."""
  return torch.minimum(a, b).sum()


def histogram_intersection(output_images, target_images):
  """histogram_intersection.py:62-76 -> (three intersections, their average), as floats in [0,1]."""
  so, st = get_statistics(output_images), get_statistics(target_images)
  ints = [float(hist_intersection(calc_hist(so[:, k]), calc_hist(st[:, k]))) for k in range(3)]
  return ints, sum(ints) / len(ints)


def read_images(src, tag=None, rng=None, device='cpu'):
  """histogram_intersection.py:36-59 -> (16 * files, 64, 64, 3) float32 in [0, 1].  ``rng``: a ``random.Random``
  (the script uses the module-level generator, i.e. a different sample every run).  The 80x80 reduction is an area
  average (``cv2.INTER_AREA``; for crops that are not a multiple of 80 the window edges are rounded to whole pixels
  here, where cv2 weights the partial ones)."""
  import numpy as np
  from PIL import Image
  rng = rng or random
  patches = []
  for f in sorted(os.listdir(src)):
    if tag and f.find(tag) == -1:
      continue
    image = np.asarray(Image.open(os.path.join(src, f)).convert('RGB'), dtype=np.float32) / 255.0
    edge = min(image.shape[0], image.shape[1])
    for _ in range(4):
      sx = rng.randrange(0, image.shape[0] - edge + 1)
      sy = rng.randrange(0, image.shape[1] - edge + 1)
      crop = torch.from_numpy(np.ascontiguousarray(image[sx:sx + edge, sy:sy + edge])).permute(2, 0, 1)[None]
      patch = torch.nn.functional.adaptive_avg_pool2d(crop, (80, 80))[0].permute(1, 2, 0)
      for _ in range(4):
        ssx = rng.randrange(0, 80 - 64)
        ssy = rng.randrange(0, 80 - 64)
        patches.append(patch[ssx:ssx + 64, ssy:ssy + 64])
  if not patches:
    raise FileNotFoundError('no images in %s' % src)
  return torch.stack(patches).to(device)


def patch_windows(shapes, rng):
  """The draws of ``read_images`` for images of these (H, W), in its order: per image four times ``sx``, ``sy`` and
  then four times ``ssx``, ``ssy``.  Returns (the 4 F windows (image, y0, x0, edge) of ``_cabi.area_resize_ragged``,
  the 16 F records (src, oy, ox) of ``_cabi.patch_stats``: src is the row of the window)."""
  windows, records = [], []
  for i, (h, w) in enumerate(shapes):
    edge = min(h, w)
    for _ in range(4):
      sx = rng.randrange(0, h - edge + 1)
      sy = rng.randrange(0, w - edge + 1)
      src = len(windows)
      windows.append((i, sx, sy, edge))
      for _ in range(4):
        ssx = rng.randrange(0, MAIN_SIZE - PATCH_SIZE)
        ssy = rng.randrange(0, MAIN_SIZE - PATCH_SIZE)
        records.append((src, ssx, ssy))
  return windows, records


_CODE_TABLES = {}


def _code_table(device):
  """float32(k / 255.0) for the 256 codes: the reference's ``(imread / 255.0).astype(np.float32)``."""
  import numpy as np
  key = torch.device(device)
  if key not in _CODE_TABLES:
    _CODE_TABLES[key] = torch.from_numpy((np.arange(256) / 255.0).astype(np.float32)).to(key)
  return _CODE_TABLES[key]


def set_statistics(images_u8, rng=None, names=None):
  """The statistics of a set of 8-bit pictures on the device: ``images_u8`` is a list of contiguous device uint8
  (H_i, W_i, 3) tensors (``load_raw``'s 'srgb8' codes, or the ``picture=True`` outputs of ``retouch_batch``), ``rng`` a
  ``random.Random`` (default: the module-level generator, as the script).  Returns a device float32 (16 F, 3) tensor:
  what ``get_statistics(read_images(...))`` computes for the same files and generator state, with cv2's INTER_AREA in
  place of the rounded windows.  ``names`` (the files) only serve the error messages."""
  import numpy as np
  from . import _cabi
  from .datasets import plan_chunks
  rng = rng or random
  if not images_u8:
    raise ValueError('set_statistics needs at least one image')
  name = lambda i: names[i] if names else 'image %d' % i
  for i, x in enumerate(images_u8):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2] != 3:
      raise ValueError('%s: expected a uint8 (H, W, 3) tensor' % name(i))
    if min(x.shape[0], x.shape[1]) < MAIN_SIZE:
      raise ValueError('%s: %dx%d is smaller than %d on its short side (the metric would have to upscale it)' %
                       (name(i), x.shape[1], x.shape[0], MAIN_SIZE))
  dev = images_u8[0].device
  windows, records = patch_windows([tuple(x.shape[:2]) for x in images_u8], rng)
  stats = torch.empty((len(records), 3), dtype=torch.float32, device=dev)
  for lo, hi in plan_chunks([x.shape[0] * x.shape[1] * 12 for x in images_u8]):
    codes = images_u8[lo:hi]
    lin = [torch.empty(tuple(c.shape), dtype=torch.float32, device=dev) for c in codes]
    _cabi.decode_ragged(codes, _code_table(dev), 0, lin)
    wins = np.array(windows[4 * lo:4 * hi], dtype=np.int32) - np.array([lo, 0, 0, 0], dtype=np.int32)
    master = torch.empty((len(wins), MAIN_SIZE, MAIN_SIZE, 3), dtype=torch.float32, device=dev)
    _cabi.area_resize_ragged(lin, wins, MAIN_SIZE, master)
    rec = np.array(records[16 * lo:16 * hi], dtype=np.int32) - np.array([4 * lo, 0, 0], dtype=np.int32)
    _cabi.patch_stats(master, torch.from_numpy(rec).to(dev), PATCH_SIZE, stats[16 * lo:16 * hi])
  return stats


def score(stats_out, stats_target):
  """``histogram_intersection`` from two sets' statistics ((Q, 3) device float32, ``set_statistics``): two
  ``expo_stat_hist`` calls, then sum_k min(ca[k] / qa, cb[k] / qb) in float64 on the 2 x 96 counts.  Division is by the
  number of patches, dropped values included, as in ``calc_hist``.  -> (three intersections, their average)."""
  import numpy as np
  from . import _cabi
  fracs = []
  for st in (stats_out, stats_target):
    if st.shape[0] == 0:
      raise ValueError('score needs at least one patch per set')
    counts = torch.empty((3, HIST_BINS), dtype=torch.int32, device=st.device)
    _cabi.stat_hist(st, HIST_BINS, counts)
    fracs.append(counts.cpu().numpy().astype(np.float64) / float(st.shape[0]))
  ints = [float(v) for v in np.minimum(fracs[0], fracs[1]).sum(axis=1)]
  return ints, sum(ints) / len(ints)


def read_statistics(src, tag=None, rng=None, device='cuda:0'):
  """The file side of the device path: the files of ``src`` in sorted order (``tag`` filters as in ``read_images``),
  read as 8-bit codes (``evaluate.load_raw``), uploaded, -> ``set_statistics``.  A file that is not an 8-bit picture is
  refused: the reference's metric reads what ``cv2.imread`` gives, 8 bits per channel."""
  import warnings
  import numpy as np
  from .evaluate import load_raw
  names, codes = [], []
  for f in sorted(os.listdir(src)):
    if tag and f.find(tag) == -1:
      continue
    path = os.path.join(src, f)
    raw, kind = load_raw(path)
    if kind != 'srgb8':
      raise ValueError('%s: a %s file; the metric reads 8-bit pictures only' % (path, kind))
    names.append(path)
    codes.append(raw)
  if not codes:
    raise FileNotFoundError('no images in %s' % src)
  with warnings.catch_warnings():  # PIL's arrays are read-only: they are only read, by the upload
    warnings.simplefilter('ignore', UserWarning)
    dev_codes = [torch.from_numpy(np.ascontiguousarray(c)).to(device) for c in codes]
  return set_statistics(dev_codes, rng, names)


CLI_DEVICE = 'cuda:0'  # the device of --device (the host tests run it against CPU stand-ins)


def format_score(ints, avg):
  """The script's two lines."""
  return ('Hist. Inter.: %.2f%% %.2f%% %.2f%%' % (ints[0] * 100, ints[1] * 100, ints[2] * 100),
          '         Avg: %.2f%%' % (avg * 100))


def main(argv=None):
  """``python -m exposure_amd.metrics [--device [--seed N]] OUTPUT_DIR TARGET_DIR`` -- histogram_intersection.py:62-76.
  ``--device`` runs the device path (``read_statistics`` + ``score``); ``--seed`` seeds its patch draws."""
  import sys
  argv = sys.argv[1:] if argv is None else argv
  if '--device' in argv:
    import argparse
    ap = argparse.ArgumentParser(prog='python -m exposure_amd.metrics')
    ap.add_argument('--device', action='store_true')
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('output_dir')
    ap.add_argument('target_dir')
    args = ap.parse_args(argv)
    rng = random.Random(args.seed) if args.seed is not None else None
    so = read_statistics(args.output_dir, rng=rng, device=CLI_DEVICE)
    ints, avg = score(so, read_statistics(args.target_dir, rng=rng, device=CLI_DEVICE))
  else:
    if len(argv) != 2:
      raise SystemExit('usage: python -m exposure_amd.metrics [--device [--seed N]] OUTPUT_DIR TARGET_DIR')
    device = 'cuda:0' if torch.cuda.is_available() else 'cpu'
    ints, avg = histogram_intersection(read_images(argv[0], device=device), read_images(argv[1], device=device))
  for line in format_score(ints, avg):
    print(line)
  return ints, avg


if __name__ == '__main__':
  main()
