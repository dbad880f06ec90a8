"""Training sets from folders of photos: the reference's two preprocessing recipes, built on the device, and
:class:`PackProvider`, which serves them like :class:`~exposure_amd.replay_memory.ResidentProvider` and augments them
like the reference's ``DataProvider``.

``build_pack`` reads each file on the host as integer codes, uploads them, linearises them on the device
(``_cabi.decode_ragged`` with the recipe's float32 table) and resamples square windows of them with INTER_AREA
(``_cabi.area_resize_ragged``) into the MASTER pack:

* ``fivek`` (``fivek.py:26-70``, ``data_provider.py:59-78``; the input set of ``config_example.py``): 8- or 16-bit TIFFs,
  ``read_tiff16`` + ``linearize_ProPhotoRGB``; ``augmentation_factor`` random squares of side ``min(H, W)`` per image,
  each to ``main_size`` squared.  The master is ``[factor n][main][main][3]``; every draw of an epoch takes a random
  ``crop_size`` crop and a left-right flip with p = 0.5.
* ``folder`` (``folder_data_provider.py:8-45``, ``artist.py:14-73``; the target sets of ``config_example.py`` and
  ``config_sintel.py``): 8-bit images as ``cv2.imread`` loads them (PIL ``.convert('RGB')``), ``/ 255``; the centre
  square (``get_image_center``) to ``main_size`` squared, then ``augmentation_factor`` pre-cut copies, each flipped
  with p = 0.5 and cropped at random to ``crop_size``.  The master is ``[factor n][crop][crop][3]``; every draw flips
  with p = 0.5 (the crop is the identity).

Random draws come from ONE ``np.random.default_rng(seed)``, file by file in the sorted order.  Within an image:
``fivek`` draws ``(y0, x0)`` of each window in turn (``y0`` first); ``folder`` draws, for each copy in turn, the flip
(``random() < 0.5``), then the crop's row, then its column in the flipped image.  ``PackProvider`` has an RNG of its own:
per epoch a permutation of the master, then every row's crop row, crop column and flip, each as one vector.
"""
import json
import os

import numpy as np
import torch

from . import _cabi
from .replay_memory import ResidentProvider, _PinnedRing

RECIPES = ('fivek', 'folder')
MAX_IMAGES = 64          # images per chunk: one ragged decode / resize call
MAX_BYTES = 4 << 30      # decoded (float32) bytes per chunk: a 24 MP photo is 288 MB
PACK_FILE, MANIFEST_FILE = 'master.npy', 'manifest.json'
_TIFF = ('.tif', '.tiff')


class DatasetError(ValueError):
  pass


def recipe_table(recipe, bits):
  """The float32 linearisation of every code of a ``bits``-bit file: the reference's own NumPy expression evaluated on
  the code range."""
  if recipe == 'fivek':  # util.read_tiff16 then linearize_ProPhotoRGB
    return (np.arange(2**bits) * (1.0 / (2**bits - 1))).astype(np.float32)**1.8
  if recipe == 'folder':  # cv2.imread(...) / 255.0, .astype(np.float32)
    if bits != 8:
      raise DatasetError('the folder recipe reads 8-bit images only')
    return (np.arange(256) / 255.0).astype(np.float32)
  raise DatasetError('recipe must be one of %s, got %r' % (RECIPES, recipe))


def read_fold(path):
  """A fold file (``data/folds/*.txt``): one 1-based index into the sorted listing per line; ``#`` lines are ignored."""
  idx = []
  with open(path) as f:
    for line in f:
      line = line.strip()
      if line and not line.startswith('#'):
        idx.append(int(line))
  return idx


def list_files(folder, fold=None, read_limit=-1):
  """The files of ``folder`` sorted by name, narrowed to the 1-based indices of a fold file (kept in sorted order,
  ``artist.py:29-51``), then to the first ``read_limit``."""
  files = sorted(f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f)))
  if fold is not None:
    idx = sorted(set(read_fold(fold) if isinstance(fold, str) else fold))
    bad = [i for i in idx if not 1 <= i <= len(files)]
    if bad:
      raise DatasetError('%s: index %d outside the %d files of %s' % (fold, bad[0], len(files), folder))
    files = [files[i - 1] for i in idx]
  if read_limit is not None and read_limit >= 0:
    files = files[:read_limit]
  return [os.path.join(folder, f) for f in files]


def _png_bit_depth(path):
  with open(path, 'rb') as f:
    head = f.read(25)
  return head[24] if head[:8] == b'\x89PNG\r\n\x1a\n' and len(head) == 25 else None


def read_codes(path, recipe):
  """The integer codes of one file as the recipe reads it -> (H, W, C) uint8 / uint16."""
  if recipe == 'fivek':
    if not path.lower().endswith(_TIFF):
      raise DatasetError('%s: the fivek recipe reads TIFF files only' % path)
    from .tiff16 import read_tiff
    codes = read_tiff(path)
  elif recipe == 'folder' and path.lower().endswith(_TIFF):
    from .tiff16 import read_tiff  # (PIL would load a 16-bit RGB TIFF without saying so)
    codes = read_tiff(path)
    if codes.dtype != np.uint8:
      raise DatasetError('%s: a 16-bit file; the folder recipe reads 8-bit images only' % path)
  elif recipe == 'folder':
    from PIL import Image
    pil = Image.open(path)
    if pil.mode.startswith(('I', 'F')) or _png_bit_depth(path) == 16:
      raise DatasetError('%s: a 16-bit file; the folder recipe reads 8-bit images only' % path)
    codes = np.array(pil.convert('RGB'))  # (a writable copy: PIL's arrays are read-only)
  else:
    raise DatasetError('recipe must be one of %s, got %r' % (RECIPES, recipe))
  if codes.ndim == 2:
    codes = codes[:, :, None]
  return np.ascontiguousarray(codes)


class JpegFile(object):
  """The bytes of a baseline JPEG file and its plan (``jpeg_decode.parse``), standing in for the file's codes in a chunk
  of ``build_pack(..., device_jpeg=True)``: ``_flush`` decodes them on the device.  shape and dtype
  are those of the codes PIL would have made."""

  def __init__(self, path, data, plan):
    self.path, self.data, self.plan = path, data, plan
    self.shape, self.dtype = (plan.h, plan.w, 3), np.dtype(np.uint8)


def read_jpeg_file(path):
  """-> ``JpegFile`` of a ``.jpg`` / ``.jpeg`` path whose file the device decoder takes, else None (the PIL path)."""
  from . import jpeg_decode
  if not jpeg_decode.is_jpeg_path(path):
    return None
  with open(path, 'rb') as f:
    data = f.read()
  try:
    return JpegFile(path, data, jpeg_decode.parse(data))
  except jpeg_decode.UnsupportedJpeg:
    return None


def draw_windows(rng, recipe, h, w, main_size=80, crop_size=64, augmentation_factor=4):
  """One image's draws -> (windows [(y0, x0, side)], pre-cut records [(oy, ox, flip)] of the resized square or None)."""
  side = min(h, w)
  if recipe == 'fivek':
    wins = []
    for _ in range(augmentation_factor):
      y0 = int(rng.integers(0, h - side + 1))
      x0 = int(rng.integers(0, w - side + 1))
      wins.append((y0, x0, side))
    return wins, None
  wins = [((h - side) // 2, (w - side) // 2, side)]  # get_image_center
  cuts = []
  for _ in range(augmentation_factor):
    flip = bool(rng.random() < 0.5)
    sy = int(rng.integers(0, main_size - crop_size + 1))
    sx = int(rng.integers(0, main_size - crop_size + 1))
    # a crop at column sx of the FLIPPED square is the flip of the crop at main - crop - sx
    cuts.append((sy, main_size - crop_size - sx if flip else sx, int(flip)))
  return wins, cuts


def plan_chunks(nbytes, max_images=MAX_IMAGES, max_bytes=MAX_BYTES):
  """Consecutive chunks [lo, hi) of at most ``max_images`` images and ``max_bytes`` decoded bytes (an image larger
  than the budget is a chunk of its own) -- the rule ``build_pack`` applies as it reads."""
  chunks, lo, acc = [], 0, 0
  for i, b in enumerate(nbytes):
    if i > lo and (i - lo == max_images or acc + b > max_bytes):
      chunks.append((lo, i))
      lo, acc = i, 0
    acc += b
  if len(nbytes) > lo:
    chunks.append((lo, len(nbytes)))
  return chunks


def pack_shape(recipe, n, main_size=80, crop_size=64, augmentation_factor=4):
  s = main_size if recipe == 'fivek' else crop_size
  return (augmentation_factor * n, s, s, 3)


def _flush(chunk, recipe, master, row, dev, out_dtype, main_size, jpeg_sync='auto'):
  """Decode, resize (and for ``folder`` pre-cut) one chunk into master[row:]; -> the next row."""
  groups, on_device = {}, {}
  jpegs = [k for k, (codes, _wins, _cuts) in enumerate(chunk) if isinstance(codes, JpegFile)]
  if jpegs:  # the chunk's JPEG files in one call: their codes never visit the host
    from . import jpeg_decode
    made, _ = jpeg_decode.decode_jpeg_batch([chunk[k][0].data for k in jpegs], dev, plans=[chunk[k][0].plan for k in jpegs],
                                            names=[chunk[k][0].path for k in jpegs], sync=jpeg_sync)
    on_device = dict(zip(jpegs, made))
  for k, (codes, _wins, _cuts) in enumerate(chunk):
    groups.setdefault((codes.dtype.itemsize * 8, codes.shape[2]), []).append(k)
  lin = [None] * len(chunk)
  for (bits, _c), idx in groups.items():
    cs = [on_device[k] if k in on_device else torch.from_numpy(chunk[k][0]).to(dev) for k in idx]
    ys = [torch.empty((c.shape[0], c.shape[1], 3), dtype=torch.float32, device=dev) for c in cs]
    _cabi.decode_ragged(cs, torch.from_numpy(recipe_table(recipe, bits)).to(dev), 0, ys)
    for k, y in zip(idx, ys):
      lin[k] = y
  windows = [(k,) + wdw for k, (_codes, wins, _cuts) in enumerate(chunk) for wdw in wins]
  if recipe == 'fivek':
    out = master[row:row + len(windows)]
    _cabi.area_resize_ragged(lin, windows, main_size, out)
    return row + len(windows)
  squares = torch.empty((len(chunk), main_size, main_size, 3), dtype=out_dtype, device=dev)
  _cabi.area_resize_ragged(lin, windows, main_size, squares)
  rec = np.array([(k,) + cut for k, (_codes, _wins, cuts) in enumerate(chunk) for cut in cuts], dtype=np.int32)
  out = master[row:row + len(rec)]
  _cabi.pack_recut(squares, torch.from_numpy(rec).to(dev), out)
  return row + len(rec)


def build_pack(paths, recipe, out_dtype, device, seed, main_size=80, crop_size=64, augmentation_factor=4,
               max_images=MAX_IMAGES, max_bytes=MAX_BYTES, timings=None, device_jpeg=False, jpeg_sync='auto'):
  """The master pack of ``paths`` (in this order) under ``recipe`` as a device tensor of ``out_dtype``.  Files are read
  one by one and processed in chunks (``plan_chunks``).  ``timings``: a dict that receives the seconds spent reading
  files ('read') and in the rest ('device', synchronised).  ``device_jpeg`` (the ``folder`` recipe): a baseline JPEG
  file is read as bytes and parsed only ('read' is then the file reads plus parsing), and every chunk's JPEGs are
  decoded on the device in one call; the sizes come from the header, so the same random numbers are drawn and the
  pack is bit for bit the host-decode pack.  ``jpeg_sync`` is ``decode_jpeg_batch``'s ``sync`` (False: the one-lane
  entropy walk for files without restart markers, for comparison runs; the pack is the same)."""
  import time
  if recipe not in RECIPES:
    raise DatasetError('recipe must be one of %s, got %r' % (RECIPES, recipe))
  if not 1 <= crop_size <= main_size:
    raise DatasetError('1 <= crop_size <= main_size required')
  dev = torch.device(device)
  rng = np.random.default_rng(seed)
  master = torch.empty(pack_shape(recipe, len(paths), main_size, crop_size, augmentation_factor), dtype=out_dtype,
                       device=dev)
  t_read = t_dev = 0.0
  chunk, acc, row = [], 0, 0
  for path in paths:
    t0 = time.perf_counter()
    codes = read_jpeg_file(path) if device_jpeg and recipe == 'folder' else None
    if codes is None:
      codes = read_codes(path, recipe)
    t_read += time.perf_counter() - t0
    h, w = codes.shape[:2]
    if min(h, w) < main_size:
      raise DatasetError('%s: %d x %d, shorter side below main_size %d' % (path, h, w, main_size))
    b = h * w * 12
    if chunk and (len(chunk) == max_images or acc + b > max_bytes):
      t0 = time.perf_counter()
      row = _flush(chunk, recipe, master, row, dev, out_dtype, main_size, jpeg_sync)
      t_dev += time.perf_counter() - t0
      chunk, acc = [], 0
    wins, cuts = draw_windows(rng, recipe, h, w, main_size, crop_size, augmentation_factor)
    chunk.append((codes, wins, cuts))
    acc += b
  t0 = time.perf_counter()
  if chunk:
    row = _flush(chunk, recipe, master, row, dev, out_dtype, main_size, jpeg_sync)
  if dev.type == 'cuda':
    torch.cuda.synchronize(dev)
  t_dev += time.perf_counter() - t0
  assert row == master.shape[0]
  if timings is not None:
    timings['read'], timings['device'] = t_read, t_dev
  return master


# ---- the cache (the reference keeps image_raw.npy for the same reason) ---------------------------------------------------
def manifest(paths, recipe, out_dtype, seed, main_size=80, crop_size=64, augmentation_factor=4):
  """What a cached pack was built from: a pack whose manifest differs from this one is rebuilt."""
  files = []
  for p in paths:
    st = os.stat(p)
    files.append([os.path.abspath(p), int(st.st_size), int(st.st_mtime_ns)])
  return dict(version=1, recipe=recipe, dtype=str(out_dtype).replace('torch.', ''), seed=int(seed),
              main_size=int(main_size), crop_size=int(crop_size), augmentation_factor=int(augmentation_factor),
              files=files)


def save_pack(folder, master, man):
  """master.npy, then manifest.json (a build interrupted between the two leaves no valid manifest behind)."""
  os.makedirs(folder, exist_ok=True)
  mpath = os.path.join(folder, MANIFEST_FILE)
  if os.path.exists(mpath):
    os.remove(mpath)
  np.save(os.path.join(folder, PACK_FILE), master.detach().cpu().numpy())
  with open(mpath + '.tmp', 'w') as f:
    json.dump(man, f)
  os.replace(mpath + '.tmp', mpath)


def load_pack(folder):
  """-> (master as a NumPy array, manifest), or None when the folder holds no complete pack."""
  mpath, ppath = os.path.join(folder, MANIFEST_FILE), os.path.join(folder, PACK_FILE)
  if not (os.path.exists(mpath) and os.path.exists(ppath)):
    return None
  with open(mpath) as f:
    man = json.load(f)
  return np.load(ppath), man


def cached_pack(folder, recipe, out_dtype, device, seed, fold=None, read_limit=-1, cache=None, device_jpeg=False,
                jpeg_sync='auto', **sizes):
  """``build_pack`` of a folder's selection, through the cache directory ``cache`` when given -> (master, hit).
  ``device_jpeg`` and ``jpeg_sync`` are ``build_pack``'s; the pack is the same either way, so they are no part of the
  manifest."""
  paths = list_files(folder, fold, read_limit)
  if not paths:
    raise DatasetError('%s: no files selected' % folder)
  man = manifest(paths, recipe, out_dtype, seed, **sizes)
  if cache is not None:
    got = load_pack(cache)
    if got is not None and got[1] == man:
      return torch.from_numpy(got[0]).to(device), True
  master = build_pack(paths, recipe, out_dtype, device, seed, device_jpeg=device_jpeg, jpeg_sync=jpeg_sync, **sizes)
  if cache is not None:
    save_pack(cache, master, man)
  return master, False


# ---- the provider --------------------------------------------------------------------------------------------------------
class PackProvider(ResidentProvider):
  """A master pack served like ``ResidentProvider`` (consecutive rows of ``images``, epoch after epoch; the unread tail
  of an epoch is skipped) and augmented like ``DataProvider`` (a shuffled epoch; every row a crop of ``crop_size`` and a
  left-right flip with p = 0.5).

  ``images`` holds two halves of ``count`` rows (``count`` = the master's length).  At every epoch wrap ``next_rows``
  draws the new epoch (permutation, crops, flips) from the provider's host RNG, re-cuts it into the IDLE half with
  ``expo_pack_recut`` on the current stream, and serves rows of that half.  Rows handed out before the wrap stay
  intact until the NEXT wrap, and work enqueued earlier is ordered before the re-cut by the stream; the storage never
  moves.  ``ReplayMemory.plan_iteration`` plans an iteration ahead only while one epoch covers one plan's consumption
  (so no plan wraps twice).  ``features`` is the row index, as in ``ResidentProvider``."""

  def __init__(self, master, crop_size=64, seed=0):
    if master.dim() != 4 or master.shape[1] != master.shape[2] or master.shape[3] != 3:
      raise DatasetError('master must be (M, S, S, 3), got %s' % (tuple(master.shape),))
    if not 1 <= crop_size <= master.shape[1]:
      raise DatasetError('1 <= crop_size <= %d required' % master.shape[1])
    self.master = master.contiguous()
    self.device, self.dtype = master.device, master.dtype
    self.count, self.size, self.main = int(master.shape[0]), int(crop_size), int(master.shape[1])
    self.rng = np.random.default_rng(seed)
    self.images = torch.empty((2 * self.count, self.size, self.size, 3), dtype=self.dtype, device=self.device)
    self.features = torch.arange(2 * self.count, device=self.device, dtype=torch.float32)
    self._ring = _PinnedRing(self.device, slots=2)
    self.epochs, self.half, self.at = 0, 1, 0
    self._recut()

  def draw_epoch(self):
    """The next epoch's (src, oy, ox, flip) records, int32 (count, 4), from the host RNG."""
    m, span = self.count, self.main - self.size + 1
    perm = self.rng.permutation(m)
    oy = self.rng.integers(0, span, size=m)
    ox = self.rng.integers(0, span, size=m)
    flip = self.rng.random(m) < 0.5
    return np.stack([perm, oy, ox, flip.astype(np.int64)], axis=1).astype(np.int32)

  def _recut(self):
    if self.images.is_cuda and torch.cuda.is_current_stream_capturing():
      raise RuntimeError('PackProvider: an epoch wrap during a stream capture (the re-cut is not part of any graph)')
    rec = self._ring.put(torch.from_numpy(self.draw_epoch()))
    self.half = 1 - self.half
    lo = self.half * self.count
    _cabi.pack_recut(self.master, rec, self.images[lo:lo + self.count])
    self.epochs += 1
    self.at = 0

  def next_rows(self, batch_size):
    """The first row of the next batch (the batch is ``images[lo:lo + batch_size]``); re-cuts at an epoch wrap."""
    assert batch_size <= self.count
    if self.at + batch_size > self.count:
      self._recut()
    lo = self.half * self.count + self.at
    self.at += batch_size
    return lo
