"""CPU: the host half of the photo training sets -- the float64 INTER_AREA restatement pinned by
hand-worked cases, file selection and fold lists, the recipes' tables against the reference's expressions, the draws,
chunking, refusals, the cache manifest, PackProvider's epoch walk, plan_iteration's fallback and the CLI's argument
checks.  The three library calls run on NumPy stand-ins (tests/_area_ref.py); tests/test_hip_datasets.py runs them on
the GPU."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import datasets, train
from exposure_amd.config import make_cfg
from exposure_amd.replay_memory import ReplayMemory, ResidentProvider
from exposure_amd.tiff16 import write_tiff
from tests import _area_ref as ref


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_five_to_two_by_hand():
  x = np.array([1.0, 10.0, 100.0, 1000.0, 10000.0])
  a = ref.area_matrix(5, 2)
  assert np.allclose(a @ x, [(x[0] + x[1] + 0.5 * x[2]) / 2.5, (0.5 * x[2] + x[3] + x[4]) / 2.5], rtol=0, atol=1e-12)
  img = np.broadcast_to(x[:, None, None], (5, 5, 1)) * np.broadcast_to(x[None, :, None], (5, 5, 1))
  assert np.allclose(ref.area_resize(img, 2)[:, :, 0], np.outer(a @ x, a @ x), rtol=1e-15)


@pytest.mark.parametrize('side,S', [(160, 80), (192, 64), (240, 80), (7, 1)])
def test_integer_ratios_are_box_means(side, S):
  k = side // S
  img = np.random.default_rng(side).random((side, side, 3))
  want = img.reshape(S, k, S, k, 3).mean(axis=(1, 3))
  assert np.abs(ref.area_resize(img, S) - want).max() < 1e-14


def test_equal_sides_are_the_identity():
  img = np.random.default_rng(0).random((80, 80, 3))
  assert np.array_equal(ref.area_resize(img, 80), img)
  assert np.array_equal(ref.area_matrix(64, 64), np.eye(64))


def test_the_thresholds():
  # 2001 -> 2000 (scale 1.0005): output 0 covers [0, 1.0005); its tail of 0.0005 in source 1 is below 1e-3: dropped
  assert ref.axis_weights(0, 2001 / 2000, 2001) == [(0, 1 / 1.0005)]
  # 1002 -> 1000 (scale 1.002): the tail of 0.002 is above it: kept, as is output 1's head of 0.998 in source 1
  w = ref.axis_weights(0, 1002 / 1000, 1002)
  assert [s for s, _ in w] == [0, 1] and w[1][1] == pytest.approx(0.002 / 1.002)
  w = ref.axis_weights(1, 1002 / 1000, 1002)
  assert [s for s, _ in w] == [1, 2] and w[0][1] == pytest.approx(0.998 / 1.002)
  # 3999 -> 2000 (scale 1.9995): output 1 starts 0.0005 before source 2: no head in source 1
  w = ref.axis_weights(1, 3999 / 2000, 3999)
  assert w[0][0] == 2 and w[0][1] == pytest.approx(1 / 1.9995)
  # 5 -> 2: partial weights on both sides of the shared source 2
  assert ref.axis_weights(1, 2.5, 5) == [(2, 0.2), (3, 0.4), (4, 0.4)]
  # every row of the matrix sums to 1 (the dropped slivers are what cv2 drops, so up to 1e-3 / cell)
  for side, S in ((97, 80), (239, 64), (1000, 80), (4001, 80), (81, 80)):
    assert np.abs(ref.area_matrix(side, S).sum(axis=1) - 1).max() < 1e-3


def sweep_sides(S):
  """Sides around the first second tile of S = 64 / 80 (4095) and about 200 more up to 65535, odd strides."""
  return sorted(set(range(4090, 4111)) | set(range(4111, 65536, 307)) | {S * 4094 // 64, 8188, 8191, 8192, 65535})


def test_tile_plans_fit_the_lds_tile_and_the_seam_cases_are_multi_tile():
  """area_resize_kernel trusts that a tile's source span fits its LDS buffer (``min(c1 - c0, kTileCols)`` must never
  truncate) and the device tests of the seams trust the tile counts pinned here: a change of kTileCols or of
  tile_out_cols shows up on the CPU, not as device cases that silently became single-tile."""
  cases = [(S, side) for S in (64, 80) for side in sweep_sides(S)]
  cases += [(1, 1), (1, 97), (1, 4094), (7, 7), (7, 4095), (7, 28657), (7, 28658), (256, 256), (256, 4095), (256, 4097),
            (256, 20001), (256, 65535)]
  for S, side in cases:
    plan = ref.tile_plan(side, S)
    assert plan[0][0] == 0 and plan[-1][1] == S and all(a[1] == b[0] for a, b in zip(plan, plan[1:])), (S, side)
    for ox0, ox1, c0, c1 in plan:
      assert ox1 > ox0 and 0 <= c0 < c1 <= side and c1 - c0 <= 4096, (S, side, ox0, ox1, c0, c1)
    if side <= 4094:
      assert len(plan) == 1, (S, side)
  with pytest.raises(AssertionError):
    ref.tile_plan(4095, 1)  # no output column fits a tile: expo_area_resize_ragged refuses such a window
  for (S, side), widths in ref.SEAM_PLANS.items():
    assert [ox1 - ox0 for ox0, ox1, _, _ in ref.tile_plan(side, S)] == widths, (S, side)
  # the sides of tests/test_hip_datasets.py::sides() are all single-tile: the seams were untested before these cases
  for S in (64, 80):
    assert all(len(ref.tile_plan(side, S)) == 1 for side in (S, S + 1, 97, 2 * S, 239, 1000, 4001))


def test_the_bound_rejects_a_shifted_and_a_dropped_second_tile():
  """What a wrong seam would look like, through the comparison of the device tests (``ref.max_err`` against
  ``ref.BOUND``), for side 6000 / S 64 (tiles of 43 and 21 output columns): the second tile read from source columns
  one to the left (a ``c - c0`` off by one), and the second tile never written."""
  side, S = 6000, 64
  (_, split, _, _), (ox0, ox1, _, _) = ref.tile_plan(side, S)
  assert (split, ox0, ox1) == (43, 43, 64)
  img = np.random.default_rng(6000).random((side, side, 1), dtype=np.float32).astype(np.float64)
  a = ref.area_matrix(side, S)
  want = ref.area_resize(img, S)
  assert ref.max_err(ref.area_resize(img, S, cols=a), want)[0] == 0.0
  assert ref.max_err(want.astype(np.float32), want)[0] <= ref.BOUND  # the store's rounding alone is inside it
  shifted = a.copy()
  shifted[ox0:, :-1] = a[ox0:, 1:]  # output column ox reads source column c - 1 where it should read c
  shifted[ox0:, -1] = 0.0
  err, at = ref.max_err(ref.area_resize(img, S, cols=shifted), want)
  assert err > 100 * ref.BOUND and at[1] >= ox0, (err, at)
  dropped = want.copy()
  dropped[:, ox0:] = 0.0
  err, at = ref.max_err(dropped, want)
  assert err > 100 * ref.BOUND and at[1] >= ox0, (err, at)


# ---- files, folds, tables ----------------------------------------------------------------------------------------------------
def test_files_are_sorted_and_folds_are_one_based(tmp_path):
  for name in ('c.png', 'a.png', 'b.png', 'd.png'):
    (tmp_path / name).write_bytes(b'')
  (tmp_path / 'sub').mkdir()
  names = lambda ps: [os.path.basename(p) for p in ps]
  assert names(datasets.list_files(str(tmp_path))) == ['a.png', 'b.png', 'c.png', 'd.png']
  fold = tmp_path.parent / ('%s_fold.txt' % tmp_path.name)
  fold.write_text('# Note: this list is 1-based, i.e. ids are among [1, 5000]\n4\n2\n\n')
  assert datasets.read_fold(str(fold)) == [4, 2]
  assert names(datasets.list_files(str(tmp_path), str(fold))) == ['b.png', 'd.png']
  assert names(datasets.list_files(str(tmp_path), str(fold), read_limit=1)) == ['b.png']
  assert names(datasets.list_files(str(tmp_path), read_limit=3)) == ['a.png', 'b.png', 'c.png']
  fold.write_text('5\n')
  with pytest.raises(datasets.DatasetError, match='index 5'):
    datasets.list_files(str(tmp_path), str(fold))


def test_recipe_tables_are_the_reference_expressions_bit_for_bit():
  for d in (8, 16):
    raw = np.arange(2**d, dtype=np.uint16 if d == 16 else np.uint8)
    want = np.power((raw * (1.0 / (2**d - 1))).astype(np.float32), 1.8)  # read_tiff16 + linearize_ProPhotoRGB
    got = datasets.recipe_table('fivek', d)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
  want = (np.arange(256, dtype=np.uint8)[:, None, None] / 255.0).astype(np.float32).ravel()  # cv2.imread / 255.0
  got = datasets.recipe_table('folder', 8)
  assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
  with pytest.raises(datasets.DatasetError):
    datasets.recipe_table('folder', 16)
  with pytest.raises(datasets.DatasetError):
    datasets.recipe_table('bnw', 8)


def test_window_and_crop_draws_per_seed():
  rng = np.random.default_rng(5)
  wins, cuts = datasets.draw_windows(rng, 'fivek', 120, 200)
  r = np.random.default_rng(5)
  assert cuts is None and wins == [(int(r.integers(0, 1)), int(r.integers(0, 81)), 120) for _ in range(4)]
  wins, cuts = datasets.draw_windows(np.random.default_rng(7), 'folder', 300, 200)
  assert wins == [(50, 0, 200)]
  r = np.random.default_rng(7)
  for oy, ox, flip in cuts:
    f = r.random() < 0.5
    sy, sx = int(r.integers(0, 17)), int(r.integers(0, 17))
    assert (oy, ox, flip) == (sy, 16 - sx if f else sx, int(f))
  # the crop of the flipped square at column sx is what the record cuts
  sq = np.random.default_rng(1).random((80, 80, 3))
  for oy, ox, flip in cuts:
    flipped = sq[:, ::-1]
    sx = 16 - ox if flip else ox
    want = (flipped if flip else sq)[oy:oy + 64, sx:sx + 64]
    assert np.array_equal(ref.recut(sq[None], [(0, oy, ox, flip, 64)])[0], want)
  a = datasets.draw_windows(np.random.default_rng(3), 'fivek', 90, 95)
  assert a == datasets.draw_windows(np.random.default_rng(3), 'fivek', 90, 95)


def test_chunking_by_count_and_bytes():
  assert datasets.plan_chunks([1] * 130) == [(0, 64), (64, 128), (128, 130)]
  assert datasets.plan_chunks([3, 3, 3, 3], max_bytes=7) == [(0, 2), (2, 4)]
  assert datasets.plan_chunks([10, 1, 1], max_bytes=7) == [(0, 1), (1, 3)]  # too big for the budget: a chunk alone
  assert datasets.plan_chunks([1, 10, 1], max_bytes=7) == [(0, 1), (1, 2), (2, 3)]
  assert datasets.plan_chunks([]) == []


def write_fivek(folder, sizes, seed=0, bits=16):
  os.makedirs(folder, exist_ok=True)
  rng = np.random.default_rng(seed)
  for k, (h, w) in enumerate(sizes):
    hi, dt = (65536, np.uint16) if bits == 16 else (256, np.uint8)
    write_tiff(os.path.join(folder, 'img%03d.tif' % k), rng.integers(0, hi, (h, w, 3), dtype=dt))
  return sorted(os.path.join(folder, f) for f in os.listdir(folder))


def write_pngs(folder, sizes, seed=0):
  from PIL import Image
  os.makedirs(folder, exist_ok=True)
  rng = np.random.default_rng(seed)
  for k, (h, w) in enumerate(sizes):
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, 'img%03d.png' % k))
  return sorted(os.path.join(folder, f) for f in os.listdir(folder))


class Spy:
  """Records the images per resize call (the chunks build_pack makes)."""

  def __init__(self):
    self.calls = []

  def __call__(self, xs, windows, S, out):
    self.calls.append(len(xs))
    return ref.area_resize_ragged(xs, windows, S, out)


def test_build_pack_on_the_stand_in(tmp_path, monkeypatch):
  ref.patch(monkeypatch)
  spy = Spy()
  monkeypatch.setattr(datasets._cabi, 'area_resize_ragged', spy)
  paths = write_fivek(str(tmp_path / 'f'), [(90, 120), (130, 81), (80, 80)])
  pack = datasets.build_pack(paths, 'fivek', torch.float32, 'cpu', seed=4, max_images=2)
  assert tuple(pack.shape) == (12, 80, 80, 3) and spy.calls == [2, 1]
  # the windows of the stand-in build are the documented draws, in file order, from one generator
  rng = np.random.default_rng(4)
  from exposure_amd.tiff16 import read_tiff
  for k, p in enumerate(paths):
    img = read_tiff(p)
    lin = datasets.recipe_table('fivek', 16)[img].astype(np.float64)
    wins, _ = datasets.draw_windows(rng, 'fivek', img.shape[0], img.shape[1])
    for j, (y0, x0, s) in enumerate(wins):
      want = ref.area_resize(lin[y0:y0 + s, x0:x0 + s], 80).astype(np.float32)
      assert np.array_equal(pack[4 * k + j].numpy(), want)
  # by bytes: an image per chunk when the budget holds one
  spy.calls.clear()
  pack2 = datasets.build_pack(paths, 'fivek', torch.float32, 'cpu', seed=4, max_bytes=130 * 81 * 12)
  assert spy.calls == [1, 1, 1] and torch.equal(pack, pack2)
  # the folder recipe: centre squares, pre-cut
  paths = write_pngs(str(tmp_path / 'r'), [(100, 90), (81, 140)])
  pack = datasets.build_pack(paths, 'folder', torch.float16, 'cpu', seed=2)
  assert tuple(pack.shape) == (8, 64, 64, 3) and pack.dtype == torch.float16
  rng = np.random.default_rng(2)
  from PIL import Image
  for k, p in enumerate(paths):
    img = np.asarray(Image.open(p).convert('RGB'))
    lin = datasets.recipe_table('folder', 8)[img].astype(np.float64)
    wins, cuts = datasets.draw_windows(rng, 'folder', img.shape[0], img.shape[1])
    (y0, x0, s), = wins
    sq = ref.area_resize(lin[y0:y0 + s, x0:x0 + s], 80).astype(np.float32)
    for j, (oy, ox, flip) in enumerate(cuts):
      want = ref.recut(sq[None], [(0, oy, ox, flip, 64)])[0]
      assert np.array_equal(pack[4 * k + j].numpy(), torch.from_numpy(np.ascontiguousarray(want)).half().numpy())


def test_refusals_name_the_file(tmp_path, monkeypatch):
  ref.patch(monkeypatch)
  small = write_fivek(str(tmp_path / 'small'), [(79, 200)])
  with pytest.raises(datasets.DatasetError, match='img000.tif.*shorter side'):
    datasets.build_pack(small, 'fivek', torch.float32, 'cpu', seed=0)
  pngs = write_pngs(str(tmp_path / 'png'), [(90, 90)])
  with pytest.raises(datasets.DatasetError, match='img000.png.*TIFF'):
    datasets.build_pack(pngs, 'fivek', torch.float32, 'cpu', seed=0)
  from PIL import Image
  p16 = str(tmp_path / 'deep.png')
  Image.fromarray(np.full((90, 90), 40000, dtype=np.uint16)).save(p16)
  with pytest.raises(datasets.DatasetError, match='deep.png.*16-bit'):
    datasets.build_pack([p16], 'folder', torch.float32, 'cpu', seed=0)
  t16 = write_fivek(str(tmp_path / 't16'), [(90, 90)])
  with pytest.raises(datasets.DatasetError, match='img000.tif.*16-bit'):
    datasets.build_pack(t16, 'folder', torch.float32, 'cpu', seed=0)
  with pytest.raises(datasets.DatasetError, match='recipe'):
    datasets.build_pack(t16, 'bnw', torch.float32, 'cpu', seed=0)


def test_cache_manifest_invalidates_when_a_file_changes(tmp_path, monkeypatch):
  ref.patch(monkeypatch)
  folder = str(tmp_path / 'f')
  paths = write_fivek(folder, [(90, 100), (85, 85)])
  cache = str(tmp_path / 'cache')
  a, hit = datasets.cached_pack(folder, 'fivek', torch.float32, 'cpu', 3, cache=cache)
  assert not hit and os.path.exists(os.path.join(cache, datasets.MANIFEST_FILE))
  b, hit = datasets.cached_pack(folder, 'fivek', torch.float32, 'cpu', 3, cache=cache)
  assert hit and torch.equal(a, b)
  master, man = datasets.load_pack(cache)
  assert man['recipe'] == 'fivek' and man['seed'] == 3 and man['main_size'] == 80 and len(man['files']) == 2
  assert np.array_equal(master, a.numpy())
  # another seed, dtype or selection is another pack
  _, hit = datasets.cached_pack(folder, 'fivek', torch.float32, 'cpu', 4, cache=cache)
  assert not hit
  _, hit = datasets.cached_pack(folder, 'fivek', torch.float32, 'cpu', 4, cache=cache)
  assert hit
  _, hit = datasets.cached_pack(folder, 'fivek', torch.float16, 'cpu', 4, cache=cache)
  assert not hit
  _, hit = datasets.cached_pack(folder, 'fivek', torch.float16, 'cpu', 4, cache=cache, read_limit=1)
  assert not hit
  # a file rewritten in place (new contents, new mtime)
  _, hit = datasets.cached_pack(folder, 'fivek', torch.float32, 'cpu', 3, cache=cache)
  assert not hit
  write_fivek(folder, [(90, 100)], seed=11)
  st = os.stat(paths[0])
  os.utime(paths[0], ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))
  c, hit = datasets.cached_pack(folder, 'fivek', torch.float32, 'cpu', 3, cache=cache)
  assert not hit and not torch.equal(c, a)
  # a pack without its manifest is no pack
  os.remove(os.path.join(cache, datasets.MANIFEST_FILE))
  assert datasets.load_pack(cache) is None


# ---- PackProvider ---------------------------------------------------------------------------------------------------------
def master_of(m, S, seed=0):
  return torch.from_numpy(np.random.default_rng(seed).random((m, S, S, 3), dtype=np.float32))


def test_pack_provider_epoch_walk_halves_and_permutation(monkeypatch):
  ref.patch(monkeypatch)
  master = master_of(10, 80)
  p = datasets.PackProvider(master, crop_size=64, seed=7)
  assert isinstance(p, ResidentProvider) and p.count == 10 and tuple(p.images.shape) == (20, 64, 64, 3)
  assert tuple(p.features.shape) == (20,)
  rng = np.random.default_rng(7)

  def epoch():
    perm = rng.permutation(10)
    oy, ox = rng.integers(0, 17, size=10), rng.integers(0, 17, size=10)
    flip = rng.random(10) < 0.5
    return ref.recut(master.numpy(), list(zip(perm, oy, ox, flip, [64] * 10)))

  first = epoch()
  assert np.array_equal(p.images[:10].numpy(), first) and p.epochs == 1
  assert [p.next_rows(4), p.next_rows(4)] == [0, 4]
  # the unread tail (rows 8, 9) is skipped: the wrap re-cuts the idle half and serves it; the old half is intact
  lo = p.next_rows(4)
  second = epoch()
  assert lo == 10 and p.epochs == 2 and np.array_equal(p.images[10:].numpy(), second)
  assert np.array_equal(p.images[:10].numpy(), first)
  x, f = p.get_next_batch(4)
  assert torch.equal(x, p.images[14:18]) and torch.equal(f, p.features[14:18])
  assert p.next_rows(4) == 0 and p.epochs == 3 and np.array_equal(p.images[:10].numpy(), epoch())
  assert np.array_equal(p.images[10:].numpy(), second)
  # every master row once per epoch
  assert sorted(np.random.default_rng(0).permutation(10)) == list(range(10))
  with pytest.raises(AssertionError):
    p.next_rows(11)
  # folder packs: the crop is the identity, only flips
  q = datasets.PackProvider(master_of(6, 64), crop_size=64, seed=1)
  for r in range(6):
    row = q.images[r].numpy()
    assert any(np.array_equal(row, m) or np.array_equal(row, m[:, ::-1]) for m in master_of(6, 64).numpy())


def cfg_small():
  cfg = make_cfg()
  cfg.batch_size, cfg.replay_memory_size, cfg.citers = 8, 24, 2
  return cfg


@pytest.mark.parametrize('fake_rows,real_rows,planned', [(24, 24, True), (23, 24, False), (24, 23, False), (200, 30, True)])
def test_plan_iteration_falls_back_when_an_epoch_is_shorter_than_a_plan(monkeypatch, fake_rows, real_rows, planned):
  """fake: the refill takes up to ceil(pool / batch) whole batches (24 rows); real: (1 + citers) batches (24 rows)."""
  ref.patch(monkeypatch)
  cfg = cfg_small()
  fd = datasets.PackProvider(master_of(fake_rows, 80), seed=1)
  rd = datasets.PackProvider(master_of(real_rows, 64), seed=2)
  mem = ReplayMemory(cfg, fd, rd, seed=0)
  mem._h_stopped[mem._order[:4]] = 1  # terminated records for the critic replays
  at = (fd.at, rd.at, fd.epochs, rd.epochs)
  plan = mem.plan_iteration(cfg.batch_size, cfg.citers)
  assert (plan is not None) == planned
  if plan is None:
    assert (fd.at, rd.at, fd.epochs, rd.epochs) == at  # nothing consumed


def test_train_cli_argument_checks(tmp_path):
  d = str(tmp_path)
  with pytest.raises(SystemExit):
    train.parse_args(['--fake-dir', d])
  with pytest.raises(SystemExit):
    train.parse_args(['--real-dir', d])
  with pytest.raises(SystemExit):
    train.parse_args(['--pack-cache', d])
  with pytest.raises(SystemExit):
    train.parse_args(['--fake-list', d])
  with pytest.raises(SystemExit):
    train.parse_args(['--read-limit', '3'])
  with pytest.raises(SystemExit):
    train.parse_args(['--fake-dir', d, '--real-dir', str(tmp_path / 'missing')])
  with pytest.raises(SystemExit):
    train.parse_args(['--fake-dir', d, '--real-dir', d, '--fake-recipe', 'bnw'])
  with pytest.raises(SystemExit):
    train.parse_args(['--fake-dir', d, '--real-dir', d, '--fake-list', str(tmp_path / 'missing.txt')])
  a = train.parse_args(['--fake-dir', d, '--real-dir', d, '--read-limit', '5', '--pack-cache', d])
  assert (a.fake_recipe, a.real_recipe, a.read_limit, a.pack_cache) == ('fivek', 'folder', 5, d)
  a = train.parse_args([])
  assert a.fake_dir is None and a.real_dir is None  # the synthetic run of before
