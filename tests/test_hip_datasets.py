"""GPU: the training sets of folders of photos: expo_area_resize_ragged against the float64
INTER_AREA restatement, expo_pack_recut against NumPy indexing, build_pack against its CPU stand-in build, PackProviders
through the iteration graph against the step-by-step calls, and the training CLI on generated folders.  The host half is
tests/test_datasets_host.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exposure_amd import _cabi, datasets
from exposure_amd.config import make_cfg
from exposure_amd.gan import GAN
from exposure_amd.tiff16 import write_tiff
from tests import _area_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
BOUND = ref.BOUND  # 4e-6: |out - float64| for fp32 output on inputs in [0, 1]


def sides(S):
  return (S, S + 1, 97, 2 * S, 239, 1000, 4001)


def make_case(rng, S, in_dtype):
  """Images (device) and windows: one image per side of the list (odd offsets), then enough windows of 97 on one more
  image that the call holds more than 64 windows.  -> (xs, host float64 images, windows)"""
  xs, hosts, wins = [], [], []
  for k, side in enumerate(sides(S)):
    h, w = side + 3, side + 2
    img = torch.from_numpy(rng.random((h, w, 3), dtype=np.float32)).to(in_dtype)
    hosts.append(img.double().numpy())
    xs.append(img.to(DEV))
    wins.append((k, 1 + 2 * (k % 2), 1 + (k % 2), side))
  img = torch.from_numpy(rng.random((131, 129, 3), dtype=np.float32)).to(in_dtype)
  hosts.append(img.double().numpy())
  xs.append(img.to(DEV))
  for j in range(60):
    wins.append((len(xs) - 1, (7 * j) % 35, (11 * j + 1) % 33, 97 - (j % 2) * 7))
  return xs, hosts, wins


def reference(hosts, wins, S):
  return np.stack([ref.area_resize(hosts[i][y0:y0 + s, x0:x0 + s], S) for i, y0, x0, s in wins])


def resize(xs, wins, S, dtype):
  """One call into the middle of a guarded buffer; the guard rows must come back untouched."""
  buf = torch.full((len(wins) + 2, S, S, 3), 7.0, dtype=dtype, device=DEV)
  _cabi.area_resize_ragged(xs, wins, S, buf[1:-1])
  torch.cuda.synchronize()
  assert bool((buf[0] == 7).all()) and bool((buf[-1] == 7).all()), 'a write outside the output'
  return buf[1:-1].clone()


@pytest.mark.parametrize('S', [80, 64])
@pytest.mark.parametrize('in_dtype', [torch.float32, torch.float16])
def test_area_resize_matches_the_float64_restatement(S, in_dtype):
  rng = np.random.default_rng(S + (in_dtype == torch.float16))
  xs, hosts, wins = make_case(rng, S, in_dtype)
  assert len(wins) > 64
  want = reference(hosts, wins, S)
  o32 = resize(xs, wins, S, torch.float32)
  err = np.abs(o32.double().cpu().numpy() - want)
  assert err.max() <= BOUND, (err.max(), np.unravel_index(err.argmax(), err.shape))
  # fp16 output: the fp32 result rounded to nearest even (the kernel rounds the same float32: exactly, not within 1 ulp)
  o16 = resize(xs, wins, S, torch.float16)
  assert torch.equal(o16, o32.half())


def test_area_resize_is_deterministic_and_ragged_equals_single_windows():
  rng = np.random.default_rng(3)
  xs, _hosts, wins = make_case(rng, 80, torch.float32)
  a = resize(xs, wins, 80, torch.float32)
  b = resize(xs, wins, 80, torch.float32)
  assert torch.equal(a, b)
  for k, win in enumerate(wins):
    one = resize([xs[win[0]]], [(0,) + tuple(win[1:])], 80, torch.float32)
    assert torch.equal(one[0], a[k]), k


def seam_image(rng, side, in_dtype):
  """One image a few pixels larger than the window, the window at an odd offset (as make_case places its windows).
  -> (device image, window, the window's pixels in float64 on the host)"""
  y0, x0 = 3, 1
  img = torch.from_numpy(rng.random((side + 3, side + 2, 3), dtype=np.float32)).to(in_dtype)
  return img.to(DEV), (0, y0, x0, side), img[y0:y0 + side, x0:x0 + side].double().numpy()


@pytest.mark.parametrize('S,side', sorted(ref.SEAM_PLANS))
def test_area_resize_across_tile_seams(S, side):
  """Windows of more than kTileCols - 2 = 4094 source columns per S output columns: the kernel cuts the output columns
  into several LDS tiles, each with its own first source column c0, re-using ``colsum`` behind a second barrier.  The
  plans (tests/_area_ref.py::SEAM_PLANS, pinned against the restated tile arithmetic in tests/test_datasets_host.py):
  64 | 63 + 1 | 51 + 13 (integer scale 80) | 43 + 21 | 54 + 26 (S = 80) | 31 + 31 + 2 output columns.  fp32 input up to
  side 6000, fp16 input for 8191 (half the memory).  BOUND does not grow with the side: both passes accumulate in
  double, and the only float32 roundings are ``colsum`` and the store."""
  widths = [ox1 - ox0 for ox0, ox1, _, _ in ref.tile_plan(side, S)]
  assert widths == ref.SEAM_PLANS[(S, side)] and (len(widths) > 1) == (side > 4094)
  in_dtype = torch.float16 if side > 6000 else torch.float32
  x, win, host = seam_image(np.random.default_rng(side + S), side, in_dtype)
  want = ref.area_resize(host, S)
  o32 = resize([x], [win], S, torch.float32)
  err, at = ref.max_err(o32[0].cpu().numpy(), want)
  print('area resize S = %d, side = %d, tiles %r: worst |err| %.3e = %.3f of BOUND at %r' % (S, side, widths, err, err / BOUND, at))
  assert err <= BOUND, (err, at, widths)
  o16 = resize([x], [win], S, torch.float16)
  assert torch.equal(o16, o32.half())


def test_a_multi_tile_window_does_not_depend_on_the_batch_or_the_launch():
  """Side 5120 at S = 64 (tiles of 51 + 13 output columns) alone == the same window inside a ragged call between
  single-tile windows (and once more at another offset of its image: other c0s against the same LDS), and == itself at a
  second launch, bit for bit."""
  rng = np.random.default_rng(11)
  S, side = 64, 5120
  assert len(ref.tile_plan(side, S)) == 2 and len(ref.tile_plan(239, S)) == 1
  big, win, _ = seam_image(rng, side, torch.float32)
  small = torch.from_numpy(rng.random((241, 243, 3), dtype=np.float32)).to(DEV)
  wins = [(1, 0, 1, 97), (0,) + win[1:], (1, 2, 3, 239), (0, 0, 2, side), (1, 5, 0, 64)]
  a = resize([big, small], wins, S, torch.float32)
  b = resize([big, small], wins, S, torch.float32)
  assert torch.equal(a, b)
  for k, w in enumerate(wins):
    one = resize([(big, small)[w[0]]], [(0,) + tuple(w[1:])], S, torch.float32)
    assert torch.equal(one[0], a[k]), k
  assert not torch.equal(a[1], a[3])  # (two different windows of the large image)


@pytest.mark.parametrize('side', [239, 1000])
def test_the_bound_rejects_equal_weight_bins_and_a_shifted_window(side):
  """adaptive_avg_pool2d (torch's 'area') and a window one pixel off both miss the bound on the same data."""
  rng = np.random.default_rng(side)
  img = rng.random((side + 1, side + 1, 3), dtype=np.float32)
  x = torch.from_numpy(img).to(DEV)
  got = resize([x], [(0, 0, 0, side)], 80, torch.float32)[0].double().cpu().numpy()
  want = ref.area_resize(img[:side, :side].astype(np.float64), 80)
  assert np.abs(got - want).max() <= BOUND
  pooled = F.adaptive_avg_pool2d(torch.from_numpy(img[:side, :side]).double().permute(2, 0, 1)[None], 80)[0]
  assert np.abs(pooled.permute(1, 2, 0).numpy() - want).max() > 100 * BOUND
  shifted = resize([x], [(0, 1, 0, side)], 80, torch.float32)[0].double().cpu().numpy()
  assert np.abs(shifted - want).max() > 100 * BOUND


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('S,C', [(80, 64), (64, 64), (9, 5)])
def test_pack_recut_equals_numpy_indexing(dtype, S, C):
  rng = np.random.default_rng(S + C)
  m, count = 37, 301
  master = torch.from_numpy(rng.random((m, S, S, 3), dtype=np.float32)).to(dtype)
  rec = np.stack([rng.integers(0, m, count), rng.integers(0, S - C + 1, count), rng.integers(0, S - C + 1, count),
                  np.arange(count) % 2], axis=1).astype(np.int32)
  buf = torch.full((count + 2, C, C, 3), 5.0, dtype=dtype, device=DEV)
  _cabi.pack_recut(master.to(DEV), torch.from_numpy(rec).to(DEV), buf[1:-1])
  torch.cuda.synchronize()
  assert bool((buf[0] == 5).all()) and bool((buf[-1] == 5).all())
  want = ref.recut(master.numpy(), [tuple(r) + (C,) for r in rec.tolist()])
  assert np.array_equal(buf[1:-1].cpu().numpy(), want)


def write_folders(root, n_fake=5, n_real=5, seed=0, sizes=None):
  """16-bit TIFFs (and one 8-bit TIFF) and 8-bit PNGs of several sizes and aspect ratios."""
  from PIL import Image
  rng = np.random.default_rng(seed)
  fake, real = os.path.join(root, 'fake'), os.path.join(root, 'real')
  os.makedirs(fake)
  os.makedirs(real)
  sizes = sizes or [(96, 130), (141, 83), (80, 80), (200, 161), (97, 97)]
  for k in range(n_fake):
    h, w = sizes[k % len(sizes)]
    if k == 2:
      write_tiff(os.path.join(fake, 'f%03d.tif' % k), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    else:
      write_tiff(os.path.join(fake, 'f%03d.tif' % k), rng.integers(0, 65536, (h, w, 3), dtype=np.uint16))
  for k in range(n_real):
    h, w = sizes[(k + 1) % len(sizes)]
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(real, 'r%03d.png' % k))
  return fake, real


@pytest.mark.parametrize('recipe', ['fivek', 'folder'])
def test_build_pack_matches_the_stand_in_build(tmp_path, monkeypatch, recipe):
  fake, real = write_folders(str(tmp_path))
  paths = datasets.list_files(fake if recipe == 'fivek' else real)
  # small chunks: the chunk boundaries must not change anything
  dev = datasets.build_pack(paths, recipe, torch.float32, DEV, seed=9, max_images=2)
  dev16 = datasets.build_pack(paths, recipe, torch.float16, DEV, seed=9)
  with monkeypatch.context() as mp:
    ref.patch(mp)
    cpu = datasets.build_pack(paths, recipe, torch.float32, 'cpu', seed=9)
  assert dev.shape == cpu.shape == datasets.pack_shape(recipe, len(paths))
  assert float((dev.cpu() - cpu).abs().max()) <= BOUND
  assert torch.equal(dev16, dev.half())


def pack_master(seed, m, S, dtype):
  g = torch.Generator().manual_seed(seed)
  return (torch.rand((m, S, S, 3), generator=g)**2.2 * 0.6).to(dtype).to(DEV)


def test_iteration_graph_over_pack_providers_equals_the_step_calls():
  """Model: test_hip_agent.py::test_iteration_graph_trains_bit_identically_to_the_step_calls, with PackProviders that
  wrap (and re-cut their idle half) several times while the iteration graph replays."""
  from exposure_amd.replay_memory import ReplayMemory
  cfg = make_cfg()
  cfg.batch_size, cfg.replay_memory_size, cfg.citers = 16, 48, 3
  fake_master, real_master = pack_master(1, 48, 80, torch.float16), pack_master(2, 64, 64, torch.float16)
  runs = []
  for planned in (True, False):
    torch.manual_seed(0)
    gan = GAN(cfg, device=DEV, use_graphs=True, seed=4)
    fd, rd = datasets.PackProvider(fake_master, seed=5), datasets.PackProvider(real_master, seed=6)
    mem = ReplayMemory(cfg, fd, rd, seed=0)
    for _ in range(7):
      feed, feats = mem.get_feed_dict_and_states(cfg.batch_size, lazy=True)
      g = gan.generator_step(feed['fake_input'], feed['z'], feed['states'], 0.0, it=0)
      mem.replace_memory(g['fake_output'], g['new_states'], feats, advanced=True)
    epochs0 = (fd.epochs, rd.epochs)
    vals = []
    for it in range(1, 9):
      if planned:
        out = gan.train_iteration(mem, it)
      else:
        out = gan._iteration_stepwise(mem, it, float(it) / cfg.max_iter_step, cfg.batch_size)
      vals += [out['g'][k].clone().reshape(-1)[:1] for k in ('g_loss', 'v_loss')]
      vals += [out['c'][k].clone().reshape(-1)[:1] for k in ('c_loss', 'emd', 'gradient_norm', 'c_average')]
      assert mem.check_host_mirror()
    assert fd.epochs - epochs0[0] >= 2 and rd.epochs - epochs0[1] >= 2, (epochs0, fd.epochs, rd.epochs)
    if planned:
      assert any(k[0] == 'it' and isinstance(v, tuple) for k, v in gan._graphs.items()), 'the iteration graph was never captured'
      assert not any(k[0] == 'c' for k in gan._graphs), 'critic steps ran outside the iteration graph'
    runs.append((torch.cat(vals), mem.images, mem.states, mem.features, fd.images.clone(), rd.images.clone(),
                 float(gan.c_average_biased)) + tuple(p.detach().clone() for p in gan.parameters()))
  assert bool(torch.isfinite(runs[0][0]).all())
  for i, (a, b) in enumerate(zip(*runs)):
    assert (a == b) if isinstance(a, float) else torch.equal(a, b), i


def test_train_cli_on_photo_folders_and_the_pack_cache(tmp_path, capsys):
  from exposure_amd import train
  fake, real = write_folders(str(tmp_path), n_fake=16, n_real=16, seed=3)
  cache = str(tmp_path / 'cache')
  argv = ['--fake-dir', fake, '--real-dir', real, '--iters', '30', '--clamp', '--log-every', '0',
          '--pack-cache', cache]
  hist = train.main(argv + ['--save', str(tmp_path / 'f.pt')])
  out = capsys.readouterr().out
  assert out.count('built') == 2 and 'cache hit' not in out
  assert len(hist) == 31 and all(np.isfinite([h['g_loss'], h['v_loss'], h['emd'], h['cgn']]).all() for h in hist)
  assert os.path.exists(str(tmp_path / 'f.pt'))
  first = {r: np.load(os.path.join(cache, r, datasets.PACK_FILE)) for r in ('fake', 'real')}
  hist2 = train.main(argv[:5] + ['2', '--clamp', '--log-every', '0', '--pack-cache', cache])
  out = capsys.readouterr().out
  assert out.count('cache hit') == 2 and len(hist2) == 3
  for role, recipe, folder, k in (('fake', 'fivek', fake, 1), ('real', 'folder', real, 2)):
    again = np.load(os.path.join(cache, role, datasets.PACK_FILE))
    assert np.array_equal(again, first[role])
    rebuilt = datasets.build_pack(datasets.list_files(folder), recipe, torch.float32, DEV, seed=k)
    assert np.array_equal(rebuilt.cpu().numpy(), first[role])
