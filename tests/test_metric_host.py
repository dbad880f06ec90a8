"""CPU: the host logic of the evaluation metric's device path with the library calls routed to the
NumPy stand-ins of tests/_metric_ref.py and tests/_area_ref.py: the draw order of metrics.patch_windows against
read_images, score against histogram_intersection, the two CLIs (evaluate --score, metrics --device) and their
refusals; and the two exports' argument checks, which run before anything is enqueued.  The GPU half is
tests/test_hip_metric.py."""
import ctypes
import os
import random
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate, metrics
from tests import _metric_ref as mr
from tests import test_cabi_symbols
from tests import test_taps_host as th

vp = ctypes.c_void_p
FAKE = 0x1000  # never dereferenced on the host


# ---- patch_windows ------------------------------------------------------------------------------------------------------
SHAPES = [(240, 160), (160, 240), (160, 160), (80, 200)]  # portrait, landscape, square, short side exactly 80


def index_image(h, w, code):
  """R = the row, G = the column, B = a code of the image: a crop's position can be read off its pixels."""
  a = np.zeros((h, w, 3), dtype=np.uint8)
  a[..., 0] = np.arange(h)[:, None]
  a[..., 1] = np.arange(w)[None, :]
  a[..., 2] = code
  return a


def test_patch_windows_reproduces_read_images_draws(tmp_path):
  from PIL import Image
  for i, (h, w) in enumerate(SHAPES):
    Image.fromarray(index_image(h, w, 20 * i + 5), 'RGB').save(str(tmp_path / ('f%d.png' % i)))
  ra, rb = random.Random(7), random.Random(7)
  got = metrics.read_images(str(tmp_path), rng=ra).double().numpy() * 255.0
  windows, records = metrics.patch_windows(SHAPES, rb)
  assert ra.getstate() == rb.getstate()  # the same draws were consumed
  assert len(windows) == 4 * len(SHAPES) and len(records) == 16 * len(SHAPES) == got.shape[0]
  grid = np.arange(64, dtype=np.float64)
  for r, (src, oy, ox) in enumerate(records):
    img, y0, x0, edge = windows[src]
    assert src // 4 == img == r // 16 and edge == min(SHAPES[img]) and 0 <= oy < 16 and 0 <= ox < 16
    assert 0 <= y0 <= SHAPES[img][0] - edge and 0 <= x0 <= SHAPES[img][1] - edge
    k = edge // 80  # the 80 x 80 reduction averages k x k blocks: the mean index of a block is its start + (k - 1) / 2
    rows = y0 + (oy + grid) * k + (k - 1) / 2
    cols = x0 + (ox + grid) * k + (k - 1) / 2
    np.testing.assert_allclose(got[r, :, :, 0], np.broadcast_to(rows[:, None], (64, 64)), atol=1e-3, err_msg=str(r))
    np.testing.assert_allclose(got[r, :, :, 1], np.broadcast_to(cols[None, :], (64, 64)), atol=1e-3, err_msg=str(r))
    np.testing.assert_allclose(got[r, :, :, 2], 20 * img + 5, atol=1e-3)
  # the draws spread: not every crop of the non-square images starts at 0
  assert len({w[1:3] for w in windows}) > 4


# ---- score ----------------------------------------------------------------------------------------------------------------
def test_score_equals_histogram_intersection(monkeypatch):
  mr.patch(monkeypatch)
  sets = [mr.patches(1), mr.patches(5)]
  stats = []
  for p in sets:
    st = torch.empty((p.shape[0], 3), dtype=torch.float32)
    rec = torch.tensor([(i, 0, 0) for i in range(p.shape[0])], dtype=torch.int32)
    _cabi.patch_stats(torch.from_numpy(p), rec, 64, st)
    stats.append(st)
  ints, avg = metrics.score(stats[0], stats[1])
  want, want_avg = metrics.histogram_intersection(torch.from_numpy(sets[0]), torch.from_numpy(sets[1]))
  assert all(isinstance(v, float) for v in ints) and isinstance(avg, float) and len(ints) == 3
  np.testing.assert_allclose(ints, want, atol=1e-6, rtol=0)
  assert abs(avg - want_avg) <= 1e-6
  assert 0.05 < min(ints) and max(ints) < 0.99  # neither empty nor trivially equal
  # dropped values still count in the divisor (calc_hist)
  a = torch.tensor([[0.1, 0.2, 0.3], [float('nan'), 1.5, -0.1]])
  ints2, _ = metrics.score(a, a[:1].clone())
  assert ints2 == [0.5, 0.5, 0.5]


def test_set_statistics_against_float64_with_stand_ins(monkeypatch):
  """The host composition (chunks, window and record offsets) through the stand-ins: two chunks of images."""
  mr.patch(monkeypatch)
  rng = np.random.default_rng(2)
  imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(96, 80), (81, 130), (120, 83)]]
  from exposure_amd import datasets
  real = datasets.plan_chunks
  monkeypatch.setattr(datasets, 'plan_chunks', lambda nbytes: real(nbytes, max_images=2))
  got = metrics.set_statistics([torch.from_numpy(a) for a in imgs], random.Random(3))
  windows, records = metrics.patch_windows([a.shape[:2] for a in imgs], random.Random(3))
  want = mr.set_statistics(imgs, windows, records)
  assert got.shape == (48, 3) and got.dtype == torch.float32
  assert np.abs(got.double().numpy() - want).max() <= 1e-6  # (the stand-ins round the master and the result to float32)


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------
def write_pngs(folder, sizes, seed):
  from PIL import Image
  os.makedirs(str(folder), exist_ok=True)
  rng = np.random.default_rng(seed)
  paths = []
  for i, (h, w) in enumerate(sizes):
    p = os.path.join(str(folder), 'im%d.png' % i)
    base = rng.integers(40, 216, (1, 1, 3))
    Image.fromarray(np.clip(base + rng.integers(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8), 'RGB').save(p)
    paths.append(p)
  return paths


def parse_lines(text):
  lines = text.strip().splitlines()
  assert lines[-2].startswith('Hist. Inter.: ') and lines[-1].startswith('         Avg: ')
  vals = [float(t.rstrip('%')) for t in lines[-2][len('Hist. Inter.: '):].split()]
  assert len(vals) == 3 and all(t.endswith('%') for t in lines[-2].split()[2:])
  return vals, float(lines[-1].split()[-1].rstrip('%'))


@pytest.mark.parametrize('mode', [['--batch', '4'], ['--batch', '1']])
def test_cli_evaluate_score(tmp_path, monkeypatch, capsys, mode):
  mr.patch(monkeypatch)
  paths = write_pngs(tmp_path / 'in', [(80, 100), (96, 88), (130, 81)], 1)
  write_pngs(tmp_path / 'target', [(90, 120), (85, 80)], 2)
  out_a, out_b = str(tmp_path / 'a') + os.sep, str(tmp_path / 'b') + os.sep
  common = ['--seed', '3', '--dtype', 'f32', *mode]
  with th.fake_taps(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    plain = evaluate.main(common + ['--device-png', '--out', out_b] + paths)
    capsys.readouterr()
    recs = evaluate.main(common + ['--score', str(tmp_path / 'target'), '--score-seed', '9', '--out', out_a] + paths)
    printed = capsys.readouterr().out
  assert len(plain) == 3 and len(recs) == 4  # existing callers see the record only with the flag
  last = recs[-1]
  assert sorted(last) == ['average', 'score'] and len(last['score']) == 3
  assert abs(last['average'] - sum(last['score']) / 3) < 1e-12 and all(0.0 <= v <= 1.0 for v in last['score'])
  vals, avg = parse_lines(printed)
  assert vals == [round(v * 100, 2) for v in last['score']] and avg == round(last['average'] * 100, 2)
  # --score implies --device-png and changes no output
  from PIL import Image
  for a, b in zip(recs[:3], plain):
    np.testing.assert_array_equal(np.load(a['output']), np.load(b['output']))
    np.testing.assert_array_equal(np.asarray(Image.open(a['png']['retouched'])), np.asarray(Image.open(b['png']['retouched'])))
  # the figures are those of the written PNGs (the pictures are the PNGs' pixels) scored with the same seed
  rng = random.Random(9)
  pics = [torch.from_numpy(np.asarray(Image.open(r['png']['retouched'])).copy()) for r in recs[:3]]
  so = metrics.set_statistics(pics, rng)
  want, want_avg = metrics.score(so, metrics.read_statistics(str(tmp_path / 'target'), rng=rng, device='cpu'))
  assert want == last['score'] and want_avg == last['average']


def test_cli_metrics_device(tmp_path, monkeypatch, capsys):
  mr.patch(monkeypatch)
  write_pngs(tmp_path / 'out', [(80, 100), (96, 88)], 3)
  write_pngs(tmp_path / 'target', [(90, 120), (85, 80), (200, 131)], 4)
  with mock.patch.object(metrics, 'CLI_DEVICE', 'cpu'):
    ints, avg = metrics.main(['--device', str(tmp_path / 'out'), str(tmp_path / 'target'), '--seed', '5'])
    printed = capsys.readouterr().out
    again = metrics.main(['--device', '--seed', '5', str(tmp_path / 'out'), str(tmp_path / 'target')])
  assert printed.count('\n') == 2
  vals, pavg = parse_lines(printed)
  assert vals == [round(v * 100, 2) for v in ints] and pavg == round(avg * 100, 2)
  assert again == (ints, avg)  # seeded: the same sample
  rng = random.Random(5)
  so = metrics.read_statistics(str(tmp_path / 'out'), rng=rng, device='cpu')
  assert so.shape == (32, 3)
  assert metrics.score(so, metrics.read_statistics(str(tmp_path / 'target'), rng=rng, device='cpu')) == (ints, avg)
  # without --device nothing changes: the host path and its usage message
  with pytest.raises(SystemExit):
    metrics.main([str(tmp_path / 'out')])


def test_small_and_16_bit_files_are_refused(tmp_path, monkeypatch):
  from PIL import Image
  calls = []
  mr.patch(monkeypatch)
  monkeypatch.setattr(_cabi, 'decode_ragged', lambda *a, **k: calls.append('decode'))
  write_pngs(tmp_path / 'small', [(90, 120), (79, 200)], 5)
  with pytest.raises(ValueError, match=r'im1\.png.*smaller than 80'):
    metrics.read_statistics(str(tmp_path / 'small'), rng=random.Random(1), device='cpu')
  with pytest.raises(ValueError, match='image 1'):
    metrics.set_statistics([torch.zeros((80, 80, 3), dtype=torch.uint8), torch.zeros((100, 79, 3), dtype=torch.uint8)])
  os.makedirs(str(tmp_path / 'deep'))
  Image.fromarray(np.full((90, 90), 40000, dtype=np.uint16)).save(str(tmp_path / 'deep' / 'g16.png'))
  with pytest.raises(ValueError, match=r'g16\.png.*8-bit'):
    metrics.read_statistics(str(tmp_path / 'deep'), device='cpu')
  with pytest.raises(FileNotFoundError):
    metrics.read_statistics(str(tmp_path / 'deep'), tag='nothing', device='cpu')
  assert calls == []  # refused before any launch


# ---- the C-ABI: exported, declared, bound; everything validated before anything is enqueued ---------------------------------
def test_symbols_exported_declared_and_bound():
  lib = ctypes.CDLL(_cabi.LIB_PATH)
  for name in ('expo_patch_stats', 'expo_stat_hist'):
    assert hasattr(lib, name) and name in _cabi.SIGNATURES and name in test_cabi_symbols.header_symbols(), name
  assert _cabi.load().expo_version() == 9  # added exports: the version does not change
  assert callable(_cabi.patch_stats) and callable(_cabi.stat_hist)


def test_patch_stats_validation_before_enqueue():
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  call = lambda master=FAKE, m=4, S=80, rec=FAKE, count=3, C=64, stats=FAKE, dtype=1: lib.expo_patch_stats(
      vp(master), m, S, vp(rec), count, C, vp(stats), dtype, None)
  assert call(dtype=3) == -2 and call(dtype=-1) == -2
  assert call(count=-1) == -1
  assert call(C=81) == -1 and b'C <= S' in err()
  assert call(C=0) == -1 and call(S=0) == -1
  assert call(master=None, rec=None, stats=None, count=0) == 0  # count == 0: no-op
  assert call(m=0) == -1
  for kw in (dict(master=None), dict(rec=None), dict(stats=None)):
    assert call(**kw) == -1 and b'null' in err(), kw


def test_stat_hist_validation_before_enqueue():
  lib = _cabi.load()
  call = lambda stats=FAKE, q=5, bins=32, counts=FAKE: lib.expo_stat_hist(vp(stats), q, bins, vp(counts), None)
  assert call(bins=0) == -1 and b'bins' in lib.expo_last_error()
  assert call(bins=1025) == -1 and call(q=-1) == -1
  assert call(stats=None) == -1 and call(counts=None) == -1 and call(counts=None, q=0) == -1


def test_bindings_refuse_host_tensors():
  master = torch.zeros((2, 80, 80, 3))
  with pytest.raises(_cabi.ExposureHipError, match='no CPU fallback'):
    _cabi.patch_stats(master, torch.zeros((1, 3), dtype=torch.int32), 64, torch.zeros((1, 3)))
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.stat_hist(torch.zeros((4, 3)), 32, torch.zeros((3, 32), dtype=torch.int32))
