"""GPU: the evaluation metric on the device: expo_patch_stats against the float64 restatement of
tests/_metric_ref.py, its determinism, expo_stat_hist against np.histogram, metrics.set_statistics end to end,
metrics.score against the host metric, and evaluate --score.  The host half is tests/test_metric_host.py.

The bound on a statistic (``_metric_ref.STAT_BOUND`` = 2e-6 absolute): the kernel computes in double and rounds once to
float32, at most 1.2e-7 on values <= 2; the one amplified term is the std near zero, where a variance error of about
4096 * 2^-53 gives at most about 7e-7 after the square root, doubled."""
import os
import random

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate, metrics
from tests import _area_ref
from tests import _metric_ref as mr

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
NP = {torch.float16: np.float16, torch.float32: np.float32}


def device_stats(master, records, c):
  """master: host array (M, S, S, 3) in its storage dtype; records: [(src, oy, ox)] -> (count, 3) device float32."""
  rec = torch.tensor(records, dtype=torch.int32).reshape(-1, 3).to(DEV)
  stats = torch.full((rec.shape[0], 3), float('nan'), dtype=torch.float32, device=DEV)
  return _cabi.patch_stats(torch.from_numpy(master).to(DEV), rec, c, stats)


def records_48():
  """48 records on 5 sources: the corner offsets, repeated sources, and one out of range that must clamp."""
  rng = np.random.default_rng(17)
  rec = [(0, 0, 0), (0, 16, 16), (4, 16, 0), (4, 0, 16), (2, 7, 9), (2, 7, 9), (9, -3, 40)]
  while len(rec) < 48:
    rec.append((int(rng.integers(0, 5)), int(rng.integers(0, 17)), int(rng.integers(0, 17))))
  return rec


@pytest.fixture(scope='module')
def case80():
  """The m = 5, S = 80 masters in both dtypes (float32 values; the fp16 master is its rounding), their records and the
  float64 statistics of what each dtype stores."""
  base = mr.patches(11, n=5, size=80)
  rec = records_48()
  out = {}
  for dt in (torch.float32, torch.float16):
    master = base.astype(NP[dt])
    out[dt] = (master, mr.statistics(mr.crops(master.astype(np.float64), rec, 64)))
  return rec, out


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_patch_stats_against_float64(case80, dtype):
  rec, by_dtype = case80
  master, want = by_dtype[dtype]
  got = device_stats(master, rec, 64).cpu().double().numpy()
  err = np.abs(got - want)
  print('patch_stats %s: worst |device - float64| per statistic %s' % (NP[dtype].__name__, err.max(axis=0)))
  assert np.isfinite(got).all() and err.max() <= mr.STAT_BOUND
  assert np.array_equal(got[4], got[5])  # the same record twice
  # the out-of-range record reads master[4][0:64, 16:80] (clamped), which is record 3
  assert np.array_equal(got[6], got[3])
  # mutants of the oracle violate the bound on these inputs: the test can tell them apart
  crops = mr.crops(master.astype(np.float64), rec, 64)
  assert np.abs(got - mr.statistics(crops, unbiased=True)).max() > mr.STAT_BOUND
  assert np.abs(got - mr.statistics(crops, weights=(0.30, 0.59, 0.11))).max() > mr.STAT_BOUND


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_patch_stats_special_patches(dtype):
  """A constant patch (std exactly 0), a grey one (saturation exactly 0), one with values outside [0, 1] (the clip)."""
  rng = np.random.default_rng(23)
  const = np.broadcast_to(np.array([0.3, 0.55, 0.8]), (80, 80, 3))
  grey = np.repeat(rng.random((80, 80, 1)), 3, axis=2)
  wild = rng.random((80, 80, 3)) * 3.0 - 1.0
  master = np.stack([const, grey, wild]).astype(NP[dtype])
  assert (master[2] < 0).any() and (master[2] > 1).any()
  rec = [(0, 3, 5), (1, 0, 16), (2, 16, 0), (2, 1, 1)]
  got = device_stats(master, rec, 64).cpu().double().numpy()
  want = mr.statistics(mr.crops(master.astype(np.float64), rec, 64))
  print('patch_stats special %s: worst %g' % (NP[dtype].__name__, np.abs(got - want).max()))
  assert np.abs(got - want).max() <= mr.STAT_BOUND
  assert got[0, 1] == 0.0 and got[0, 2] > 0.1
  assert got[1, 2] == 0.0 and got[1, 1] > 0.1
  assert np.abs(got[2, :2] - _no_clip(master, rec)[2, :2]).max() > 1e-2  # the clip is there


def _no_clip(master, rec):
  """the luminance statistics without the clip to [0, 1] (a mutant: it must be told apart on the wild patch)"""
  p = mr.crops(master.astype(np.float64), rec, 64)
  lum = (p[..., 0] * 0.27 + p[..., 1] * 0.67 + p[..., 2] * 0.06).reshape(p.shape[0], -1)
  return np.stack([lum.mean(axis=1), 2 * lum.std(axis=1)], axis=1)


@pytest.mark.parametrize('s,c', [(1, 1), (7, 5)])
def test_patch_stats_small_sizes(s, c):
  """S = C = 1 (one pixel: most threads hold nothing) and a pixel count that is no multiple of the block."""
  rng = np.random.default_rng(5)
  master = rng.random((3, s, s, 3)).astype(np.float32)
  rec = [(0, 0, 0), (2, s - c, s - c), (1, 1, 0), (1, 99, 99)]
  got = device_stats(master, rec, c).cpu().double().numpy()
  want = mr.statistics(mr.crops(master.astype(np.float64), rec, c))
  assert np.abs(got - want).max() <= mr.STAT_BOUND
  if c == 1:
    assert (got[:, 1] == 0.0).all()


def test_patch_stats_determinism(case80):
  rec, by_dtype = case80
  master = by_dtype[torch.float32][0]
  a, b = device_stats(master, rec, 64), device_stats(master, rec, 64)
  assert torch.equal(a, b)
  for r in (0, 6, 31, 47):  # a row computed alone is the row of the 48-record call
    assert torch.equal(device_stats(master, [rec[r]], 64)[0], a[r]), r
  empty = _cabi.patch_stats(torch.from_numpy(master).to(DEV), torch.empty((0, 3), dtype=torch.int32, device=DEV), 64,
                            torch.empty((0, 3), dtype=torch.float32, device=DEV))
  assert empty.shape == (0, 3)


# ---- stat_hist ---------------------------------------------------------------------------------------------------------------
def hist_values():
  rng = np.random.default_rng(3)
  one, edge = np.float32(1.0), np.float32(5 / 32)
  special = [0.0, 1.0, -0.0, 1 / 32, 2 / 32, 5 / 32, 16 / 32, 31 / 32, np.nextafter(edge, np.float32(0)),
             np.nextafter(edge, one), np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)),
             np.nextafter(np.float32(0), one), -1e-3, 1.001, np.nan, np.inf, -np.inf]
  v = np.concatenate([np.array(special, dtype=np.float32), rng.random(600 - len(special), dtype=np.float32)])
  return rng.permutation(v).reshape(200, 3)


@pytest.mark.parametrize('bins', [32, 1])
def test_stat_hist_against_numpy(bins):
  v = hist_values()
  counts = torch.full((3, bins), -7, dtype=torch.int32, device=DEV)  # fully overwritten: no fill by the caller
  _cabi.stat_hist(torch.from_numpy(v).to(DEV), bins, counts)
  want = mr.histogram(v, bins)
  assert np.array_equal(counts.cpu().numpy(), want)
  assert want.sum() == 600 - 6  # the six values outside [0, 1] or not a number are dropped (-0.0 counts as 0)


def test_stat_hist_empty():
  counts = torch.full((3, 32), -7, dtype=torch.int32, device=DEV)
  _cabi.stat_hist(torch.empty((0, 3), dtype=torch.float32, device=DEV), 32, counts)
  assert not counts.any()


# ---- set_statistics ------------------------------------------------------------------------------------------------------
def test_set_statistics_end_to_end(tmp_path):
  from PIL import Image
  rng = np.random.default_rng(29)
  sizes = [(96, 80), (160, 240), (200, 131)]
  hosts = []
  for h, w in sizes:
    base = rng.integers(30, 226, (1, 1, 3))
    hosts.append(np.clip(base + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8))
  imgs = [torch.from_numpy(a).to(DEV) for a in hosts]
  wide = torch.zeros((160, 2 * 240 + 1, 3), dtype=torch.uint8, device=DEV)
  wide[:, 1::2] = imgs[1]
  view = wide[:, 1::2]  # an odd-strided view, made contiguous
  assert not view.is_contiguous()
  imgs[1] = view.contiguous()
  got = metrics.set_statistics(imgs, random.Random(3))
  windows, records = metrics.patch_windows(sizes, random.Random(3))
  want = mr.set_statistics(hosts, windows, records)
  assert got.shape == (48, 3) and got.dtype == torch.float32 and got.device == imgs[0].device
  err = np.abs(got.cpu().double().numpy() - want)
  print('set_statistics: worst |device - float64| per statistic %s' % err.max(axis=0))
  assert err.max() <= mr.STAT_BOUND + _area_ref.BOUND
  assert torch.equal(got, metrics.set_statistics(imgs, random.Random(3)))
  # the device path follows INTER_AREA where the host path rounds its windows: at side 131 they differ visibly
  for i, a in enumerate(hosts):
    Image.fromarray(a, 'RGB').save(str(tmp_path / ('f%d.png' % i)))
  host = metrics.get_statistics(metrics.read_images(str(tmp_path), rng=random.Random(3))).double().numpy()
  diff = np.abs(got.cpu().double().numpy() - host)
  print('set_statistics vs the host read_images path: worst per image %s' % [float(diff[16 * i:16 * i + 16].max())
                                                                          for i in range(3)])
  assert diff[32:].max() > 1e-3
  with pytest.raises(ValueError, match='image 1'):
    metrics.set_statistics([imgs[0], imgs[0][:79].contiguous()], random.Random(1))


# ---- score ----------------------------------------------------------------------------------------------------------------
def test_score_against_host_metric():
  sets = [mr.patches(1), mr.patches(5)]
  rec = [(i, 0, 0) for i in range(48)]
  want64 = [mr.statistics(p) for p in sets]
  # the condition under which a 2e-6 deviation cannot move a value across a bin edge
  assert min(mr.edge_distance(w) for w in want64) > 1e-5
  stats = [device_stats(p, rec, 64) for p in sets]
  for st, w in zip(stats, want64):
    counts = torch.empty((3, 32), dtype=torch.int32, device=DEV)
    _cabi.stat_hist(st, 32, counts)
    assert np.array_equal(counts.cpu().numpy(), mr.histogram(w, 32))
    assert all(int((c > 0).sum()) >= 5 for c in counts.cpu())  # the sets spread over the bins
  ints, avg = metrics.score(stats[0], stats[1])
  want, want_avg = metrics.histogram_intersection(torch.from_numpy(sets[0]), torch.from_numpy(sets[1]))
  print('score: device %s, host %s' % (ints, want))
  np.testing.assert_allclose(ints, want, atol=1e-6, rtol=0)
  assert abs(avg - want_avg) <= 1e-6 and 0.05 < min(ints) and max(ints) < 0.99


# ---- evaluate --score -----------------------------------------------------------------------------------------------------
def test_cli_evaluate_score(tmp_path, capsys):
  from PIL import Image
  from tests.test_metric_host import parse_lines, write_pngs
  paths = write_pngs(tmp_path / 'in', [(80, 100), (96, 88), (200, 131), (120, 160)], 1)
  target = str(tmp_path / 'target')
  write_pngs(target, [(90, 120), (85, 80), (160, 100)], 2)
  out_a, out_b = str(tmp_path / 'a') + os.sep, str(tmp_path / 'b') + os.sep
  common = ['--seed', '0', '--batch', '4']
  recs = evaluate.main(common + ['--score', target, '--score-seed', '9', '--out', out_a] + paths)
  printed = capsys.readouterr().out
  plain = evaluate.main(common + ['--device-png', '--out', out_b] + paths)
  assert len(recs) == 5 and len(plain) == 4 and sorted(recs[-1]) == ['average', 'score']
  for a, b in zip(recs[:4], plain):  # --score changes none of the outputs
    np.testing.assert_array_equal(np.load(a['output']), np.load(b['output']))
    np.testing.assert_array_equal(np.asarray(Image.open(a['png']['retouched'])), np.asarray(Image.open(b['png']['retouched'])))
  # the figures, recomputed from the pictures (= the PNGs' pixels) with the same seed
  rng = random.Random(9)
  pics = [torch.from_numpy(np.asarray(Image.open(r['png']['retouched'])).copy()).to(DEV) for r in recs[:4]]
  so = metrics.set_statistics(pics, rng)
  want, want_avg = metrics.score(so, metrics.read_statistics(target, rng=rng, device=DEV))
  assert recs[-1]['score'] == want and recs[-1]['average'] == want_avg
  vals, avg = parse_lines(printed)
  assert vals == [round(v * 100, 2) for v in want] and avg == round(want_avg * 100, 2)


# ---- refusals, all before any launch --------------------------------------------------------------------------------------
def test_refusals():
  master = torch.zeros((2, 80, 80, 3), device=DEV)
  rec = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
  stats = torch.zeros((1, 3), device=DEV)
  with pytest.raises(_cabi.ExposureHipError, match='records'):
    _cabi.patch_stats(master, rec.cpu(), 64, stats)  # records on the host
  with pytest.raises(_cabi.ExposureHipError, match='C <= S'):
    _cabi.patch_stats(master, rec, 81, stats)
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.patch_stats(master.double(), rec, 64, stats)
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.patch_stats(master, rec, 64, stats.cpu())
  with pytest.raises(_cabi.ExposureHipError, match='bins'):
    _cabi.stat_hist(stats, 0, torch.zeros((3, 0), dtype=torch.int32, device=DEV))
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.stat_hist(stats, 32, torch.zeros((3, 32), dtype=torch.int32))
  lib = _cabi.load()
  assert lib.expo_patch_stats(None, 2, 80, None, 1, 64, None, 1, None) == -1  # null pointers with count > 0
  assert lib.expo_patch_stats(None, 2, 80, None, 1, 64, None, 5, None) == -2  # a bad dtype
  assert (stats == 0).all()  # nothing ran
