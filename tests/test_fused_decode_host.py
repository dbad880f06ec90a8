"""CPU: the host half of retouching straight from integer codes -- evaluate.retouch_batch_raw's
grouping and ordering, its refusals, and the CLI's --fused-decode / --pictures-only, against CPU stand-ins of the three
new binding functions defined here by what include/exposure_hip.h promises (tables: the records, the division and the
cast of expo_decode_ragged; a tap or a pixel: float(table[code])).  The path they are compared with runs on the
stand-ins of tests/test_decode_host.py, tests/_bilinear_ref.py and tests/test_taps16_host.py.  The GPU counterpart is
tests/test_hip_fused_decode.py."""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import evaluate
from exposure_amd.config import make_cfg
from exposure_amd.tiff16 import write_tiff
from tests import _bilinear_ref as br
from tests import test_taps16_host as t16
from tests.test_decode_host import fake_decode_ragged
from tests.test_taps_host import agent, inputs

calls = []  # (entry point, number of images, code dtype, channels) of every call of a stand-in


def _c3(codes):
  """the codes of the three output channels as int64 indices (C = 1: replicated; C = 4: alpha dropped)"""
  a = codes.numpy()
  a = np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a[:, :, :3]
  return a.astype(np.int64)


def fake_decode_tables(codes, table, normalize, dtype, workspace=None):
  calls.append(('tables', len(codes), codes[0].dtype, codes[0].shape[2]))
  t = table.numpy()
  if not normalize:
    return torch.from_numpy(t)[None].to(dtype), 0
  rows = []
  with np.errstate(invalid='ignore'):
    for c in codes:
      d = np.float32(2) * t[_c3(c).max()]
      rows.append(torch.from_numpy(t / (d if d != 0 else np.float32('nan'))).to(dtype))
  return torch.stack(rows), t.shape[0]


def _gather(codes, tables, stride):
  """the image the decode would have made of every list entry: T table value per code"""
  entries = tables.shape[1]
  return [tables[i * stride // entries][torch.from_numpy(_c3(c))][None] for i, c in enumerate(codes)]


def fake_bilinear_codes(codes, tables, stride, windows, S, out):
  calls.append(('proxy', len(codes), codes[0].dtype, codes[0].shape[2]))
  return br.bilinear_resize_ragged(_gather(codes, tables, stride), windows, S, out)


def fake_chain_codes(ids, params, codes, tables, stride, ys, tap_mask=0, taps=None):
  calls.append(('pass', len(codes), codes[0].dtype, codes[0].shape[2]))
  assert ys is not None or tap_mask
  assert ids.shape[0] == params.shape[0] == len(codes)
  t16._ragged_taps_fwd(ids, params, _gather(codes, tables, stride), ys, tap_mask, taps)


@contextlib.contextmanager
def stand_ins():
  with t16.fake_taps16(), mock.patch.multiple(
      'exposure_amd._cabi', decode_ragged=fake_decode_ragged, bilinear_resize_ragged=br.bilinear_resize_ragged,
      decode_tables=fake_decode_tables, bilinear_resize_ragged_codes=fake_bilinear_codes,
      chain_fused_fwd_ragged_codes=fake_chain_codes):
    yield


def mixed_raws(seed):
  rng = np.random.default_rng(seed)
  return [(rng.integers(1, 256, (40, 56, 3), dtype=np.uint8), 'srgb8'),
          (rng.integers(1, 65536, (30, 44, 3), dtype=np.uint16), 'prophoto16'),
          (rng.integers(1, 256, (33, 21, 4), dtype=np.uint8), 'srgb8'),
          (rng.integers(1, 65536, (25, 37, 1), dtype=np.uint16), 'srgb16'),
          (rng.integers(1, 256, (70, 65, 3), dtype=np.uint8), 'srgb8'),
          (rng.integers(1, 65536, (9, 12, 3), dtype=np.uint16), 'prophoto16')]


def same(got, want, what):
  if isinstance(want, dict):
    assert sorted(got) == sorted(want), what
    for k in want:
      same(got[k], want[k], '%s[%s]' % (what, k))
  elif isinstance(want, (list, tuple)):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
      same(g, w, '%s[%d]' % (what, i))
  else:
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), what


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('code', ['u8', 'u16'])
def test_retouch_batch_raw_groups_order_and_results(dtype, code):
  cfg = make_cfg()
  ag = agent(cfg)
  raws = mixed_raws(5)
  n = len(raws)
  z, masks = inputs(cfg, n, 6)
  kw = dict(z=z, dropout_masks=masks, return_trace='full', intermediates=code, picture=code)
  with stand_ins():
    want = evaluate.retouch_batch(ag, evaluate.decode_images(raws, dtype, 'cpu'), proxy='device', **kw)
    del calls[:]
    got = evaluate.retouch_batch_raw(ag, raws, dtype, 'cpu', **kw)
    made = list(calls)
    bare = evaluate.retouch_batch_raw(ag, raws, dtype, 'cpu', outputs=False, **kw)
    plain = evaluate.retouch_batch_raw(ag, raws, dtype, 'cpu', z=z, dropout_masks=masks)
  # per (kind, channels) group, in order of first appearance: tables then proxy; after the one agent run, the passes
  groups = [(2, torch.uint8, 3), (2, torch.uint16, 3), (1, torch.uint8, 4), (1, torch.uint16, 1)]
  assert made == [(name,) + g for g in groups for name in ('tables', 'proxy')] + [('pass',) + g for g in groups]
  assert len(got) == len(want) == 6
  for name, g, w in zip(('outputs', 'low', 'states', 'ops', 'intermediates', 'pictures'), got, want):
    same(g, w, name)
  for (codes, _kind), o in zip(raws, got[0]):  # argument order, whatever the grouping
    assert tuple(o.shape) == (1, codes.shape[0], codes.shape[1], 3)
  assert bare[0] == [None] * n
  same(bare[1:], want[1:], 'outputs=False')
  assert len(plain) == 3
  same(plain[0], want[0], 'no taps')


def test_retouch_batch_raw_value_errors():
  cfg = make_cfg()
  raws = mixed_raws(7)[:2]
  with stand_ins():
    with pytest.raises(ValueError, match='no images'):
      evaluate.retouch_batch_raw(agent(cfg), [], torch.float32, 'cpu')
    with pytest.raises(ValueError, match='outputs=False'):
      evaluate.retouch_batch_raw(agent(cfg), raws, torch.float32, 'cpu', outputs=False)
    with pytest.raises(ValueError, match='intermediates'):
      evaluate.retouch_batch_raw(agent(cfg), raws, torch.float32, 'cpu', intermediates='png')
    with pytest.raises(ValueError, match='one call'):
      evaluate.retouch_batch_raw(agent(cfg), raws, torch.float32, 'cpu', intermediates='u8', picture='u16')
    masked = make_cfg()
    masked.masking = True
    with pytest.raises(ValueError, match='masking'):
      evaluate.retouch_batch_raw(agent(masked), raws, torch.float32, 'cpu')
    generic = make_cfg()
    generic.curve_steps = 6
    with mock.patch.multiple('exposure_amd._cabi', decode_tables=mock.Mock(side_effect=AssertionError('called'))):
      with pytest.raises(ValueError, match='curve_steps'):
        evaluate.retouch_batch_raw(agent(generic), raws, torch.float32, 'cpu')


def _write_files(tmp_path):
  from PIL import Image
  rng = np.random.default_rng(21)
  paths = []
  for i, (h, w, mode) in enumerate([(40, 56, 'RGB'), (33, 21, 'RGBA'), (64, 48, 'RGB')]):
    p = str(tmp_path / ('in%d.png' % i))
    Image.fromarray(rng.integers(1, 256, (h, w, len(mode)), dtype=np.uint8), mode).save(p)
    paths.append(p)
  p = str(tmp_path / 'grey16.png')
  Image.fromarray(rng.integers(1, 65536, (25, 37), dtype=np.uint16)).save(p)
  paths.append(p)
  for i, (h, w, c) in enumerate([(30, 44, 3), (25, 19, 4)]):
    p = str(tmp_path / ('in%d.tif' % i))
    write_tiff(p, rng.integers(1, 65536, (h, w, c), dtype=np.uint16))
    paths.append(p)
  return paths


def _run(argv):
  with stand_ins(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    return evaluate.main(argv)


@pytest.mark.parametrize('mode', [['--device-png', '--step-by-step', '--batch', '4'], ['--tiff16', '--step-by-step', '--batch', '3'],
                                  ['--device-png', '--batch', '1'], ['--batch', '4']])
def test_cli_fused_decode_writes_the_same_files(tmp_path, mode):
  paths = _write_files(tmp_path)
  runs = {}
  for name, extra in (('parent', ['--device-decode', '--device-proxy']), ('fused', ['--fused-decode'])):
    out = str(tmp_path / name) + os.sep
    runs[name] = _run(['--seed', '3', '--dtype', 'f32', '--out', out, *mode, *extra, *paths])
  assert len(runs['parent']) == len(runs['fused']) == len(paths)
  for a, b in zip(runs['parent'], runs['fused']):
    assert a['filters'] == b['filters'] and a['states'] == b['states'] and a['abi_filter_ids'] == b['abi_filter_ids']
    assert np.array_equal(a['params24'], b['params24'])
    assert open(a['output'], 'rb').read() == open(b['output'], 'rb').read()
    assert sorted(a['png']) == sorted(b['png']) and sorted(a['tiff']) == sorted(b['tiff'])
    for kind in ('png', 'tiff'):
      for k in a[kind]:
        assert open(a[kind][k], 'rb').read() == open(b[kind][k], 'rb').read(), k
  assert sorted(os.listdir(str(tmp_path / 'parent'))) == sorted(os.listdir(str(tmp_path / 'fused')))


@pytest.mark.parametrize('fused', [True, False])
def test_cli_pictures_only_writes_no_npy(tmp_path, fused):
  paths = _write_files(tmp_path)[:4]
  full, only = str(tmp_path / 'full') + os.sep, str(tmp_path / 'only') + os.sep
  extra = ['--fused-decode'] if fused else ['--device-decode', '--device-proxy']
  common = ['--seed', '3', '--dtype', 'f32', '--device-png', '--step-by-step', '--batch', '4', *extra]
  a = _run(common + ['--out', full] + paths)
  del calls[:]
  b = _run(common + ['--pictures-only', '--out', only] + paths)
  for ra, rb in zip(a, b):
    assert rb['output'] is None and ra['output'].endswith('.npy')
    assert sorted(ra['png']) == sorted(rb['png'])
    for k in ra['png']:
      assert open(ra['png'][k], 'rb').read() == open(rb['png'][k], 'rb').read(), k
  assert not [f for f in os.listdir(only) if f.endswith('.npy')]
  assert [f for f in os.listdir(full) if f.endswith('.npy')]
  assert sorted(f for f in os.listdir(full) if not f.endswith('.npy')) == sorted(os.listdir(only))


def test_cli_pictures_only_passes_outputs_false(tmp_path):
  paths = _write_files(tmp_path)[:2]
  seen = []
  real = evaluate.retouch_batch_raw

  def spy(*a, **kw):
    seen.append(kw.get('outputs'))
    return real(*a, **kw)

  with mock.patch.object(evaluate, 'retouch_batch_raw', spy):
    _run(['--fused-decode', '--tiff16', '--pictures-only', '--batch', '2', '--out', str(tmp_path / 'o') + os.sep] + paths)
    _run(['--fused-decode', '--tiff16', '--batch', '2', '--out', str(tmp_path / 'p') + os.sep] + paths)
  assert seen == [False, True]


@pytest.mark.parametrize('flags', [['--fused-decode', '--stepwise'], ['--fused-decode', '--masking'],
                                   ['--fused-decode', '--show-input'], ['--pictures-only'],
                                   ['--pictures-only', '--png'], ['--fused-decode', '--pictures-only']])
def test_cli_refusals(tmp_path, flags, capsys):
  paths = _write_files(tmp_path)[:1]
  with pytest.raises(SystemExit):
    _run(flags + paths)
  assert ('--fused-decode' if '--pictures-only' not in flags else '--pictures-only') in capsys.readouterr().err


def test_cli_score_with_pictures_only_is_accepted(tmp_path):
  """--score implies --device-png: --pictures-only goes with it"""
  paths = _write_files(tmp_path)[:1]
  with mock.patch('exposure_amd.metrics.set_statistics', return_value=None), \
      mock.patch('exposure_amd.metrics.read_statistics', return_value=None), \
      mock.patch('exposure_amd.metrics.score', return_value=([1.0, 1.0, 1.0], 1.0)):
    rec = _run(['--fused-decode', '--pictures-only', '--score', str(tmp_path), '--out', str(tmp_path / 'o') + os.sep] + paths)
  assert rec[0]['output'] is None and rec[-1] == dict(score=[1.0, 1.0, 1.0], average=1.0)
