"""CPU: the host half of the device decode -- load_raw's file-level choices, the code tables, the
ABI formula stated in numpy against load_image bit for bit, and the CLI's --device-decode against a CPU stand-in of
_cabi.decode_ragged defined here by what expo_decode_ragged promises.  The GPU counterpart is tests/test_hip_decode.py."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import evaluate
from exposure_amd.tiff16 import write_tiff
from tests.test_taps_host import fake_taps


def abi_formula(codes, table, normalize):
  """include/exposure_hip.h, expo_decode_ragged: table gather, the largest code over the output channels, the float32
  division"""
  c3 = np.repeat(codes, 3, axis=2) if codes.shape[2] == 1 else codes[:, :, :3]
  out = table[c3]
  if normalize:
    with np.errstate(invalid='ignore'):
      out = out / (np.float32(2) * table[c3.max()])
  return out


def fake_decode_ragged(codes, table, normalize, outs, workspace=None):
  t = table.numpy()
  for c, y in zip(codes, outs):
    y.copy_(torch.from_numpy(abi_formula(c.numpy(), t, normalize)).reshape(y.shape).to(y.dtype))


def same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  assert a.shape == b.shape and a.dtype == b.dtype == np.float32
  assert np.array_equal(a.view(np.int32), b.view(np.int32)) or (np.isnan(a).all() and np.isnan(b).all())


def _pngs(tmp_path):
  from PIL import Image
  rng = np.random.default_rng(17)
  out = {}
  out['rgb'] = Image.fromarray(rng.integers(0, 256, (21, 34, 3), dtype=np.uint8), 'RGB')
  out['rgba'] = Image.fromarray(rng.integers(0, 256, (13, 8, 4), dtype=np.uint8), 'RGBA')
  out['l'] = Image.fromarray(rng.integers(0, 256, (9, 30), dtype=np.uint8), 'L')
  out['p'] = out['rgb'].convert('P', palette=Image.ADAPTIVE, colors=37)
  out['black'] = Image.fromarray(np.zeros((5, 7, 3), dtype=np.uint8), 'RGB')
  out['grey16'] = Image.fromarray(rng.integers(0, 65536, (11, 19), dtype=np.uint16))
  paths = {}
  for k, im in out.items():
    paths[k] = str(tmp_path / ('%s.png' % k))
    im.save(paths[k])
  paths['tif_rgb'] = str(tmp_path / 'rgb16.tif')
  write_tiff(paths['tif_rgb'], rng.integers(0, 65536, (15, 12, 3), dtype=np.uint16))
  paths['tif_rgba'] = str(tmp_path / 'rgba16.tiff')
  write_tiff(paths['tif_rgba'], rng.integers(0, 65536, (6, 23, 4), dtype=np.uint16))
  return paths


def test_load_raw_kinds_and_abi_formula_equal_load_image(tmp_path):
  paths = _pngs(tmp_path)
  want_kind = dict(rgb='srgb8', rgba='srgb8', l='srgb8', p='srgb8', black='srgb8', grey16='srgb16',
                   tif_rgb='prophoto16', tif_rgba='prophoto16')
  for k, p in paths.items():
    codes, kind = evaluate.load_raw(p)
    assert kind == want_kind[k], k
    assert codes.ndim == 3 and codes.dtype == (np.uint8 if kind == 'srgb8' else np.uint16), k
    assert codes.shape[2] == {'srgb8': 3, 'srgb16': 1, 'prophoto16': 4 if k == 'tif_rgba' else 3}[kind], k
    table = evaluate.decode_table(kind, 'cpu').numpy()
    with np.errstate(invalid='ignore'):
      want = evaluate.load_image(p)
    same(abi_formula(codes, table, evaluate.DECODE_NORMALIZE[kind]), want)
  assert np.isnan(abi_formula(*evaluate.load_raw(paths['black'])[:1], evaluate.decode_table('srgb8', 'cpu').numpy(),
                              1)).all()


def test_8bit_tiff_rejected(tmp_path):
  p = str(tmp_path / 'x.tif')
  write_tiff(p, np.zeros((4, 4, 3), dtype=np.uint8))
  with pytest.raises(ValueError, match='16-bit'):
    evaluate.load_raw(p)
  with pytest.raises(ValueError, match='16-bit'):
    evaluate.load_image(p)


def test_tables_non_decreasing_and_cached():
  for kind, n in (('srgb8', 256), ('srgb16', 65536), ('prophoto16', 65536)):
    t = evaluate.decode_table(kind, 'cpu')
    assert t.dtype == torch.float32 and t.shape == (n,)
    a = t.numpy()
    assert (np.diff(a) >= 0).all() and a[0] == 0 and a[-1] == 1
    assert evaluate.decode_table(kind, 'cpu') is t
  with pytest.raises(ValueError):
    evaluate.decode_table('srgb12', 'cpu')


@pytest.mark.parametrize('kind', ('srgb8', 'srgb16', 'prophoto16'))
def test_table_gather_equals_elementwise_expression(kind):
  """numpy's SIMD pow must not depend on an element's position: table[codes] against the expression on a large image"""
  rng = np.random.default_rng(23)
  hi = 256 if kind == 'srgb8' else 65536
  codes = rng.integers(0, hi, (1000, 1501, 3)).astype(np.uint8 if hi == 256 else np.uint16)
  x = codes.astype(np.float32) / np.float32(hi - 1)
  want = x**1.8 if kind == 'prophoto16' else x**2.2
  same(evaluate.decode_table(kind, 'cpu').numpy()[codes], want)


def test_decode_images_order_and_groups():
  rng = np.random.default_rng(4)
  raws = [(rng.integers(0, 256, (5, 6, 3), dtype=np.uint8), 'srgb8'),
          (rng.integers(0, 65536, (3, 4, 4), dtype=np.uint16), 'prophoto16'),
          (rng.integers(0, 256, (7, 2, 3), dtype=np.uint8), 'srgb8')]
  calls = []

  def rec(codes, table, normalize, outs, workspace=None):
    calls.append((len(codes), normalize))
    fake_decode_ragged(codes, table, normalize, outs)

  with mock.patch('exposure_amd._cabi.decode_ragged', rec):
    outs = evaluate.decode_images(raws, torch.float32, 'cpu')
  assert sorted(calls) == [(1, 0), (2, 1)]
  for (c, kind), y in zip(raws, outs):
    assert tuple(y.shape) == (1, c.shape[0], c.shape[1], 3)
    same(y[0].numpy(), abi_formula(c, evaluate.decode_table(kind, 'cpu').numpy(), evaluate.DECODE_NORMALIZE[kind]))


@pytest.mark.parametrize('mode', [['--batch', '1'], ['--batch', '3'], ['--stepwise']])
def test_cli_device_decode_writes_the_same_files(tmp_path, mode):
  paths = [p for k, p in sorted(_pngs(tmp_path).items()) if k not in ('black', 'grey16')]
  runs = {}
  for name in ('host', 'device'):
    out = str(tmp_path / name) + os.sep
    extra = ['--device-decode'] if name == 'device' else []
    with fake_taps(), mock.patch('exposure_amd._cabi.decode_ragged', fake_decode_ragged), \
        mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
      runs[name] = evaluate.main(['--seed', '3', '--dtype', 'f32', '--png', '--show-input', '--out', out, *mode,
                                  *extra, *paths])
  assert len(runs['host']) == len(runs['device']) == len(paths)
  for a, b in zip(runs['host'], runs['device']):
    assert a['filters'] == b['filters'] and a['states'] == b['states'] and a['abi_filter_ids'] == b['abi_filter_ids']
    assert np.array_equal(a['params24'], b['params24'])
    assert open(a['output'], 'rb').read() == open(b['output'], 'rb').read()
    assert sorted(a['png']) == sorted(b['png']) == ['input_tone_mapped', 'retouched']
    for k in a['png']:
      assert open(a['png'][k], 'rb').read() == open(b['png'][k], 'rb').read(), k


def test_cli_default_path_never_decodes_on_the_device(tmp_path):
  paths = [_pngs(tmp_path)['rgb']]
  with fake_taps(), mock.patch('exposure_amd._cabi.decode_ragged', side_effect=AssertionError('called')), \
      mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    assert len(evaluate.main(['--seed', '1', '--dtype', 'f32', '--out', str(tmp_path / 'o') + os.sep, *paths])) == 1
