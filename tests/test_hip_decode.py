"""GPU: expo_decode_ragged against load_image's own float32 maths, bit for bit.  The host half (the
tables, load_raw, the CLI against a CPU stand-in) is tests/test_decode_host.py."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate
from exposure_amd.tiff16 import write_tiff

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
KINDS = ('srgb8', 'srgb16', 'prophoto16')
DTYPES = (torch.float16, torch.float32)


def host_math(codes, kind):
  """load_image's float32 expressions on (H, W, C) codes (C = 1: replicated; C = 4: alpha dropped)"""
  c3 = np.repeat(codes, 3, axis=2) if codes.shape[2] == 1 else codes[:, :, :3]
  if kind == 'prophoto16':
    return evaluate.linearize_ProPhotoRGB(c3.astype(np.float32) / 65535.0)
  img = (c3.astype(np.float32) / (255.0 if kind == 'srgb8' else 65535.0))**2.2
  return img / (2 * img.max())


def codes_of(rng, kind, h, w, c):
  hi = 256 if kind == 'srgb8' else 65536
  return rng.integers(0, hi, (h, w, c), dtype=np.uint8 if kind == 'srgb8' else np.uint16)


def decode(codes_list, kind, dtype):
  cs = [torch.from_numpy(np.ascontiguousarray(c)).to(DEV) for c in codes_list]
  ys = [torch.empty((c.shape[0], c.shape[1], 3), dtype=dtype, device=DEV) for c in codes_list]
  _cabi.decode_ragged(cs, evaluate.decode_table(kind, DEV), evaluate.DECODE_NORMALIZE[kind], ys)
  torch.cuda.synchronize()
  return ys


def same_bits(got, want):
  g, w = got.cpu(), want.cpu()
  assert g.shape == w.shape and g.dtype == w.dtype
  if g.dtype == torch.float16:
    g, w = g.view(torch.int16), w.view(torch.int16)
  else:
    g, w = g.view(torch.int32), w.view(torch.int32)
  bad = int((g != w).sum())
  assert bad == 0, '%d values differ' % bad


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', (1, 3, 4))
def test_every_kind_dtype_channels_and_size(kind, c):
  rng = np.random.default_rng(10 * KINDS.index(kind) + c)
  sizes = [(1, 1), (3, 5), (67, 129), (1023, 1537)]
  codes = [codes_of(rng, kind, h, w, c) for h, w in sizes]
  for dt in DTYPES:
    for cd, y in zip(codes, decode(codes, kind, dt)):  # one ragged call of the four sizes
      same_bits(y, torch.from_numpy(host_math(cd, kind)).to(dt))
    for cd in codes:  # one call per image
      same_bits(decode([cd], kind, dt)[0], torch.from_numpy(host_math(cd, kind)).to(dt))


def test_24mp_8bit():
  rng = np.random.default_rng(5)
  cd = rng.integers(0, 250, (4000, 6000, 3), dtype=np.uint8)
  want = torch.from_numpy(host_math(cd, 'srgb8'))
  for dt in DTYPES:
    same_bits(decode([cd], 'srgb8', dt)[0], want.to(dt))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('place', ('first', 'last', 'channel2', 'alpha'))
def test_every_code_and_where_the_maximum_sits(kind, place):
  hi = 256 if kind == 'srgb8' else 65536
  ct = np.uint8 if kind == 'srgb8' else np.uint16
  rng = np.random.default_rng(hi + len(place))
  c = 4 if place == 'alpha' else 3
  h, w = (16, 16) if hi == 256 else (128, 171)  # h w 3 >= hi - 1: every code below the largest appears
  img = rng.permutation(np.arange(h * w * 3) % (hi - 1)).astype(ct).reshape(h, w, 3)
  if c == 4:
    img = np.concatenate([img, rng.integers(0, hi - 1, (h, w, 1)).astype(ct)], axis=2)
  top = hi - 1
  if place == 'first':
    img[0, 0, 0] = top
  elif place == 'last':
    img[-1, -1, 2] = top
  elif place == 'channel2':
    img[h // 2, w // 3, 2] = top
  else:  # only alpha holds the largest code: it must not count
    img[h // 2, w // 3, 3] = top
  for dt in DTYPES:
    same_bits(decode([img], kind, dt)[0], torch.from_numpy(host_math(img, kind)).to(dt))


@pytest.mark.parametrize('kind', ('srgb8', 'srgb16'))
def test_all_zero_image_is_nan(kind):
  ct = np.uint8 if kind == 'srgb8' else np.uint16
  img = np.zeros((33, 17, 3), dtype=ct)
  img4 = np.zeros((33, 17, 4), dtype=ct)
  img4[..., 3] = 200  # alpha does not count
  with np.errstate(invalid='ignore'):
    assert np.isnan(host_math(img, kind)).all()
  for dt in DTYPES:
    for y in decode([img], kind, dt) + decode([img4], kind, dt):
      assert torch.isnan(y.float()).all()


@pytest.mark.parametrize('n', (1, 64, 65, 130))
def test_ragged_counts_equal_single_calls(n):
  rng = np.random.default_rng(n)
  for kind, c in (('srgb8', 3), ('srgb16', 4)):
    sizes = [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(n)]
    codes = [codes_of(rng, kind, h, w, c) for h, w in sizes]
    got = decode(codes, kind, torch.float16)
    for cd, y in zip(codes, got):
      same_bits(y, decode([cd], kind, torch.float16)[0])


@pytest.mark.parametrize('kind', KINDS)
def test_odd_offsets_and_guard_elements(kind):
  rng = np.random.default_rng(3)
  ct = torch.uint8 if kind == 'srgb8' else torch.uint16
  table = evaluate.decode_table(kind, DEV)
  for c in (1, 3, 4):
    for dt in DTYPES:
      sizes = [(7, 9), (16, 32), (5, 5)]
      codes = [codes_of(rng, kind, h, w, c) for h, w in sizes]
      # codes at odd element offsets inside one buffer
      total = sum(cd.size for cd in codes) + 16
      buf = torch.zeros(total, dtype=ct, device=DEV)
      views, at = [], 1
      for cd in codes:
        v = buf[at:at + cd.size].view(cd.shape)
        v.copy_(torch.from_numpy(cd).to(DEV))
        views.append(v)
        at += cd.size + 1
      # outputs at odd element offsets inside one buffer full of guard values
      outn = sum(h * w * 3 for h, w in sizes) + 16
      guard = torch.full((outn,), 7.0, dtype=dt, device=DEV)
      outs, at, spans = [], 1, []
      for h, w in sizes:
        outs.append(guard[at:at + h * w * 3].view(h, w, 3))
        spans.append((at, at + h * w * 3))
        at += h * w * 3 + 1
      _cabi.decode_ragged(views, table, evaluate.DECODE_NORMALIZE[kind], outs)
      torch.cuda.synchronize()
      for cd, y in zip(codes, outs):
        same_bits(y, torch.from_numpy(host_math(cd, kind)).to(dt))
      mask = torch.ones(outn, dtype=torch.bool)
      for a, b in spans:
        mask[a:b] = False
      assert (guard.cpu()[mask] == 7.0).all()


def test_repeated_calls_identical_bits():
  rng = np.random.default_rng(9)
  codes = [codes_of(rng, 'srgb16', 301, 257, 3), codes_of(rng, 'srgb16', 64, 64, 3)]
  a = decode(codes, 'srgb16', torch.float16)
  b = decode(codes, 'srgb16', torch.float16)
  for x, y in zip(a, b):
    same_bits(x, y)


def test_decode_images_groups_and_order():
  rng = np.random.default_rng(12)
  raws = [(codes_of(rng, 'srgb8', 20, 30, 3), 'srgb8'), (codes_of(rng, 'prophoto16', 9, 7, 4), 'prophoto16'),
          (codes_of(rng, 'srgb8', 5, 6, 3), 'srgb8'), (codes_of(rng, 'srgb16', 11, 3, 1), 'srgb16')]
  outs = evaluate.decode_images(raws, torch.float16, DEV)
  for (cd, kind), y in zip(raws, outs):
    assert tuple(y.shape) == (1, cd.shape[0], cd.shape[1], 3)
    same_bits(y[0], torch.from_numpy(host_math(cd, kind)).to(torch.float16))


def _write_files(tmp_path):
  from PIL import Image
  rng = np.random.default_rng(21)
  paths = []
  for i, (h, w) in enumerate([(40, 56), (33, 21), (64, 48)]):
    p = str(tmp_path / ('in%d.png' % i))
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'RGB').save(p)
    paths.append(p)
  for i, (h, w, c) in enumerate([(30, 44, 3), (25, 19, 4)]):
    p = str(tmp_path / ('in%d.tif' % i))
    write_tiff(p, rng.integers(0, 65536, (h, w, c), dtype=np.uint16))
    paths.append(p)
  return paths


@pytest.mark.parametrize('batch', ('1', '4'))
def test_cli_device_decode_matches_default(tmp_path, batch):
  paths = _write_files(tmp_path)
  runs = {}
  for mode in ('host', 'device'):
    out = str(tmp_path / mode) + os.sep
    extra = ['--device-decode'] if mode == 'device' else []
    runs[mode] = (out, evaluate.main(['--seed', '3', '--batch', batch, '--png', '--show-input', '--step-by-step',
                                      '--out', out] + extra + paths))
  (oh, rh), (od, rd) = runs['host'], runs['device']
  assert len(rh) == len(rd) == len(paths)
  for a, b in zip(rh, rd):
    assert a['filters'] == b['filters'] and a['states'] == b['states'] and a['abi_filter_ids'] == b['abi_filter_ids']
    assert np.array_equal(a['params24'], b['params24'])
    assert open(a['output'], 'rb').read() == open(b['output'], 'rb').read()
    assert sorted(a['png']) == sorted(b['png']) and 'input_tone_mapped' in a['png']
    for k in a['png']:
      assert open(a['png'][k], 'rb').read() == open(b['png'][k], 'rb').read(), k
