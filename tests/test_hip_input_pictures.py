"""GPU: the reference's input pictures from the integer codes -- expo_codes_max_ragged against torch
maxima over the output channels, expo_codes_lut_ragged against lut[codes] on the host, and evaluate.input_pictures_raw /
the CLI's --device-input-png against the host pictures (save_png's encoding of the decoded input and of
tone_mapped_input of it).  Everything is equal in every value: the device only gathers.  uint16 tensors are compared
through their bytes."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate
from tests.test_hip_decode import codes_of
from tests.test_hip_fused_decode import (DEV, DTYPES, KINDS, _mixed_raws, _write_files, guarded, guards_intact, same,
                                         upload)

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 5), (7, 9), (17, 23)]
NP_CODE = {8: np.uint8, 16: np.uint16}
TORCH_CODE = {8: torch.uint8, 16: torch.uint16}


def c3(cd):
  """the codes of the three output channels (C = 1: replicated; C = 4: alpha dropped)"""
  return np.repeat(cd, 3, axis=2) if cd.shape[2] == 1 else cd[:, :, :3]


def host(t):
  return evaluate._host_codes(t)


# ---------------------------------------------------------------------------------------------------- maxima
@pytest.mark.parametrize('bits', (8, 16))
def test_codes_max_over_the_output_channels(bits):
  rng = np.random.default_rng(bits)
  ct, hi = NP_CODE[bits], (1 << bits) - 1
  for c in (1, 3, 4):
    imgs = [rng.integers(0, hi // 2, (h, w, c)).astype(ct) for h, w in SIZES + [(40, 24), (33, 100), (67, 129)]]
    if c == 4:
      imgs[4][20, 10, 3] = hi  # the largest sample sits only in alpha: it must not count
    # the largest sample only in the last output element, after the last whole 16-byte vector: (33, 100), or with four
    # channels (7, 9), whose 252 / 504 code bytes are no multiple of 16 (the last element of all is alpha there)
    k = 2 if c == 4 else 5
    last = imgs[k]
    assert (last.size * last.itemsize) % 16 >= (2 if c != 4 else 4) * last.itemsize
    last.reshape(-1)[-1 if c != 4 else -2] = hi
    got = _cabi.codes_max_ragged(upload(imgs)).cpu().numpy()
    want = [int(c3(im).max()) for im in imgs]
    assert got.dtype == np.int32 and got.tolist() == want, (c, got.tolist(), want)
    if c == 4:
      assert want[4] < hi
    assert want[k] == hi and sum(w == hi for w in want) == 1


@pytest.mark.parametrize('bits', (8, 16))
def test_codes_max_unaligned_base_and_65_images(bits):
  rng = np.random.default_rng(10 + bits)
  ct = NP_CODE[bits]
  n = 65
  imgs = [rng.integers(0, 1 << bits, (int(rng.integers(1, 30)), int(rng.integers(1, 30)), 3)).astype(ct) for _ in range(n)]
  buf = torch.zeros(sum(im.size for im in imgs) + 2 * n + 4, dtype=TORCH_CODE[bits], device=DEV)
  views, at = [], 1
  for im in imgs:
    v = buf[at:at + im.size].view(im.shape)
    v.copy_(torch.from_numpy(im).to(DEV))
    views.append(v)
    at += im.size + 2 - (im.size % 2)  # every view starts at an odd element
  assert all((v.data_ptr() // v.element_size()) % 2 == 1 for v in views)
  want = [int(im.max()) for im in imgs]
  assert _cabi.codes_max_ragged(views).cpu().tolist() == want
  assert _cabi.codes_max_ragged(upload(imgs)).cpu().tolist() == want


# ---------------------------------------------------------------------------------------------------- gather
def every_code_image(rng, bits, c):
  side = 16 if bits == 8 else 256
  img = rng.permutation(1 << bits).astype(NP_CODE[bits]).reshape(side, side, 1)
  return np.concatenate([img, np.roll(img, 1, 0), np.roll(img, 1, 1), np.roll(img, 2, 0)][:c], axis=2)


@pytest.mark.parametrize('bits', (8, 16))
@pytest.mark.parametrize('out_bits', (8, 16))
@pytest.mark.parametrize('c', (1, 3, 4))
def test_codes_lut_equals_host_gather(bits, out_bits, c):
  rng = np.random.default_rng(100 * bits + 10 * out_bits + c)
  entries = 1 << bits
  imgs = [rng.integers(0, entries, (h, w, c)).astype(NP_CODE[bits]) for h, w in SIZES] + [every_code_image(rng, bits, c)]
  n = len(imgs)
  # random permutation tables (16-bit entries: of the 65536 values, cut to the table), so a wrong entry cannot hide
  luts = np.stack([rng.permutation(1 << out_bits if out_bits >= bits else entries)[:entries] % (1 << out_bits)
                   for _ in range(n)]).astype(NP_CODE[out_bits])
  cs = upload(imgs)
  for shared in (False, True):
    lut = torch.from_numpy(luts[:1] if shared else luts).to(DEV)
    outs = [torch.empty((im.shape[0], im.shape[1], 3), dtype=TORCH_CODE[out_bits], device=DEV) for im in imgs]
    _cabi.codes_lut_ragged(cs, lut, 0 if shared else entries, outs)
    torch.cuda.synchronize()
    for i, (im, o) in enumerate(zip(imgs, outs)):
      want = luts[0 if shared else i][c3(im).astype(np.int64)]
      assert np.array_equal(host(o), want), 'image %d shared %s' % (i, shared)


@pytest.mark.parametrize('bits', (8, 16))
@pytest.mark.parametrize('out_bits', (8, 16))
def test_codes_lut_odd_offsets_and_guards(bits, out_bits):
  rng = np.random.default_rng(7 * bits + out_bits)
  entries = 1 << bits
  ot = TORCH_CODE[out_bits]
  sizes = SIZES + [(16, 32), (40, 56)]
  for c in (1, 3, 4):
    imgs = [rng.integers(0, entries, (h, w, c)).astype(NP_CODE[bits]) for h, w in sizes]
    luts = rng.integers(0, 1 << out_bits, (len(imgs), entries)).astype(NP_CODE[out_bits])
    lut = torch.from_numpy(luts).to(DEV)
    buf = torch.zeros(sum(im.size for im in imgs) + 2 * len(imgs) + 4, dtype=TORCH_CODE[bits], device=DEV)
    views, at = [], 1
    for im in imgs:
      v = buf[at:at + im.size].view(im.shape)
      v.copy_(torch.from_numpy(im).to(DEV))
      views.append(v)
      at += im.size + 2 - (im.size % 2)
    aligned = upload(imgs)
    for src, off in ((views, 1), (aligned, 1), (views, 0), (aligned, 0), (aligned, 3)):
      pairs = [guarded((im.shape[0], im.shape[1], 3), ot, off) for im in imgs]
      _cabi.codes_lut_ragged(src, lut, entries, [t for _b, t in pairs])
      torch.cuda.synchronize()
      for i, (im, (b, t)) in enumerate(zip(imgs, pairs)):
        assert guards_intact(b, t, ot), 'guards: C %d image %d offset %d' % (c, i, off)
        assert np.array_equal(host(t), luts[i][c3(im).astype(np.int64)]), 'C %d image %d offset %d' % (c, i, off)


@pytest.mark.parametrize('n', (1, 64, 65))
def test_codes_lut_ragged_counts(n):
  """the launch split at 64 images: the tables of the second launch start at image 64"""
  rng = np.random.default_rng(n)
  for bits, out_bits, c in ((8, 8, 3), (16, 8, 4), (16, 16, 1)):
    entries = 1 << bits
    imgs = [rng.integers(0, entries, (int(rng.integers(1, 40)), int(rng.integers(1, 40)), c)).astype(NP_CODE[bits])
            for _ in range(n)]
    luts = rng.integers(0, 1 << out_bits, (n, entries)).astype(NP_CODE[out_bits])
    outs = [torch.empty((im.shape[0], im.shape[1], 3), dtype=TORCH_CODE[out_bits], device=DEV) for im in imgs]
    _cabi.codes_lut_ragged(upload(imgs), torch.from_numpy(luts).to(DEV), entries, outs)
    torch.cuda.synchronize()
    for i, (im, o) in enumerate(zip(imgs, outs)):
      assert np.array_equal(host(o), luts[i][c3(im).astype(np.int64)]), 'image %d' % i


def test_codes_lut_lds_staged_16_bit_table(monkeypatch):
  """EXPO_CODES_LUT_LDS16=1: the 64 KiB table of uint8 entries in LDS, blocks walking several chunks -- the same values
  (one image large enough for two trips per block)"""
  rng = np.random.default_rng(77)
  # (2900, 2900): 2054 chunks of 4096 pixels, so the launch's blocks walk two chunks each
  imgs = [every_code_image(rng, 16, 3), rng.integers(0, 65536, (67, 129, 4)).astype(np.uint16),
          rng.integers(0, 65536, (2900, 2900, 1), dtype=np.uint16), rng.integers(0, 65536, (3, 5, 1)).astype(np.uint16)]
  for group in ([imgs[0]], [imgs[1]], [imgs[2], imgs[3]]):
    luts = rng.integers(0, 256, (len(group), 65536)).astype(np.uint8)
    lut, cs = torch.from_numpy(luts).to(DEV), upload(group)
    got = {}
    for flag in ('0', '1'):
      monkeypatch.setenv('EXPO_CODES_LUT_LDS16', flag)
      pairs = [guarded((im.shape[0], im.shape[1], 3), torch.uint8) for im in group]
      _cabi.codes_lut_ragged(cs, lut, 65536, [t for _b, t in pairs])
      torch.cuda.synchronize()
      assert all(guards_intact(b, t, torch.uint8) for b, t in pairs)
      got[flag] = [t for _b, t in pairs]
    for i, im in enumerate(group):
      want = luts[i][c3(im).astype(np.int64)]
      assert np.array_equal(got['0'][i].cpu().numpy(), want) and np.array_equal(got['1'][i].cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- pictures
def host_pictures(raws, dtype):
  """save_png's encoding of the decoded input and of tone_mapped_input of it, per image"""
  lin, tone = [], []
  for im in evaluate.decode_images(raws, dtype, DEV):
    a = im[0].float().cpu().numpy()
    enc = lambda x: np.clip(np.rint(np.asarray(x, dtype=np.float32) * 255.0), 0, 255).astype(np.uint8)  # noqa: E731
    lin.append(enc(a))
    tone.append(enc(evaluate.tone_mapped_input(a)))
  return lin, tone


@pytest.mark.parametrize('dtype', DTYPES)
def test_input_pictures_raw_equals_the_host_pictures(dtype):
  rng = np.random.default_rng(3)
  raws = _mixed_raws(rng) + [(codes_of(rng, k, 17, 23, c), k) for k in KINDS for c in (1, 3, 4)
                             if not (k == 'srgb8' and c == 1)]
  want_lin, want_tone = host_pictures(raws, dtype)
  lin, tone = evaluate.input_pictures_raw(raws, dtype, DEV)
  assert len(lin) == len(tone) == len(raws)
  for i in range(len(raws)):
    assert lin[i].dtype is torch.uint8 and np.array_equal(lin[i].cpu().numpy(), want_lin[i]), 'linear %d' % i
    assert np.array_equal(tone[i].cpu().numpy(), want_tone[i]), 'tone-mapped %d' % i
  only, = evaluate.input_pictures_raw(raws, dtype, DEV, linear=False)
  assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(only, want_tone))
  # 16-bit pictures: encode_u16's encoding of the same float pictures
  lin16, tone16 = evaluate.input_pictures_raw(raws[:4], dtype, DEV, code='u16')
  for i, im in enumerate(evaluate.decode_images(raws[:4], dtype, DEV)):
    same(lin16[i], evaluate.encode_u16(im[0]), 'u16 linear %d' % i)
    t = torch.from_numpy(evaluate.tone_mapped_input(im[0].float().cpu().numpy())).to(DEV)
    same(tone16[i], evaluate.encode_u16(t), 'u16 tone-mapped %d' % i)


@pytest.mark.parametrize('fused', (False, True))
def test_cli_device_input_png_writes_the_host_bytes(tmp_path, fused):
  paths = _write_files(tmp_path)
  common = ['--png', '--show-input', '--show-linear', '--batch', '4', '--seed', '3']
  host_run = evaluate.main(common + ['--device-decode', '--device-proxy', '--out', str(tmp_path / 'host') + os.sep] + paths)
  extra = ['--fused-decode'] if fused else ['--device-decode', '--device-proxy']
  dev_run = evaluate.main(common + extra + ['--device-input-png', '--out', str(tmp_path / 'dev') + os.sep] + paths)
  assert len(host_run) == len(dev_run) == len(paths)
  for a, b in zip(host_run, dev_run):
    assert sorted(a['png']) == sorted(b['png']) == ['input_tone_mapped', 'linear', 'retouched']
    for k in a['png']:
      assert open(a['png'][k], 'rb').read() == open(b['png'][k], 'rb').read(), k
  assert sorted(os.listdir(str(tmp_path / 'host'))) == sorted(os.listdir(str(tmp_path / 'dev')))
