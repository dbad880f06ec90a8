"""GPU: expo_png_encode_ragged -- the device's files through independent decoders, never against the
code under test: PIL gives back the picture in every value; zlib (which checks the Adler-32) inflates the concatenated
IDAT payloads to the filtered stream of the NumPy restatement (tests/png_host.py) byte for byte, type bytes included,
which pins the adaptive choice; every chunk's CRC-32 is zlib's; the chunks come in the specified order; and the file
lengths equal the restatement's exactly (an optimal code's cost is unique and the header is fixed, so this holds for
any tie-breaking while no segment needs the length limit)."""
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from exposure_amd import _cabi, evaluate
from tests import png_host
from tests.test_hip_fused_decode import guarded, guards_intact

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
# (3, 21845): rows longer than a segment; (33, 341): three segments, rows straddling them; the others: one segment
SHAPES = [(1, 1), (1, 2), (2, 1), (7, 9), (64, 64), (33, 341), (3, 21845)]
FILTERS = range(6)


def seg_bytes():
  return _cabi.png_segment_bytes()


def encode(pics, filt, **kw):
  """numpy pictures -> the device's files as bytes, and the lengths it reported"""
  outs, sizes = _cabi.png_encode_ragged([torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in pics], filt, **kw)
  sizes = sizes.cpu().tolist()
  return [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, sizes)], sizes


def check_file(data, pic, filt, what):
  h, w, _ = pic.shape
  got = np.array(Image.open(io.BytesIO(data)))
  assert got.shape == pic.shape and got.dtype == np.uint8 and np.array_equal(got, pic), what
  total, _stored, depth, stream = png_host.file_plan(pic, filt, seg_bytes())
  zstream = png_host.check_structure(data, h, w, seg_bytes())  # every CRC, the chunk order
  assert zlib.decompress(zstream) == stream.tobytes(), what
  return total, depth


@pytest.fixture(scope='module')
def cases():
  return [(shape, name, pic) for shape in SHAPES
          for name, pic in png_host.contents(shape[0], shape[1], seed=shape[0] * 100003 + shape[1]).items()]


@pytest.mark.parametrize('filt', FILTERS)
def test_files_decode_to_the_pixels_and_have_the_restatements_lengths(cases, filt):
  files, sizes = encode([pic for _, _, pic in cases], filt)  # 28 pictures of mixed sizes in one call
  for (shape, name, pic), data, size in zip(cases, files, sizes):
    what = (shape, name, png_host.FILTERS[filt])
    assert size == len(data) <= _cabi.png_encode_bound(*shape), what
    total, depth = check_file(data, pic, filt, what)
    assert depth <= 15, what  # no length limit here, so the length is the optimal code's
    assert size == total, (what, size, total)
    if name == 'noise' and filt == 0 and shape[0] * shape[1] >= 64 * 64:  # incompressible: every segment stored
      assert size == _cabi.png_encode_bound(*shape), what


def _length_of(payload, sym):
  """the code length of a literal/length symbol in a dynamic segment's header"""
  bits = np.unpackbits(np.frombuffer(payload[:160], dtype=np.uint8), bitorder='little')
  at = 74 + 4 * sym
  return int(bits[at]) * 8 + int(bits[at + 1]) * 4 + int(bits[at + 2]) * 2 + int(bits[at + 3])  # sent from the top bit


def test_zeros_give_two_codes_of_length_one():
  pic = np.zeros((64, 64, 3), np.uint8)
  (data,), _ = encode([pic], 0)
  first = png_host.idat_payloads(data)[1]
  assert first[0] & 7 == 0b101  # BFINAL, BTYPE 10
  lengths = [_length_of(first, s) for s in range(257)]
  assert lengths[0] == 1 and lengths[256] == 1 and sum(lengths) == 2


def test_segment_edges():
  seg = seg_bytes()
  rng = np.random.default_rng(11)
  pics = []
  for h in (seg // 16 - 1, seg // 16, seg // 16 + 1, 2 * seg + 7):  # rows of 16 stream bytes
    yy = np.arange(h)[:, None, None]
    pics.append(((yy // 3 + np.arange(5)[None, :, None] * 9 + rng.integers(-2, 3, (h, 5, 3))) % 256).astype(np.uint8))
  pics.append(rng.integers(0, 256, (seg // 16, 5, 3), dtype=np.uint8))  # one stored segment of exactly SEG bytes
  for filt in (0, 4, 5):
    files, sizes = encode(pics, filt)
    for pic, data, size in zip(pics, files, sizes):
      total, _ = check_file(data, pic, filt, (pic.shape, filt))
      assert size == len(data) == total, (pic.shape, filt, size, total)


def test_length_limit():
  pic = png_host.deep_picture()  # asserts that the optimal code is deeper than 15 bits
  (data,), (size,) = encode([pic], 0)
  check_file(data, pic, 0, 'deep')
  assert size == len(data) <= _cabi.png_encode_bound(1, 1925)
  first = png_host.idat_payloads(data)[1]
  assert first[0] & 7 == 0b101  # one dynamic block: the limited code is in use


def test_batches_equal_single_calls_and_repeat():
  rng = np.random.default_rng(13)
  mixed = [png_host.contents(h, w, seed=h + w)['smooth'] for h, w in ((1, 1), (7, 9), (33, 341), (64, 64), (130, 5))]
  together, _ = encode(mixed, 5)
  again, _ = encode(mixed, 5)
  assert together == again
  for pic, data in zip(mixed, together):
    (alone,), _ = encode([pic], 5)
    assert alone == data, pic.shape
  small = [rng.integers(0, 40, (3 + i % 5, 2 + i % 7, 3), dtype=np.uint8) for i in range(65)]  # two launch groups
  files, sizes = encode(small, 5)
  for pic, data, size in zip(small, files, sizes):
    assert size == len(data) == check_file(data, pic, 5, pic.shape)[0]


@pytest.mark.parametrize('slack', (0, 37))
def test_nothing_is_written_outside_the_buffers(slack):
  rng = np.random.default_rng(17)
  pics = [rng.integers(0, 256, (33, 341, 3), dtype=np.uint8), png_host.contents(64, 64, seed=2)['smooth'],
          rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)]
  dev = [torch.from_numpy(p).to(DEV) for p in pics]
  held = [guarded((_cabi.png_encode_bound(p.shape[0], p.shape[1]) + slack,), torch.uint8, off=i) for i, p in enumerate(pics)]
  import ctypes
  n = len(pics)
  need = int(_cabi.load().expo_png_encode_workspace_bytes((ctypes.c_int * n)(*[p.shape[0] for p in pics]),
                                                          (ctypes.c_int * n)(*[p.shape[1] for p in pics]), n))
  wbuf, wsp = guarded((need,), torch.uint8)
  assert wsp.data_ptr() % 16 == 0
  outs, sizes = _cabi.png_encode_ragged(dev, 5, outs=[t for _, t in held], workspace=wsp)
  sizes = sizes.cpu().tolist()
  assert guards_intact(wbuf, wsp, torch.uint8)
  for (buf, t), pic, size in zip(held, pics, sizes):
    assert guards_intact(buf, t, torch.uint8), pic.shape
    assert bool((t[size:] == 0xA5).all()), pic.shape  # nothing behind the file either
    check_file(t[:size].cpu().numpy().tobytes(), pic, 5, pic.shape)
  assert sizes[0] == _cabi.png_encode_bound(33, 341)  # noise under the adaptive filter: still every segment stored


def test_encode_png_batch_and_validation():
  pics = [torch.from_numpy(png_host.contents(7, 9, seed=3)['smooth']).to(DEV), torch.zeros((2, 1, 3), dtype=torch.uint8, device=DEV)]
  files = evaluate.encode_png_batch(pics, 'paeth')
  assert [np.array_equal(np.array(Image.open(io.BytesIO(f))), p.cpu().numpy()) for f, p in zip(files, pics)] == [True, True]
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.png_encode_ragged([pics[0].float()])
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.png_encode_ragged([pics[0][:, ::2]])
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.png_encode_ragged([pics[0]], outs=[torch.empty((10,), dtype=torch.uint8, device=DEV)])


def test_cli_device_png_encode_writes_the_same_pixels(tmp_path, capsys):
  rng = np.random.default_rng(19)
  paths = []
  for i, (h, w) in enumerate(((40, 56), (61, 94), (67, 129))):
    yy, xx = np.mgrid[0:h, 0:w]
    pic = ((yy * 2 + xx)[:, :, None] // 2 + np.arange(3) * 30 + rng.integers(0, 6, (h, w, 3))) % 256
    paths.append(str(tmp_path / ('in%d.png' % i)))
    Image.fromarray(pic.astype(np.uint8), 'RGB').save(paths[-1])
  common = ['--fused-decode', '--device-png', '--step-by-step', '--show-input', '--show-linear', '--device-input-png',
            '--batch', '3', '--seed', '5']
  host = evaluate.main(common + ['--out', str(tmp_path / 'host') + os.sep] + paths)
  dev = evaluate.main(common + ['--device-png-encode', '--out', str(tmp_path / 'dev') + os.sep] + paths)
  assert sorted(os.listdir(str(tmp_path / 'host'))) == sorted(os.listdir(str(tmp_path / 'dev')))
  assert len(host) == len(dev) == 3
  for a, b in zip(host, dev):
    assert sorted(a['png']) == sorted(b['png']) and {'retouched', 'linear', 'input_tone_mapped', 'intermediate00'} <= set(b['png'])
    for k in a['png']:
      assert os.path.basename(a['png'][k]) == os.path.basename(b['png'][k])
      assert np.array_equal(np.asarray(Image.open(a['png'][k])), np.asarray(Image.open(b['png'][k]))), k
      data = open(b['png'][k], 'rb').read()
      assert [c for c, _ in png_host.parse(data)][:3] == [b'IHDR', b'IDAT', b'IDAT'] and png_host.parse(data)[1][1] == b'\x78\x01'
    for k in ('image', 'filters', 'states', 'abi_filter_ids', 'tiff'):
      assert a[k] == b[k], k
    assert np.array_equal(a['params24'], b['params24']) and np.array_equal(np.load(a['output']), np.load(b['output']))
  capsys.readouterr()
  with pytest.raises(SystemExit):
    evaluate.main(['--device-png-encode', '--tiff16'] + paths[:1])
  assert '--device-png-encode' in capsys.readouterr().err
