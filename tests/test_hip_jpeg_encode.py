"""GPU: expo_jpeg_encode_ragged -- the device's files against the NumPy restatement of the format
(tests/jpeg_host.py, written from the format's text) byte for byte, never against the code under test; PIL decodes
them.  tests/test_jpeg_host.py holds the restatement to PIL's tables and decoder and proves that the case set reaches
every path of the entropy coder."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from exposure_amd import _cabi, evaluate
from tests import jpeg_host
from tests.test_hip_fused_decode import guarded, guards_intact

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SUBS = jpeg_host.SUBSAMPLINGS


def ri_of(sub):
  return _cabi.jpeg_restart_mcus(sub)


def upload(pic):
  return torch.from_numpy(np.ascontiguousarray(pic)).to(DEV)


def bounds(pics, sub):
  return [_cabi.jpeg_encode_bound(p.shape[0], p.shape[1], sub) for p in pics]


def encode(pics, quality, sub, **kw):
  """numpy pictures -> the device's files as bytes (None where the capacity was too small), and the reported lengths;
  the capacity is the bound unless one is given (the default, 629 + 3 h w, is below the file of a tiny picture)"""
  if 'capacity' not in kw and 'outs' not in kw:
    kw['capacity'] = bounds(pics, sub)
  outs, sizes = _cabi.jpeg_encode_ragged([upload(p) for p in pics], quality, sub, **kw)
  sizes = sizes.cpu().tolist()
  return [o[:n].cpu().numpy().tobytes() if n <= o.numel() else None for o, n in zip(outs, sizes)], sizes


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('quality', jpeg_host.QUALITIES)
def test_files_equal_the_restatement_byte_for_byte(quality, sub):
  ri = ri_of(sub)
  cases, want = jpeg_host.case_pictures(ri), jpeg_host.case_files(quality, sub, ri)
  # 42 pictures of mixed sizes in one call; the bound as capacity, so every file is written
  files, sizes = encode([pic for _, _, pic in cases], quality, sub)
  for (shape, name, pic), full, data, size in zip(cases, want, files, sizes):
    what = (shape, name, quality, sub)
    assert size == len(full['file']), (what, size, len(full['file']))
    assert data == full['file'], what
    assert np.array(Image.open(io.BytesIO(data))).shape == pic.shape, what


def test_65_tiny_pictures_cross_the_launch_group():
  rng = np.random.default_rng(5)
  pics = [rng.integers(0, 256, (1 + i % 9, 1 + i % 11, 3), dtype=np.uint8) for i in range(65)]
  for sub in SUBS:
    files, sizes = encode(pics, 90, sub)
    for pic, data, size in zip(pics, files, sizes):
      want = jpeg_host.encode(pic, 90, sub, ri_of(sub))
      assert size == len(want) and data == want, (pic.shape, sub)


def test_batches_equal_single_calls_and_a_dirty_shared_workspace():
  mixed = [jpeg_host.contents(h, w, seed=h + w)[name] for (h, w), name in
           (((1, 1), 'noise'), ((17, 33), 'smooth'), ((64, 64), 'noise'), ((40, 200), 'smooth'), ((130, 5), 'checker'))]
  dev = [upload(p) for p in mixed]
  for sub in SUBS:
    need = _cabi.jpeg_encode_workspace_bytes([p.shape[0] for p in mixed], [p.shape[1] for p in mixed], sub)
    wbuf, wsp = guarded((need,), torch.uint8)  # uninitialised for the library: full of the sentinel
    assert wsp.data_ptr() % 16 == 0
    outs, sizes = _cabi.jpeg_encode_ragged(dev, 75, sub, capacity=bounds(mixed, sub), workspace=wsp)
    together = [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, sizes.cpu().tolist())]
    wsp.copy_(torch.randint(0, 256, (need,), dtype=torch.uint8, device=DEV))  # dirtied on purpose
    outs, sizes = _cabi.jpeg_encode_ragged(dev[::-1], 75, sub, capacity=bounds(mixed[::-1], sub), workspace=wsp)
    again = [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, sizes.cpu().tolist())][::-1]
    assert together == again
    assert guards_intact(wbuf, wsp, torch.uint8)
    for pic, data in zip(mixed, together):
      (alone,), _ = encode([pic], 75, sub)
      assert alone == data == jpeg_host.encode(pic, 75, sub, ri_of(sub)), (pic.shape, sub)


@pytest.mark.parametrize('sub', SUBS)
def test_capacity_decides_whether_a_file_is_written(sub):
  pics = [jpeg_host.contents(17, 33, seed=2)['smooth'], jpeg_host.contents(64, 64, seed=3)['noise'],
          jpeg_host.contents(1, 1, seed=4)['noise']]
  want = [jpeg_host.encode(p, 90, sub, ri_of(sub)) for p in pics]
  dev = [upload(p) for p in pics]
  # one byte short: the length is still exact and not one byte of the buffer is written
  held = [guarded((len(w) - 1,), torch.uint8, off=i) for i, w in enumerate(want)]
  _, sizes = _cabi.jpeg_encode_ragged(dev, 90, sub, outs=[t for _, t in held])
  assert sizes.cpu().tolist() == [len(w) for w in want]
  for (buf, t), pic in zip(held, pics):
    assert bool((buf == 0xA5).all()), pic.shape
  # the exact size: written, and the guard bytes behind it are intact; a short and a fitting buffer in one call
  held = [guarded((len(w),), torch.uint8, off=2 * i + 1) for i, w in enumerate(want)]
  short = guarded((len(want[1]) - 1,), torch.uint8, off=3)
  outs = [held[0][1], short[1], held[2][1]]
  _, sizes = _cabi.jpeg_encode_ragged(dev, 90, sub, outs=outs)
  assert sizes.cpu().tolist() == [len(w) for w in want] and bool((short[0] == 0xA5).all())
  _, sizes = _cabi.jpeg_encode_ragged(dev, 90, sub, outs=[t for _, t in held])
  assert sizes.cpu().tolist() == [len(w) for w in want]
  for (buf, t), w in zip(held, want):
    assert guards_intact(buf, t, torch.uint8) and t.cpu().numpy().tobytes() == w


def test_encode_jpeg_batch_takes_the_second_call_for_noise_at_quality_100():
  pics = [jpeg_host.contents(64, 64, seed=6)['noise'], jpeg_host.contents(64, 64, seed=6)['smooth']]
  want = [jpeg_host.encode(p, 100, 0, ri_of(0)) for p in pics]
  assert len(want[0]) > 629 + 64 * 64 * 3 >= len(want[1])  # the first does not fit the default capacity
  calls = []
  inner = _cabi.jpeg_encode_ragged

  def counting(pictures, *a, **kw):
    calls.append(len(pictures))
    return inner(pictures, *a, **kw)

  _cabi.jpeg_encode_ragged = counting
  try:
    files = evaluate.encode_jpeg_batch([upload(p) for p in pics], 100, '444')
  finally:
    _cabi.jpeg_encode_ragged = inner
  assert calls == [2, 1] and files == want


def test_odd_byte_offsets_of_pictures_and_outputs():
  for sub in SUBS:
    for off in (1, 2, 3):
      pic = jpeg_host.contents(17, 33, seed=off)['noise']
      want = jpeg_host.encode(pic, 90, sub, ri_of(sub))
      store = torch.empty((pic.size + 8,), dtype=torch.uint8, device=DEV)
      src = store[off:off + pic.size].view(17, 33, 3)
      src.copy_(upload(pic))
      buf, out = guarded((len(want) + 5,), torch.uint8, off=off)
      assert src.data_ptr() % 4 == off and src.is_contiguous()
      _, sizes = _cabi.jpeg_encode_ragged([src], 90, sub, outs=[out])
      assert sizes.cpu().tolist() == [len(want)] and out[:len(want)].cpu().numpy().tobytes() == want, (sub, off)
      assert guards_intact(buf, out, torch.uint8) and bool((out[len(want):] == 0xA5).all())


def test_validation_of_the_binding():
  pic = upload(jpeg_host.contents(7, 9, seed=3)['smooth'])
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.jpeg_encode_ragged([pic.float()])
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.jpeg_encode_ragged([pic[:, ::2]])
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.jpeg_encode_ragged([pic], capacity=[10, 10])
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.jpeg_encode_ragged([pic], workspace=torch.empty((8,), dtype=torch.uint8, device=DEV))


def test_cli_device_jpeg_encode_writes_the_files_of_encode_jpeg_batch(tmp_path, capsys):
  rng = np.random.default_rng(19)
  paths = []
  for i, (h, w) in enumerate(((40, 56), (61, 94))):
    yy, xx = np.mgrid[0:h, 0:w]
    pic = ((yy * 2 + xx)[:, :, None] // 2 + np.arange(3) * 30 + rng.integers(0, 6, (h, w, 3))) % 256
    paths.append(str(tmp_path / ('in%d.png' % i)))
    Image.fromarray(pic.astype(np.uint8), 'RGB').save(paths[-1])
  common = ['--fused-decode', '--step-by-step', '--show-input', '--show-linear', '--device-input-png', '--batch', '2',
            '--seed', '5']
  png = evaluate.main(common + ['--device-png-encode', '--out', str(tmp_path / 'png') + os.sep] + paths)
  jpg = evaluate.main(common + ['--device-jpeg-encode', '--jpeg-quality', '85', '--jpeg-subsampling', '444', '--out',
                                str(tmp_path / 'jpg') + os.sep] + paths)
  stems = lambda d, ext: sorted(f[:-len(ext)] for f in os.listdir(str(tmp_path / d)) if f.endswith(ext))
  assert stems('png', '.png') == stems('jpg', '.jpg') and not stems('jpg', '.png')
  assert sorted(os.listdir(str(tmp_path / 'png'))) == sorted(f[:-4] + '.png' if f.endswith('.jpg') else f
                                                              for f in os.listdir(str(tmp_path / 'jpg')))
  assert len(png) == len(jpg) == 2
  for a, b in zip(png, jpg):
    assert sorted(a['png']) == sorted(b['jpeg']) and b['png'] == {}
    assert {'retouched', 'linear', 'input_tone_mapped', 'intermediate00'} <= set(b['jpeg'])
    for k in a['png']:
      assert os.path.basename(a['png'][k])[:-4] + '.jpg' == os.path.basename(b['jpeg'][k])
      picture = torch.from_numpy(np.asarray(Image.open(a['png'][k]))).to(DEV)  # the 8-bit picture of the same run
      (want,) = evaluate.encode_jpeg_batch([picture], 85, '444')
      assert open(b['jpeg'][k], 'rb').read() == want, k
    for k in ('image', 'filters', 'states', 'abi_filter_ids', 'tiff'):
      assert a[k] == b[k], k
    assert np.array_equal(a['params24'], b['params24']) and np.array_equal(np.load(a['output']), np.load(b['output']))
  capsys.readouterr()
  for other in ('--device-png-encode', '--tiff16'):
    with pytest.raises(SystemExit):
      evaluate.main(['--device-jpeg-encode', other] + paths[:1])
    assert '--device-jpeg-encode' in capsys.readouterr().err
