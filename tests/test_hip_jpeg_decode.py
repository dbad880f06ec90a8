"""GPU: expo_jpeg_decode_ragged -- the device's pictures against the NumPy restatement of the decoder
(tests/jpeg_decode_host.py, written from the section's text and held to PIL bit for bit by
tests/test_jpeg_decode_host.py), never against the code under test; then the callers: the CLI with and without
--device-jpeg-decode, and the folder recipe's master pack."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from exposure_amd import _cabi, jpeg_decode
from tests import jpeg_decode_host as host
from tests import jpeg_host
from tests.test_hip_fused_decode import guarded, guards_intact

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pick(prefix, suffix):
  """the name of the case file of a shape (prefix) and a quality, sampling and variant (suffix)"""
  return next(n for n, _ in host.case_files() if n.startswith(prefix) and n.endswith(suffix))


def decode(datas, **kw):
  outs, statuses = jpeg_decode.decode_jpeg_batch(datas, DEV, **kw)
  return [o.cpu().numpy() for o in outs], statuses


def test_the_case_set_equals_the_restatement_bit_for_bit():
  files, want = host.case_files(), host.case_decoded()
  # ~400 files of mixed sizes, samplings, tables and restart intervals in one call (seven launch groups)
  got, statuses = decode([data for _, data in files], errors='return')
  assert statuses == [0] * len(files)
  for (name, _), full, pic in zip(files, want, got):
    assert pic.shape == full['rgb'].shape and pic.dtype == np.uint8, name
    assert np.array_equal(pic, full['rgb']), (name, int(np.abs(pic.astype(int) - full['rgb'].astype(int)).max()))


def test_65_one_pixel_files_cross_the_launch_group():
  rng = np.random.default_rng(5)
  datas = [host.pil_encode(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), quality=90, subsampling=i % 3) for i in range(65)]
  got, statuses = decode(datas)
  assert statuses == [0] * 65
  for data, pic in zip(datas, got):
    assert np.array_equal(pic, host.decode(data))


def raw_call(datas, plans, outs, status, workspace=None, file_off=0):
  """expo_jpeg_decode_ragged on files uploaded one by one, `file_off` bytes into their buffers"""
  files = []
  for d in datas:
    buf = torch.zeros(len(d) + file_off + 16, dtype=torch.uint8, device=DEV)
    buf[file_off:file_off + len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(DEV)
    files.append(buf[file_off:file_off + len(d)])
  blobs = [torch.from_numpy(p.blob).to(DEV) for p in plans]
  _cabi.jpeg_decode_ragged(files, blobs, [p.h for p in plans], [p.w for p in plans], [p.sampling for p in plans],
                           [p.ncomp for p in plans], [p.nsegs for p in plans], outs, status, workspace=workspace)
  return files, blobs


def test_alone_in_a_batch_and_across_calls_on_a_dirtied_workspace():
  names = [pick('33x50-', '-q90-s2-rst3'), pick('17x33-', '-q50-s1-default'), pick('64x64-L-', '-q100-optimize'), '8x1040-rst1', '1x1-own-s0']
  datas = [dict(host.case_files())[n] for n in names]
  want = [host.decode(d) for d in datas]
  plans = [jpeg_decode.parse(d) for d in datas]
  need = jpeg_decode.workspace_bytes(plans)
  wbuf, wsp = guarded((need,), torch.uint8)  # uninitialised for the library: full of the sentinel
  assert wsp.data_ptr() % 16 == 0
  for order in (list(range(5)), [4, 3, 2, 1, 0], [2], [0, 0, 3]):
    outs = [torch.empty(want[i].shape, dtype=torch.uint8, device=DEV) for i in order]
    status = torch.full((len(order),), 77, dtype=torch.int32, device=DEV)  # written for every picture
    raw_call([datas[i] for i in order], [plans[i] for i in order], outs, status, workspace=wsp)
    assert status.cpu().tolist() == [0] * len(order)
    for i, o in zip(order, outs):
      assert np.array_equal(o.cpu().numpy(), want[i]), (order, names[i])
    assert guards_intact(wbuf, wsp, torch.uint8)
    wsp.copy_(torch.randint(0, 256, (need,), dtype=torch.uint8, device=DEV))  # dirtied on purpose
  alone, _ = decode(datas[:1])
  assert np.array_equal(alone[0], want[0])


def test_outputs_and_files_at_odd_byte_offsets_keep_their_guards():
  by_name = dict(host.case_files())
  datas = [by_name[n] for n in by_name if n.startswith(('7x9-', '17x33-', '33x50-')) and n.endswith(('-q90-s0-default', '-q90-s1-rst3', '-q90-s2-rstrow', '-L-q50-default'))]
  assert len(datas) == 12
  plans = [jpeg_decode.parse(d) for d in datas]
  for off in (1, 2, 3):
    pairs = [guarded((p.h, p.w, 3), torch.uint8, off=off) for p in plans]
    assert pairs[0][1].data_ptr() % 4 == off
    status = torch.empty((len(datas),), dtype=torch.int32, device=DEV)
    raw_call(datas, plans, [t for _, t in pairs], status, file_off=off)
    assert status.cpu().tolist() == [0] * len(datas)
    for d, (buf, t) in zip(datas, pairs):
      assert np.array_equal(t.cpu().numpy(), host.decode(d)), off
      assert guards_intact(buf, t, torch.uint8), off


def test_malformed_files_set_their_status_and_touch_nothing_else():
  """ordinary malformed inputs that the kernel is built to bound (tools/jpeg_decode_rehearse.cpp walks the same files
  under AddressSanitizer): the statuses are the restatement's, the guards are intact, the good files are unaffected"""
  by_name = dict(host.case_files())
  good = [by_name['33x50-merged-s2'], by_name['8x1040-rst1'], by_name['17x33-merged-s0']]
  bad = [data for _, data in host.malformed_files()]
  datas = [good[0], bad[0], good[1], bad[1], bad[2], good[2]]
  want_status = [host.decode_full(d)['status'] for d in datas]
  assert want_status[0] == want_status[2] == want_status[5] == 0 and sorted(want_status[i] for i in (1, 3, 4)) == [1, 2, 4]
  plans = [jpeg_decode.parse(d) for d in datas]
  pairs = [guarded((p.h, p.w, 3), torch.uint8, off=1) for p in plans]
  need = jpeg_decode.workspace_bytes(plans)
  wbuf, wsp = guarded((need,), torch.uint8)
  status = torch.full((6,), 77, dtype=torch.int32, device=DEV)
  raw_call(datas, plans, [t for _, t in pairs], status, workspace=wsp)
  torch.cuda.synchronize()  # the call returns
  assert status.cpu().tolist() == want_status
  assert guards_intact(wbuf, wsp, torch.uint8)
  for i, (buf, t) in enumerate(pairs):
    assert guards_intact(buf, t, torch.uint8), i
    if want_status[i] == 0:
      assert np.array_equal(t.cpu().numpy(), host.decode(datas[i])), i


def test_decode_jpeg_batch_names_the_bad_files_and_splits_by_the_byte_budget():
  by_name = dict(host.case_files())
  bad = dict(host.malformed_files())
  datas = [by_name[pick('64x64-', '-q90-s0-default')], bad['cut'], bad['ones']]
  with pytest.raises(jpeg_decode.JpegDataError, match=r'b\.jpg \(TRUNCATED\), c\.jpg \(BAD_CODE\)'):
    jpeg_decode.decode_jpeg_batch(datas, DEV, names=['a.jpg', 'b.jpg', 'c.jpg'])
  outs, statuses = jpeg_decode.decode_jpeg_batch(datas, DEV, errors='return')
  assert statuses == [0, host.TRUNCATED, host.BAD_CODE] and [tuple(o.shape) for o in outs] == [host.decode(datas[0]).shape, (33, 50, 3), (33, 50, 3)]
  # a budget below two pictures' workspace: one call per picture, the same pictures
  files = [d for n, d in host.case_files() if n.startswith('33x50-')][:9]
  split, statuses = decode(files, max_bytes=1)
  assert statuses == [0] * 9
  for d, pic in zip(files, split):
    assert np.array_equal(pic, host.decode(d))
  with pytest.raises(jpeg_decode.UnsupportedJpeg, match='progressive'):
    jpeg_decode.decode_jpeg_batch([host.pil_encode(host.decode(files[0]), progressive=True)], DEV)
  assert jpeg_decode.decode_jpeg_batch([], DEV) == ([], [])


# ------------------------------------------------------------------------------------------------------------ the callers
@pytest.fixture(scope='module')
def cli_inputs(tmp_path_factory):
  """case files of every shape but 1 x 1 as .jpg / .jpeg paths (every sampling, variant, a grey and an own file among
  them), one progressive JPEG and one PNG"""
  d = tmp_path_factory.mktemp('inputs')
  by_name = dict(host.case_files())
  names = [pick('7x9-', '-q90-s2-default'), pick('8x8-', '-q50-s1-optimize'), pick('16x16-', '-q100-s0-rst3'),
           pick('17x33-', '-q90-s2-rstrow'), pick('33x50-', '-q1-s1-default'), pick('64x64-', '-q90-s2-optimize'),
           pick('64x64-L-', '-q50-default'), '33x50-own-s2', '33x50-comment-exif', '17x33-merged-s0']
  paths = []
  for i, n in enumerate(names):
    paths.append(str(d / ('%02d-%s%s' % (i, n, '.jpeg' if i % 4 == 3 else '.jpg'))))
    with open(paths[-1], 'wb') as f:
      f.write(by_name[n])
  pic = jpeg_host.contents(33, 50, seed=11)['smooth']
  paths.insert(3, str(d / 'progressive.jpg'))
  with open(paths[3], 'wb') as f:
    f.write(host.pil_encode(pic, quality=90, progressive=True))
  paths.insert(7, str(d / 'lossless.png'))
  Image.fromarray(pic, 'RGB').save(paths[7])
  return paths


@pytest.mark.parametrize('mode', (['--device-decode', '--png'], ['--fused-decode', '--device-png'],
                                  ['--fused-decode-curves', '--curve-steps', '16', '--device-png']), ids=lambda m: m[0])
def test_cli_writes_the_same_bytes_with_and_without_device_jpeg_decode(mode, cli_inputs, tmp_path, capsys):
  from exposure_amd import evaluate
  common = mode + ['--batch', '5', '--seed', '5']
  evaluate.main(common + ['--out', str(tmp_path / 'host') + os.sep] + cli_inputs)
  capsys.readouterr()
  evaluate.main(common + ['--device-jpeg-decode', '--out', str(tmp_path / 'device') + os.sep] + cli_inputs)
  err = capsys.readouterr().err
  lines = [l for l in err.splitlines() if l.startswith('--device-jpeg-decode')]
  assert len(lines) == 2  # one line per --batch group that holds a fallback
  assert 'progressive.jpg (progressive (SOF2))' in lines[0] and 'lossless.png (not a .jpg / .jpeg path)' in lines[1]
  written = sorted(os.listdir(str(tmp_path / 'host')))
  assert written == sorted(os.listdir(str(tmp_path / 'device'))) and len(written) >= 2 * len(cli_inputs)
  for name in written:
    a, b = (open(str(tmp_path / d / name), 'rb').read() for d in ('host', 'device'))
    assert a == b, name


@pytest.mark.parametrize('dtype', (torch.float16, torch.float32), ids=('f16', 'f32'))
def test_build_pack_from_device_decoded_jpegs_equals_the_host_decode_pack(dtype, tmp_path):
  from exposure_amd import datasets
  paths = []
  for i, ((h, w), kw) in enumerate((((80, 80), dict(subsampling=2)), ((81, 97), dict(subsampling=0, optimize=True)),
                                    ((100, 83), dict(subsampling=1, restart_marker_blocks=3)), ((96, 128), dict(subsampling=2, restart_marker_rows=1)),
                                    ((83, 131), dict(subsampling=2, progressive=True)), ((128, 85), dict(subsampling=1)),
                                    ((90, 90), None), ((85, 120), dict(subsampling=0, quality=100)))):
    pics = jpeg_host.contents(h, w, seed=1000 + i)
    paths.append(str(tmp_path / ('%d.jpg' % i)))
    with open(paths[-1], 'wb') as f:
      if kw is None:
        f.write(host.pil_encode(np.ascontiguousarray(pics['smooth'][..., 0]), 'L', quality=90))
      else:
        f.write(host.pil_encode(pics['smooth' if i % 2 else 'noise'], **dict(dict(quality=90), **kw)))
  plain, t_plain = {}, {}
  want = datasets.build_pack(paths, 'folder', dtype, DEV, seed=3, timings=plain)
  got = datasets.build_pack(paths, 'folder', dtype, DEV, seed=3, timings=t_plain, device_jpeg=True)
  assert got.dtype == want.dtype and got.shape == want.shape == (32, 64, 64, 3)
  assert torch.equal(got, want)
  assert set(t_plain) == {'read', 'device'}
  # chunks of three images: three decode calls, the same pack
  assert torch.equal(datasets.build_pack(paths, 'folder', dtype, DEV, seed=3, device_jpeg=True, max_images=3), want)
