"""GPU: expo_jpeg_decode_sync_ragged -- the device's pictures and status words against the NumPy
restatement of the decoder (tests/jpeg_decode_host.py) and its info words against the Python restatement of the
parallel walk's schedule (tests/jpeg_sync_host.py), never against the code under test; then the callers: the three
``sync`` modes of ``decode_jpeg_batch``, the CLI with and without --jpeg-serial-entropy, and the folder recipe's pack."""
import functools
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, jpeg_decode
from tests import jpeg_decode_host as host
from tests import jpeg_host
from tests import jpeg_sync_host as sync
from tests.test_hip_fused_decode import guarded, guards_intact

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
CACHE = {}


@functools.lru_cache(maxsize=None)
def parsed_of(data):
  return host.parse(data)


def want_info(data, sub_bytes, grid_rounds):
  """the restatement's info word: every (subsequence, entry) of a file is walked once for the whole module"""
  return sync.decode_sync(parsed_of(data), data, sub_bytes, 256, grid_rounds, cache=CACHE)['info']


def decode(datas, **kw):
  outs, statuses, info = jpeg_decode.decode_jpeg_batch(datas, DEV, info=True, **kw)
  return [o.cpu().numpy() for o in outs], statuses, info


@pytest.mark.parametrize('sub_bytes,grid_rounds', ((32, 4), (32, 0), (32, 1), (64, 4), (128, 4)))
def test_the_case_set_equals_the_restatements_bit_for_bit(sub_bytes, grid_rounds):
  files, want = host.case_files(), host.case_decoded()
  # ~400 files of mixed sizes, samplings, tables and restart intervals in one call (seven launch groups)
  got, statuses, info = decode([data for _, data in files], errors='return', sync=True, sub_bytes=sub_bytes, grid_rounds=grid_rounds)
  assert statuses == [0] * len(files)
  for (name, _), full, pic in zip(files, want, got):
    assert pic.shape == full['rgb'].shape and pic.dtype == np.uint8, name
    assert np.array_equal(pic, full['rgb']), (name, int(np.abs(pic.astype(int) - full['rgb'].astype(int)).max()))
  want_words = [want_info(data, sub_bytes, grid_rounds) for _, data in files]
  assert info == want_words, [(f[0], g, w) for f, g, w in zip(files, info, want_words) if g != w][:10]
  assert 1 in info and 0 in info and ((sub_bytes, grid_rounds) != (32, 0) or 2 in info)


def test_defaults_decode_every_default_input_through_verified_subsequences():
  """tests/test_jpeg_sync_host.py holds that the restatement alone gives info 1 for each of these at the defaults: an
  info 2 here is a broken sync hiding behind the fallback"""
  from tests.test_jpeg_sync_host import default_files
  cases = [c for c in default_files() if c[4] == 0]
  got, statuses, info = decode([c[1] for c in cases], sync=True)
  assert statuses == [0] * len(cases) and info == [1] * len(cases)
  for c, pic in zip(cases, got):
    assert np.array_equal(pic, host.decode(c[1])), c[0]


def test_noise_at_quality_100_crosses_waves_and_workgroups():
  pic = jpeg_host.contents(64, 64, seed=4242)['noise']
  data = host.pil_encode(pic, quality=100, subsampling=0)
  plan = jpeg_decode.parse(data)
  assert 400 <= plan.nsubs(32) <= 560  # two workgroups of 256 lanes, eight waves
  for grid_rounds in (0, 4):
    got, statuses, info = decode([data], sync=True, sub_bytes=32, grid_rounds=grid_rounds)
    assert statuses == [0] and info == [want_info(data, 32, grid_rounds)]
    assert np.array_equal(got[0], host.decode(data))
  assert want_info(data, 32, 4) == 1


def test_65_pictures_cross_the_launch_group():
  rng = np.random.default_rng(6)
  datas = [host.pil_encode(rng.integers(0, 256, (9 + i % 5, 17, 3), dtype=np.uint8), quality=90, subsampling=i % 3) for i in range(65)]
  got, statuses, info = decode(datas, sync=True, sub_bytes=32)
  assert statuses == [0] * 65 and info == [want_info(d, 32, jpeg_decode.GRID_ROUNDS) for d in datas] and set(info) == {1}
  for data, pic in zip(datas, got):
    assert np.array_equal(pic, host.decode(data))


def test_one_pixel_files_are_one_subsequence():
  rng = np.random.default_rng(5)
  datas = [host.pil_encode(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), quality=90, subsampling=i % 3) for i in range(9)]
  assert all(jpeg_decode.parse(d).nsubs(32) == 1 for d in datas)
  got, statuses, info = decode(datas, sync=True, sub_bytes=32)
  assert statuses == [0] * 9 and info == [0] * 9
  for data, pic in zip(datas, got):
    assert np.array_equal(pic, host.decode(data))


def test_restart_interval_plain_and_grey_files_mixed_in_one_call():
  by_name = dict(host.case_files())
  pick = lambda prefix, suffix: next(n for n in by_name if n.startswith(prefix) and n.endswith(suffix))
  names = [pick('33x50-', '-q90-s2-rst3'), pick('33x50-', '-q90-s0-default'), pick('64x64-L-', '-q100-default'), '8x1040-rst1',
           pick('64x64-L-', '-q50-optimize'), pick('17x33-', '-q50-s1-default'), pick('64x64-L-', '-q100-rst3'), '33x50-own-s2']
  datas = [by_name[n] for n in names]
  got, statuses, info = decode(datas, sync=True, sub_bytes=32)
  assert statuses == [0] * len(datas) and info == [0, 1, 1, 0, 1, 1, 0, 0]
  for n, data, pic in zip(names, datas, got):
    assert np.array_equal(pic, host.decode(data)), n


def raw_call(datas, plans, outs, status, info, sub_bytes, grid_rounds=4, workspace=None, file_off=0):
  """expo_jpeg_decode_sync_ragged on files uploaded one by one, `file_off` bytes into their buffers"""
  files = []
  for d in datas:
    buf = torch.zeros(len(d) + file_off + 16, dtype=torch.uint8, device=DEV)
    buf[file_off:file_off + len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(DEV)
    files.append(buf[file_off:file_off + len(d)])
  blobs = [torch.from_numpy(p.blob).to(DEV) for p in plans]
  _cabi.jpeg_decode_sync_ragged(files, blobs, [p.h for p in plans], [p.w for p in plans], [p.sampling for p in plans],
                                [p.ncomp for p in plans], [p.nsegs for p in plans], [p.nsubs(sub_bytes) for p in plans], sub_bytes,
                                grid_rounds, outs, status, info, workspace=workspace)
  return files, blobs


def test_malformed_files_set_their_status_and_touch_nothing_else():
  """ordinary malformed inputs that the kernels are built to bound (tools/jpeg_sync_rehearse.cpp walks the same files
  under AddressSanitizer): the statuses and info words are the restatements', the guards are intact, the good files are
  unaffected"""
  by_name = dict(host.case_files())
  good = [by_name['33x50-merged-s2'], by_name['8x1040-rst1'], by_name['17x33-merged-s0']]
  bad = [data for _, data in host.malformed_files()]
  datas = [good[0], bad[0], good[1], bad[1], bad[2], good[2]]
  want_status = [host.decode_full(d)['status'] for d in datas]
  assert want_status[0] == want_status[2] == want_status[5] == 0 and sorted(want_status[i] for i in (1, 3, 4)) == [1, 2, 4]
  plans = [jpeg_decode.parse(d) for d in datas]
  for sub_bytes in (32, 128):
    pairs = [guarded((p.h, p.w, 3), torch.uint8, off=1) for p in plans]
    need = jpeg_decode.workspace_bytes(plans, sub_bytes)
    wbuf, wsp = guarded((need,), torch.uint8)
    status = torch.full((6,), 77, dtype=torch.int32, device=DEV)
    info = torch.full((6,), 77, dtype=torch.int32, device=DEV)
    raw_call(datas, plans, [t for _, t in pairs], status, info, sub_bytes, workspace=wsp)
    torch.cuda.synchronize()  # the call returns
    assert status.cpu().tolist() == want_status
    assert info.cpu().tolist() == [want_info(d, sub_bytes, 4) for d in datas] and info.cpu().tolist()[1] == 1
    assert guards_intact(wbuf, wsp, torch.uint8)
    for i, (buf, t) in enumerate(pairs):
      assert guards_intact(buf, t, torch.uint8), i
      if want_status[i] == 0:
        assert np.array_equal(t.cpu().numpy(), host.decode(datas[i])), i


def test_odd_byte_offsets_and_a_dirtied_guarded_workspace_across_two_calls():
  by_name = dict(host.case_files())
  datas = [by_name[n] for n in by_name if n.startswith(('7x9-', '17x33-', '33x50-', '64x64-')) and
           n.endswith(('-q90-s0-default', '-q100-s1-optimize', '-q90-s2-rstrow', '-L-q50-default'))]
  assert len(datas) >= 12
  plans = [jpeg_decode.parse(d) for d in datas]
  want = [host.decode(d) for d in datas]
  need = jpeg_decode.workspace_bytes(plans, 32)
  wbuf, wsp = guarded((need,), torch.uint8)  # uninitialised for the library: full of the sentinel
  assert wsp.data_ptr() % 16 == 0
  for off in (1, 2, 3):
    pairs = [guarded((p.h, p.w, 3), torch.uint8, off=off) for p in plans]
    assert pairs[0][1].data_ptr() % 4 == off
    status = torch.empty((len(datas),), dtype=torch.int32, device=DEV)
    raw_call(datas, plans, [t for _, t in pairs], status, None, 32, workspace=wsp, file_off=off)  # no info words asked for
    assert status.cpu().tolist() == [0] * len(datas)
    for w, (buf, t) in zip(want, pairs):
      assert np.array_equal(t.cpu().numpy(), w), off
      assert guards_intact(buf, t, torch.uint8), off
    assert guards_intact(wbuf, wsp, torch.uint8)
    wsp.copy_(torch.randint(0, 256, (need,), dtype=torch.uint8, device=DEV))  # dirtied on purpose


def test_the_three_sync_modes_give_identical_tensors():
  by_name = dict(host.case_files())
  datas = [d for n, d in by_name.items() if n.startswith(('33x50-', '64x64-'))]
  plans = [jpeg_decode.parse(d) for d in datas]
  assert any(p.nsegs == 1 and p.segment_bytes >= jpeg_decode.SYNC_MIN_BYTES for p in plans)  # 'auto' takes the new call
  runs = {mode: decode(datas, sync=mode) for mode in ('auto', False, True)}
  assert runs['auto'][2] == runs[True][2] and 1 in runs[True][2] and set(runs[False][2]) == {0}
  small = [d for d, p in zip(datas, plans) if p.segment_bytes < jpeg_decode.SYNC_MIN_BYTES][:8]
  assert set(decode(small, sync='auto')[2]) == {0}  # 'auto' leaves a call of small files to the old entry
  for mode in ('auto', True):
    assert runs[mode][1] == runs[False][1] == [0] * len(datas)
    for a, b, full in zip(runs[mode][0], runs[False][0], [host.decode(d) for d in datas]):
      assert a.tobytes() == b.tobytes() == full.tobytes()
  outs, statuses = jpeg_decode.decode_jpeg_batch(datas[:3], DEV)  # without info: the two lists as before
  assert statuses == [0, 0, 0] and len(outs) == 3


# ------------------------------------------------------------------------------------------------------------ the callers
def test_cli_writes_the_same_bytes_with_and_without_jpeg_serial_entropy(tmp_path, capsys):
  from exposure_amd import evaluate
  by_name = dict(host.case_files())
  names = [n for n in by_name if n.startswith('64x64-') and n.endswith(('-q100-s0-default', '-q90-s2-optimize', '-q90-s1-rst3', '-L-q100-default'))]
  assert len(names) >= 4
  paths = []
  for i, n in enumerate(names):
    paths.append(str(tmp_path / ('%02d-%s.jpg' % (i, n))))
    with open(paths[-1], 'wb') as f:
      f.write(by_name[n])
  assert any(jpeg_decode.parse(by_name[n]).segment_bytes >= jpeg_decode.SYNC_MIN_BYTES for n in names)
  common = ['--fused-decode', '--device-jpeg-decode', '--device-png', '--batch', '3', '--seed', '5']
  evaluate.main(common + ['--out', str(tmp_path / 'sync') + os.sep] + paths)
  evaluate.main(common + ['--jpeg-serial-entropy', '--out', str(tmp_path / 'serial') + os.sep] + paths)
  capsys.readouterr()
  written = sorted(os.listdir(str(tmp_path / 'sync')))
  assert written == sorted(os.listdir(str(tmp_path / 'serial'))) and len(written) >= 2 * len(paths)
  for name in written:
    a, b = (open(str(tmp_path / d / name), 'rb').read() for d in ('sync', 'serial'))
    assert a == b, name


def test_build_pack_from_device_decoded_jpegs_equals_the_host_decode_pack(tmp_path):
  from exposure_amd import datasets
  paths = []
  for i, ((h, w), kw) in enumerate((((80, 80), dict(subsampling=2)), ((81, 97), dict(subsampling=0, optimize=True)),
                                    ((100, 83), dict(subsampling=1, restart_marker_blocks=3)), ((90, 90), None),
                                    ((85, 120), dict(subsampling=0, quality=100)))):
    pics = jpeg_host.contents(h, w, seed=2000 + i)
    paths.append(str(tmp_path / ('%d.jpg' % i)))
    with open(paths[-1], 'wb') as f:
      if kw is None:
        f.write(host.pil_encode(np.ascontiguousarray(pics['smooth'][..., 0]), 'L', quality=90))
      else:
        f.write(host.pil_encode(pics['smooth' if i % 2 else 'noise'], **dict(dict(quality=90), **kw)))
  assert any(jpeg_decode.parse(open(p, 'rb').read()).segment_bytes >= jpeg_decode.SYNC_MIN_BYTES for p in paths)
  want = datasets.build_pack(paths, 'folder', torch.float16, DEV, seed=3)
  assert torch.equal(datasets.build_pack(paths, 'folder', torch.float16, DEV, seed=3, device_jpeg=True), want)
  assert torch.equal(datasets.build_pack(paths, 'folder', torch.float16, DEV, seed=3, device_jpeg=True, jpeg_sync=False), want)
