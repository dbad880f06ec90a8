"""CPU: the parallel entropy decoding of files without restart markers through its Python restatement
(tests/jpeg_sync_host.py) -- the restatement against the serial restatement's coefficients over a grid of subsequence
sizes, workgroup sizes and grid rounds, the malformed files and the good_blocks rule, the coverage the GPU test's inputs
must have, ``Plan.nsubs`` and the workspace arithmetic, every refusal of the entry point, and
tools/jpeg_sync_rehearse.cpp under the sanitizers against the restatement."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from exposure_amd import _cabi, jpeg_decode
from tests import jpeg_decode_host as host
from tests import jpeg_sync_host as sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
FAKE = 0x1000  # never dereferenced on the host


@functools.lru_cache(maxsize=None)
def one_segment_cases():
  """[(name, data, parsed, the serial restatement's coefficients and status)] of the case set's files without restart
  markers and of the three malformed files, computed once"""
  out = []
  for name, data in host.case_files() + host.malformed_files():
    parsed = host.parse(data)
    if len(parsed['segments']) == 1:
      out.append((name, data, parsed) + host.decode_coefficients(parsed, data)[:2])
  return out


CACHE = {}  # the cut files by (parsed, sub_bytes): every (subsequence, entry) is walked once for the whole module


def run(case, sub_bytes, W=256, grid_rounds=4):
  return sync.decode_sync(case[2], case[1], sub_bytes, W, grid_rounds, cache=CACHE)


def test_one_subsequence_over_the_whole_segment_is_the_serial_walk():
  """``walk`` and ``emit`` on a subsequence that covers the segment: the coefficients and the status of the serial
  restatement, the malformed files included (the scan's rules turn the walk's exit into the status)"""
  for name, data, parsed, coef, status in one_segment_cases():
    begin, end = parsed['segments'][0]
    f = sync.SyncFile(parsed, data, max(32, -(-(end - begin) // 16) * 16))
    assert f.n == 1, name
    exit_state = f.walk(0, sync.START)[0]
    verdict = sync.scan(f, [sync.START], [exit_state])
    assert verdict['settled'] and verdict['status'] == status, name
    assert np.array_equal(sync.emit(f, [sync.START], verdict), coef), name


@pytest.mark.parametrize('sub_bytes', (32, 64, 128))
def test_grid_of_workgroups_and_rounds_equals_the_serial_coefficients(sub_bytes):
  cases = one_segment_cases()
  assert len(cases) >= 150
  seen = set()
  for case in cases:
    for W in (64, 256):
      for grid_rounds in (0, 1, 4):
        got = run(case, sub_bytes, W, grid_rounds)
        assert np.array_equal(got['coef'], case[3]) and got['status'] == case[4], (case[0], W, grid_rounds)
        assert (got['info'] == 0) == (got['nsubs'] == 1) and got['info'] in (0, 1, 2)
        seen.add(got['info'])
  assert seen >= {0, 1} and (sub_bytes != 32 or 2 in seen)  # the fallback is taken at 32 bytes with few rounds


def test_malformed_files_give_the_serial_statuses_and_cut_exercises_good_blocks():
  bad = {c[0]: c for c in one_segment_cases() if c[0] in ('cut', 'ones', 'random')}
  assert sorted(c[4] for c in bad.values()) == [host.TRUNCATED, host.BAD_CODE, host.BAD_RUN]
  for name, case in bad.items():
    for sub_bytes in (32, 128):
      got = run(case, sub_bytes)
      assert got['info'] == 1 and got['status'] == case[4] and np.array_equal(got['coef'], case[3]), (name, sub_bytes)
  got = run(bad['cut'], 32)
  verdict, f = got['verdict'], got['file']
  blocks = f.parsed['mcus'] * f.bpm
  assert 0 < verdict['good_blocks'] < blocks and got['outs'][verdict['last']] == sync.DEAD  # an error before the count is reached
  # the block the error struck was partly read -- the emitting walk meets its coefficients -- and is left all-zero
  last = verdict['last']
  struck = [ev for ev in f.walk(last, got['ins'][last])[4] if verdict['first_block'][last] + ev[0] == verdict['good_blocks']]
  earlier = got['ins'][last][2] > 0 and f.walk(last, got['ins'][last])[1] == 0
  assert struck or earlier
  assert not got['coef'].reshape(-1, 64)[verdict['good_blocks']:].any()
  assert got['coef'].reshape(-1, 64)[verdict['good_blocks'] - 1].any()


def test_padding_bits_behind_the_last_block_are_no_error():
  """the walk of the last subsequence reads the padding, which the serial lane never does: a dead exit there leaves
  the status 0 and good_blocks at the picture's count"""
  met_dead = 0
  for case in one_segment_cases():
    if case[4]:
      continue
    got = run(case, 32)
    if got['info'] != 1:
      continue
    f, verdict = got['file'], got['verdict']
    assert verdict['good_blocks'] == f.parsed['mcus'] * f.bpm and verdict['status'] == 0
    met_dead += got['outs'][verdict['last']] == sync.DEAD
  assert met_dead


def test_coverage_of_the_case_set_at_32_bytes():
  """asserted on the restatement alone: what the GPU test's files at sub_bytes 32 make the kernels meet"""
  met = dict(dropped=0, ends_ff=0, three=0, no_block=0, k_entry=0, crosses=0, later=0)
  for case in one_segment_cases():
    got = run(case, 32)
    if got['info'] != 1 or case[4]:
      continue
    f, ins = got['file'], got['ins']
    met['dropped'] += any(f.first_dropped)
    met['ends_ff'] += any(f.last_is_ff[:-1])
    ended = [f.walk(i, ins[i])[1] for i in range(f.n)]
    met['no_block'] += any(n == 0 for n in ended[:-1])
    met['k_entry'] += any(s[2] > 0 for s in ins)
    # a block that starts before subsequence i, ends in none of it and goes on behind it spans at least three
    three = any(ended[i] == 0 and ins[i][2] > 0 and got['outs'][i] != sync.DEAD and got['outs'][i][2] > 0 for i in range(1, f.n - 1))
    met['three'] += three and 'noise-q100' in case[0]
    met['crosses'] += f.n > 256
    met['later'] += f.n > 256 and run(case, 32, 256, 0)['info'] == 2  # settled by a later launch only
  assert all(met.values()), met


def default_files():
  """the inputs of the GPU test at the default parameters: the case set's and the malformed files without restart
  markers of more than one default subsequence"""
  return [c for c in one_segment_cases() if sync.nsubs_of(c[2]['segments'][0][1] - c[2]['segments'][0][0], jpeg_decode.SUB_BYTES) > 1]


def test_defaults_settle_every_default_input():
  """GRID_ROUNDS caps what may hide behind the fallback: with the defaults the restatement alone reports info 1 for
  every input of tests/test_hip_jpeg_sync.py's default-parameter test, so an info 2 on the device is a broken sync"""
  assert (jpeg_decode.SUB_BYTES, jpeg_decode.GRID_ROUNDS, jpeg_decode.SYNC_MIN_BYTES) == (128, 4, 4096)
  files = default_files()
  assert len(files) >= 60
  for case in files:
    assert run(case, jpeg_decode.SUB_BYTES, 256, jpeg_decode.GRID_ROUNDS)['info'] == 1, case[0]
  # 'auto' takes the new call for at least one case file and leaves it for others
  sizes = [jpeg_decode.parse(c[1]).segment_bytes for c in one_segment_cases()]
  assert max(sizes) >= jpeg_decode.SYNC_MIN_BYTES > min(sizes)
  # one file needs a later launch: info 2 without grid rounds, 1 with the default
  late = [c for c in one_segment_cases() if run(c, 32, 256, 0)['info'] == 2]
  assert late and all(run(c, 32, 256, jpeg_decode.GRID_ROUNDS)['info'] == 1 for c in late)


# ---------------------------------------------------------------------------------------- the plan and the workspace
def align16(v):
  return (v + 15) // 16 * 16


def sync_bytes(nsubs):
  return 2 * align16(4 * nsubs) + 32 * nsubs + align16(8 * (-(-nsubs // 256))) + 16


def test_plan_nsubs_and_the_workspace_arithmetic():
  by_name = dict(host.case_files())
  name = next(n for n in by_name if n.startswith('64x64-noise-q100-s0'))
  plan = jpeg_decode.parse(by_name[name])
  length = int(plan.segments[0, 1] - plan.segments[0, 0])
  assert plan.nsegs == 1 and plan.segment_bytes == length
  for b in (32, 48, 128, 4096):
    assert plan.nsubs(b) == -(-length // b)
  assert plan.nsubs(65536) == 1 and plan.nsubs(length) == 1 and plan.nsubs(-(-length // 16) * 16 - 16) == 2
  rst = jpeg_decode.parse(by_name['8x1040-rst1'])
  assert rst.nsegs == 130 and rst.segment_bytes == 0 and rst.nsubs(32) == 1
  tiny = jpeg_decode.parse(next(d for n, d in by_name.items() if n.startswith('1x1-') and n.endswith('-default')))
  assert tiny.nsubs(32) == 1  # an empty or short segment is one subsequence
  old = jpeg_decode.workspace_bytes([plan, rst, tiny])
  assert jpeg_decode.workspace_bytes([plan, rst, tiny], 65536) == old  # no sync picture: the old call's layout
  for b in (32, 128):
    assert jpeg_decode.workspace_bytes([plan, rst, tiny], b) == old + sync_bytes(plan.nsubs(b))
    assert jpeg_decode.workspace_bytes([plan, plan], b) == jpeg_decode.workspace_bytes([plan, plan]) + 2 * sync_bytes(plan.nsubs(b))
  # the largest launch group's sum: 64 plain pictures and a sync picture in the second group
  group = [tiny] * 64 + [plan]
  assert jpeg_decode.workspace_bytes(group, 32) == max(jpeg_decode.workspace_bytes([tiny] * 64), jpeg_decode.workspace_bytes([plan], 32))
  lib = _cabi.load()
  one = (ctypes.c_int * 1)
  assert lib.expo_jpeg_decode_sync_workspace_bytes(one(16), one(16), one(0), one(3), one(1), one(0), 1) == 0
  assert lib.expo_jpeg_decode_sync_workspace_bytes(one(16), one(16), one(0), one(3), one(2), one(2), 1) == 0  # nsubs 2 with restart intervals
  assert lib.expo_jpeg_decode_sync_workspace_bytes(one(16), one(16), one(0), one(3), one(1), one((1 << 26) + 1), 1) == 0
  assert lib.expo_jpeg_decode_sync_workspace_bytes(one(16), one(16), one(0), one(3), one(1), one(3), 1) == 12 * 128 + 3 * 256 + sync_bytes(3)
  assert lib.expo_jpeg_decode_sync_workspace_bytes(None, None, None, None, None, None, 1) == 0


# ------------------------------------------------------------------------------------------------------ the ABI surface
def ints(*v):
  return (ctypes.c_int * len(v))(*v)


def ptrs(*v):
  return (vp * len(v))(*v)


def call(lib, files=None, file_bytes=None, plans=None, hs=None, ws=None, samplings=None, ncomps=None, nsegs=None, nsubs=None,
         n=1, sub_bytes=128, grid_rounds=4, outs=None, status=FAKE, info=FAKE, workspace=FAKE, workspace_bytes=1 << 30):
  files = ptrs(FAKE) if files is None else files
  plans = ptrs(FAKE) if plans is None else plans
  outs = ptrs(FAKE) if outs is None else outs
  file_bytes = (ctypes.c_int64 * 1)(700) if file_bytes is None else file_bytes
  hs, ws = ints(16) if hs is None else hs, ints(16) if ws is None else ws
  samplings, ncomps = ints(0) if samplings is None else samplings, ints(3) if ncomps is None else ncomps
  nsegs, nsubs = ints(1) if nsegs is None else nsegs, ints(5) if nsubs is None else nsubs
  return lib.expo_jpeg_decode_sync_ragged(files, file_bytes, plans, hs, ws, samplings, ncomps, nsegs, nsubs, n, sub_bytes,
                                          grid_rounds, outs, vp(status), vp(info), vp(workspace), workspace_bytes, None)


def test_validation_before_enqueue():
  """every failing call below would otherwise dereference fake device pointers"""
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  for name in ('expo_jpeg_decode_sync_workspace_bytes', 'expo_jpeg_decode_sync_ragged'):
    assert name in _cabi.SIGNATURES and hasattr(ctypes.CDLL(_cabi.LIB_PATH), name)
  assert lib.expo_version() == 9
  assert call(lib, n=-1) == -1
  assert lib.expo_jpeg_decode_sync_ragged(None, None, None, None, None, None, None, None, None, 0, 128, 4, None, None, None, None, 0, None) == 0
  for bad in (0, 16, 40, 120, 65552, -128):
    assert call(lib, sub_bytes=bad) == -1 and b'sub_bytes' in err()
  for bad in (-1, 17):
    assert call(lib, grid_rounds=bad) == -1 and b'grid_rounds' in err()
  assert call(lib, hs=ints(0)) == -1 and b'65535' in err()
  assert call(lib, ws=ints(65536)) == -1 and b'65535' in err()
  assert call(lib, samplings=ints(3)) == -1 and b'sampling' in err()
  assert call(lib, ncomps=ints(2)) == -1 and b'ncomps' in err()
  assert call(lib, ncomps=ints(1), samplings=ints(2)) == -1 and b'grey' in err()
  assert call(lib, nsegs=ints(0)) == -1 and b'nsegs' in err()
  assert call(lib, nsegs=ints(5)) == -1 and b'nsegs' in err()  # 4 MCUs
  assert call(lib, file_bytes=(ctypes.c_int64 * 1)(1 << 31)) == -1 and b'file_bytes' in err()
  assert call(lib, file_bytes=(ctypes.c_int64 * 1)(-1)) == -1 and b'file_bytes' in err()
  assert call(lib, nsubs=ints(0)) == -1 and b'nsubs' in err()
  assert call(lib, nsubs=ints((1 << 26) + 1)) == -1 and b'nsubs' in err()
  assert call(lib, nsegs=ints(2), nsubs=ints(2)) == -1 and b'restart' in err()
  assert lib.expo_jpeg_decode_sync_ragged(ptrs(FAKE), (ctypes.c_int64 * 1)(700), ptrs(FAKE), ints(16), ints(16), ints(0), ints(3), ints(1),
                                          None, 1, 128, 4, ptrs(FAKE), vp(FAKE), None, vp(FAKE), 1 << 30, None) == -1 and b'null' in err()
  assert call(lib, files=ptrs(None)) == -1 and b'null' in err()
  assert call(lib, plans=ptrs(None)) == -1 and b'null' in err()
  assert call(lib, outs=ptrs(None)) == -1 and b'null' in err()
  assert call(lib, status=None) == -1 and b'null' in err()
  assert call(lib, plans=ptrs(FAKE + 8)) == -1 and b'aligned' in err()
  need = 12 * 128 + 3 * 256 + sync_bytes(5)
  assert call(lib, workspace_bytes=need - 1) == -1 and b'too small' in err()
  assert call(lib, workspace=None, workspace_bytes=need) == -1 and b'null workspace' in err()
  assert call(lib, workspace=FAKE + 4, workspace_bytes=need) == -1 and b'aligned' in err()
  # the second picture's fault is found before the first is enqueued
  assert call(lib, files=ptrs(FAKE, FAKE), file_bytes=(ctypes.c_int64 * 2)(700, 700), plans=ptrs(FAKE, FAKE), hs=ints(16, 16), ws=ints(16, 16),
              samplings=ints(0, 0), ncomps=ints(3, 3), nsegs=ints(1, 1), nsubs=ints(5, 0), n=2, outs=ptrs(FAKE, FAKE)) == -1 and b'nsubs' in err()


def test_python_side_refuses_what_it_can_see():
  with pytest.raises(ValueError, match='sync'):
    jpeg_decode.decode_jpeg_batch([b'x'], 'cpu', sync='yes')
  assert jpeg_decode.decode_jpeg_batch([], 'cpu', info=True) == ([], [], [])
  with pytest.raises(_cabi.ExposureHipError, match='same length'):
    _cabi.jpeg_decode_sync_ragged([1], [], [], [], [], [], [], [], 128, 4, [], None)


# ---------------------------------------------------------------------------------------------------------- the rehearsal
def test_rehearsal_program_under_sanitizers(tmp_path):
  """tools/jpeg_sync_rehearse.cpp: the kernels' serial routines (csrc/jpeg_decode_sync.h) and the launches' phases on the
  host, a stand-alone program built with AddressSanitizer and UBSan, every buffer of exactly the size the ABI reports:
  its self-test; its pictures, status words and info words equal to the restatement's on the whole case set and the
  malformed files, at 32 bytes with and without grid rounds and at the defaults, with the sanitizers silent"""
  cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
  if cxx is None:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'jpeg_sync_rehearse')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(ROOT, 'tools', 'jpeg_sync_rehearse.cpp'), '-o', exe])
  assert subprocess.run([exe, 'selftest'], stdout=subprocess.PIPE).stdout.decode().strip() == 'jpeg_sync_rehearse selftest: ok'
  files = host.case_files() + host.malformed_files()
  serial = host.case_decoded() + [host.decode_full(d) for _, d in host.malformed_files()]
  by_name = {c[0]: c for c in one_segment_cases()}
  args = []
  for i, (name, data) in enumerate(files):
    plan = jpeg_decode.parse(data)
    (tmp_path / ('%d.jpg' % i)).write_bytes(data)
    plan.blob.tofile(str(tmp_path / ('%d.plan' % i)))
    args += [str(tmp_path / ('%d.jpg' % i)), str(tmp_path / ('%d.plan' % i)), str(plan.h), str(plan.w), str(plan.sampling),
             str(plan.ncomp), str(plan.nsegs), str(tmp_path / ('%d.rgb' % i))]
  infos = set()
  for sub_bytes, grid_rounds in ((32, 0), (32, 4), (jpeg_decode.SUB_BYTES, jpeg_decode.GRID_ROUNDS)):
    want = [(full['status'], run(by_name[name], sub_bytes, 256, grid_rounds)['info'] if name in by_name else 0)
            for (name, _), full in zip(files, serial)]
    proc = subprocess.run([exe, 'decode', str(sub_bytes), str(grid_rounds)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert proc.returncode == 0 and proc.stderr == b'', proc.stderr.decode()[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in proc.stdout.decode().splitlines()]
    assert got == want, [(f[0], g, w) for f, g, w in zip(files, got, want) if g != w][:10]
    infos |= {g[1] for g in got}
    assert [g[0] for g in got[-3:]] != [0, 0, 0]
    for i, ((name, _), full) in enumerate(zip(files, serial)):
      if full['status'] == 0:  # the pixels of a picture with a status are unspecified
        pic = np.fromfile(str(tmp_path / ('%d.rgb' % i)), np.uint8).reshape(full['rgb'].shape)
        assert np.array_equal(pic, full['rgb']), (name, sub_bytes, grid_rounds)
  assert infos == {0, 1, 2}
