"""CPU: the device JPEG decoder of DESIGN.md §3.35 through its NumPy restatement (tests/jpeg_decode_host.py) -- the
restatement against PIL bit for bit on the whole case set, the product's parser against the restatement's, every refusal,
the coverage the GPU test's case set must have, the host side of the three entry points, and
tools/jpeg_decode_rehearse.cpp under the sanitizers against the restatement, the malformed files included."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from exposure_amd import _cabi, jpeg_decode
from tests import jpeg_decode_host as host
from tests import jpeg_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
FAKE = 0x1000  # never dereferenced on the host


def test_restatement_equals_pil_bit_for_bit():
  files, decoded = host.case_files(), host.case_decoded()
  assert len(files) >= 7 * 4 * 3 * 4
  worst = []
  for (name, data), full in zip(files, decoded):
    want = host.pil_decode(data)
    assert full['status'] == 0 and full['rgb'].shape == want.shape, name
    diff = int(np.abs(full['rgb'].astype(np.int64) - want.astype(np.int64)).max())
    if diff:
      worst.append((name, diff))
  assert not worst, 'this Pillow build differs from the restatement on (case, largest difference): %r' % worst[:20]


def test_case_set_holds_what_the_issue_lists():
  names = [name for name, _ in host.case_files()]
  for shape in host.SHAPES:
    for quality in host.QUALITIES:
      for sub in (0, 1, 2):
        for variant, _ in host.VARIANTS:
          assert any(n.startswith('%dx%d-' % shape) and n.endswith('-q%d-s%d-%s' % (quality, sub, variant)) for n in names)
    assert any(n.startswith('%dx%d-L-' % shape) for n in names) and '%dx%d-own-s0' % shape in names and '%dx%d-own-s2' % shape in names
  by_name = dict(zip(names, host.case_decoded()))
  assert len(by_name['8x1040-rst1']['parsed']['segments']) == 130 and by_name['8x1040-rst1']['parsed']['ri'] == 1
  assert b'a comment' in dict(host.case_files())['33x50-comment-exif'] and b'Exif' in dict(host.case_files())['33x50-comment-exif']
  for name in ('33x50-merged-s2', '17x33-merged-s0'):
    data = dict(host.case_files())[name]
    assert data.count(b'\xff\xdb') == 1 and data.count(b'\xff\xc4') == 1 and by_name[name]['status'] == 0
  assert by_name['16x16-own-s0']['parsed']['ri'] == 16 and by_name['16x16-own-s2']['parsed']['ri'] == 8
  assert by_name['64x64-L-q50-default']['parsed']['ncomp'] == 1


def test_coverage_of_the_case_set():
  """on the restatement alone: what the decoder's paths need is in the files"""
  names = [name for name, _ in host.case_files()]
  met = [d['met'] for d in host.case_decoded()]
  total = lambda key: sum(m[key] for m in met)
  assert max(m['longest'] for m in met) == 16  # a 16-bit code is decoded (from Annex K's tables)
  # the longest code these small pictures' optimised tables reach is 13 bits (Pillow 12.2.0 with libjpeg-turbo); the
  # loop over the lengths is the same one that reaches 16 above, behind tables built by the same parse
  assert max(m['longest'] for n, m in zip(names, met) if n.endswith('-optimize')) >= 13
  assert total('zrl') > 0 and total('eob') > 0 and total('last') > 0 and total('stuffed') > 0 and total('resets') > 0
  for sub, keys in ((1, ('left', 'right', 'inner_x')), (2, ('left', 'right', 'inner_x', 'up', 'down', 'inner_y'))):
    for key in keys:
      assert any(m.get(key) for d, m in zip(host.case_decoded(), met) if d['parsed']['sampling'] == sub and d['parsed']['ncomp'] == 3), (sub, key)
  assert any(m.get('below') for m in met) and any(m.get('above') for m in met)  # colour clamped at 0 and at 255
  # the upsampling's clamp really replicates: a one-sample chroma plane gives that sample everywhere
  one = np.array([[77]])
  assert (host.upsample(one, 2, 2, 2) == 77).all() and (host.upsample(one, 1, 1, 2) == 77).all()


def test_parse_returns_the_restatements_fields():
  for (name, data), full in zip(host.case_files() + host.malformed_files(),
                                host.case_decoded() + [host.decode_full(d) for _, d in host.malformed_files()]):
    want, got = full['parsed'], jpeg_decode.parse(data)
    assert (got.h, got.w, got.ncomp, got.sampling, got.ri) == (want['h'], want['w'], want['ncomp'], want['sampling'], want['ri']), name
    assert got.segments.tolist() == [list(s) for s in want['segments']], name
    assert got.comps == want['comps'] and got.nbytes == len(data) and got.mcus == want['mcus'], name
    assert sorted(got.quant) == sorted(want['quant']) and all((got.quant[k] == want['quant'][k]).all() for k in got.quant), name
    assert got.huff == want['huff'], name
    assert got.blob.size == _cabi.jpeg_decode_plan_bytes(got.nsegs) and got.blob.dtype == np.uint8, name
    # the plan's Huffman arrays against T.81 Annex C, table by table
    for (cls, ident), (bits, vals) in want['huff'].items():
      o = 272 + 384 * (2 * cls + ident)
      limit, offs = got.blob[o:o + 64].view('<u4'), got.blob[o + 64:o + 128].view('<i4')
      codes = jpeg_host.canonical_codes(bits, vals)
      for sym, (code, length) in codes.items():
        window = code << (16 - length)
        first = next(l for l in range(1, 17) if window < limit[l - 1])
        assert first == length and got.blob[o + 128 + ((code + offs[length - 1]) & 255)] == sym, (name, cls, ident, sym)


def _segments(data):
  """[(offset, marker, length)] up to SOS"""
  out, at = [], 2
  while True:
    marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], 'big')
    out.append((at, marker, length))
    at += 2 + length
    if marker == 0xDA:
      return out


def _patch(data, marker, offset, value, nth=0):
  at = [s for s in _segments(data) if s[1] == marker][nth][0]
  out = bytearray(data)
  out[at + 4 + offset] = value
  return bytes(out)


def test_every_refusal():
  pic = jpeg_host.contents(33, 50, seed=5)['smooth']
  good = host.pil_encode(pic, quality=90, subsampling=2)
  jpeg_decode.parse(good)
  sof = [s for s in _segments(good) if s[1] == 0xC0][0][0]
  remark = lambda m: good[:sof + 1] + bytes([m]) + good[sof + 2:]
  dht = [s for s in _segments(good) if s[1] == 0xC4]
  adobe = b'\xff\xee' + (14).to_bytes(2, 'big') + b'Adobe' + bytes([0, 100, 0, 0, 0, 0, 0])
  buf = io.BytesIO()
  Image.fromarray(np.dstack([pic, pic[..., :1]]), 'CMYK').save(buf, 'JPEG')
  cases = {
      'progressive': (host.pil_encode(pic, quality=90, progressive=True), 'progressive'),
      'cmyk': (buf.getvalue(), '4 components'),
      'sof1': (remark(0xC1), 'SOF1'),
      'arithmetic': (remark(0xC9), 'arithmetic'),
      'lossless': (remark(0xC3), 'lossless'),
      '12-bit': (_patch(good, 0xC0, 0, 12), '12-bit samples'),
      '16-bit dqt': (_patch(good, 0xDB, 0, 0x10), '16-bit quantiser'),
      'adobe rgb': (good[:2] + adobe + good[2:], 'Adobe'),
      'sampling y': (_patch(good, 0xC0, 7, 0x41), 'sampling'),
      'sampling cb': (_patch(good, 0xC0, 10, 0x21), 'sampling'),
      'two scans': (_patch(good, 0xDA, 0, 1), 'more than one scan'),
      'dnl': (_patch(_patch(good, 0xC0, 1, 0), 0xC0, 2, 0), 'DNL'),
      'missing table': (good[:dht[-1][0]] + good[dht[-1][0] + 2 + dht[-1][2]:], 'no segment defines'),
      'spectral selection': (_patch(good, 0xDA, 8, 5), 'sequential'),
      'not a jpeg': (b'\x89PNG\r\n\x1a\n' + bytes(32), 'SOI'),
      'marker in the scan': (good[:-2] + b'\xff\xd3' + b'\x00' * 4 + b'\xff\xd9', 'inside the scan'),
      'bytes behind eoi': (good + b'\0', 'behind EOI'),
  }
  for name, (data, reason) in cases.items():
    with pytest.raises(jpeg_decode.UnsupportedJpeg, match=reason):
      jpeg_decode.parse(data)
    if name not in ('not a jpeg',):
      with pytest.raises(host.Refused):
        host.parse(data)
  assert issubclass(jpeg_decode.UnsupportedJpeg, ValueError)


def test_statuses_of_the_malformed_files():
  full = {name: host.decode_full(data) for name, data in host.malformed_files()}
  assert full['cut']['status'] == host.TRUNCATED
  assert full['ones']['status'] == host.BAD_CODE  # sixteen 1-bits are no code of Annex K's tables
  assert full['random']['status'] in (host.TRUNCATED, host.BAD_CODE, host.BAD_RUN)  # one lane: it stops at its first error
  assert {f['status'] for f in full.values()} == {host.TRUNCATED, host.BAD_CODE, host.BAD_RUN}
  assert (jpeg_decode.TRUNCATED, jpeg_decode.BAD_CODE, jpeg_decode.BAD_RUN) == (host.TRUNCATED, host.BAD_CODE, host.BAD_RUN)
  assert jpeg_decode.status_text(5) == 'TRUNCATED|BAD_RUN' and jpeg_decode.status_text(0) == 'OK'


def test_rehearsal_program_under_sanitizers(tmp_path):
  """tools/jpeg_decode_rehearse.cpp: the kernels' serial routines (csrc/jpeg_decode.h) and phases on the host, a
  stand-alone program built with AddressSanitizer and UBSan, every buffer of exactly the size the ABI reports: its
  self-test, its pictures equal to the restatement's on the whole case set, and on the malformed files the
  restatement's statuses with the sanitizers silent"""
  cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
  if cxx is None:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'jpeg_decode_rehearse')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(ROOT, 'tools', 'jpeg_decode_rehearse.cpp'), '-o', exe])
  assert subprocess.run([exe, 'selftest'], stdout=subprocess.PIPE).stdout.decode().strip() == 'jpeg_decode_rehearse selftest: ok'
  files = host.case_files() + host.malformed_files()
  want = host.case_decoded() + [host.decode_full(d) for _, d in host.malformed_files()]
  args = []
  for i, (name, data) in enumerate(files):
    plan = jpeg_decode.parse(data)
    (tmp_path / ('%d.jpg' % i)).write_bytes(data)
    plan.blob.tofile(str(tmp_path / ('%d.plan' % i)))
    args += [str(tmp_path / ('%d.jpg' % i)), str(tmp_path / ('%d.plan' % i)), str(plan.h), str(plan.w), str(plan.sampling),
             str(plan.ncomp), str(plan.nsegs), str(tmp_path / ('%d.rgb' % i))]
  run = subprocess.run([exe, 'decode'] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
  assert run.returncode == 0 and run.stderr == b'', run.stderr.decode()[-2000:]
  statuses = [int(s) for s in run.stdout.split()]
  assert statuses == [full['status'] for full in want]
  assert statuses[-3:] != [0, 0, 0]
  for i, ((name, _), full) in enumerate(zip(files, want)):
    if full['status'] == 0:  # the pixels of a picture with a status are unspecified
      got = np.fromfile(str(tmp_path / ('%d.rgb' % i)), np.uint8).reshape(full['rgb'].shape)
      assert np.array_equal(got, full['rgb']), name


# ------------------------------------------------------------------------------------------------------ the ABI surface
def ints(*v):
  return (ctypes.c_int * len(v))(*v)


def ptrs(*v):
  return (vp * len(v))(*v)


def call(lib, files=None, file_bytes=None, plans=None, hs=None, ws=None, samplings=None, ncomps=None, nsegs=None, n=1,
         outs=None, status=FAKE, workspace=FAKE, workspace_bytes=1 << 30):
  files = ptrs(FAKE) if files is None else files
  plans = ptrs(FAKE) if plans is None else plans
  outs = ptrs(FAKE) if outs is None else outs
  file_bytes = (ctypes.c_int64 * 1)(700) if file_bytes is None else file_bytes
  hs, ws = ints(16) if hs is None else hs, ints(16) if ws is None else ws
  samplings, ncomps, nsegs = ints(0) if samplings is None else samplings, ints(3) if ncomps is None else ncomps, ints(1) if nsegs is None else nsegs
  return lib.expo_jpeg_decode_ragged(files, file_bytes, plans, hs, ws, samplings, ncomps, nsegs, n, outs, vp(status),
                                     vp(workspace), workspace_bytes, None)


def test_validation_before_enqueue():
  """every failing call below would otherwise dereference fake device pointers"""
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  for name in ('expo_jpeg_decode_plan_bytes', 'expo_jpeg_decode_workspace_bytes', 'expo_jpeg_decode_ragged'):
    assert name in _cabi.SIGNATURES and hasattr(ctypes.CDLL(_cabi.LIB_PATH), name)
  assert lib.expo_version() == 9
  assert call(lib, n=-1) == -1
  assert lib.expo_jpeg_decode_ragged(None, None, None, None, None, None, None, None, 0, None, None, None, 0, None) == 0  # no-op
  assert call(lib, hs=ints(0)) == -1 and b'65535' in err()
  assert call(lib, ws=ints(65536)) == -1 and b'65535' in err()
  assert call(lib, samplings=ints(3)) == -1 and b'sampling' in err()
  assert call(lib, samplings=ints(-1)) == -1
  assert call(lib, ncomps=ints(4)) == -1 and b'ncomps' in err()
  assert call(lib, ncomps=ints(1), samplings=ints(2)) == -1 and b'grey' in err()
  # 16 x 16 in 4:4:4 is 4 MCUs: 1, 2 and 4 segments are ceil(4 / Ri), 0, 3 and 5 are not
  for k, ok in ((0, False), (1, True), (2, True), (3, False), (4, True), (5, False)):
    if not ok:
      assert call(lib, nsegs=ints(k)) == -1 and b'nsegs' in err(), k
  assert call(lib, file_bytes=(ctypes.c_int64 * 1)(-1)) == -1 and b'file_bytes' in err()
  assert call(lib, file_bytes=(ctypes.c_int64 * 1)(1 << 31)) == -1
  for kw in (dict(files=ctypes.cast(None, ctypes.POINTER(vp))), dict(plans=ctypes.cast(None, ctypes.POINTER(vp))),
             dict(outs=ctypes.cast(None, ctypes.POINTER(vp))), dict(status=None), dict(hs=ctypes.cast(None, ctypes.POINTER(ctypes.c_int)))):
    assert call(lib, **kw) == -1 and b'null' in err(), kw
  assert call(lib, files=ptrs(None)) == -1 and b'null picture' in err()
  assert call(lib, outs=ptrs(None)) == -1 and call(lib, plans=ptrs(None)) == -1
  assert call(lib, plans=ptrs(FAKE + 8)) == -1 and b'aligned' in err()
  need = lib.expo_jpeg_decode_workspace_bytes(ints(16), ints(16), ints(0), ints(3), 1)
  assert call(lib, workspace=None) == -1 and b'workspace' in err()
  assert call(lib, workspace=FAKE + 8) == -1 and b'workspace' in err()
  assert call(lib, workspace_bytes=need - 1) == -1 and b'workspace' in err()
  # a bad entry in the last picture is found before anything is enqueued
  assert call(lib, n=2, files=ptrs(FAKE, FAKE), plans=ptrs(FAKE, FAKE), outs=ptrs(FAKE, None), hs=ints(16, 16), ws=ints(16, 16),
              samplings=ints(0, 0), ncomps=ints(3, 3), nsegs=ints(1, 1), file_bytes=(ctypes.c_int64 * 2)(700, 700)) == -1


def test_plan_and_workspace_bytes():
  lib = _cabi.load()
  assert [lib.expo_jpeg_decode_plan_bytes(k) for k in (-1, 0, 1, 2, 3, 130)] == [0, 0, 1824, 1824, 1840, 1808 + 1040]
  wb = lambda hs, ws, ss, cs: lib.expo_jpeg_decode_workspace_bytes(ints(*hs), ints(*ws), ints(*ss), ints(*cs), len(hs))
  assert lib.expo_jpeg_decode_workspace_bytes(None, None, None, None, 0) == 0
  assert lib.expo_jpeg_decode_workspace_bytes(None, ints(4), ints(0), ints(3), 1) == 0
  assert wb([0], [4], [0], [3]) == 0 and wb([4], [4], [3], [3]) == 0 and wb([4], [4], [0], [2]) == 0 and wb([4], [4], [1], [1]) == 0
  # per picture 128 bytes per block and the planes: real rows of whole blocks across, each piece rounded up to 16
  assert wb([1], [1], [0], [1]) == 128 + 16
  assert wb([1], [1], [0], [3]) == 3 * 128 + 3 * 16
  assert wb([17], [33], [2], [3]) == 36 * 128 + (17 * 40 + 8) + 2 * (9 * 24 + 8)   # Y 17 x 40 = 680 -> 688; Cb, Cr 9 x 24 = 216 -> 224
  assert wb([17], [33], [1], [3]) == 36 * 128 + (17 * 40 + 8) + 2 * (17 * 24 + 8)  # 3 x 3 MCUs of 4 blocks; Cb, Cr 17 x 24 = 408 -> 416
  assert wb([17, 1], [33, 1], [2, 0], [3, 1]) == wb([17], [33], [2], [3]) + wb([1], [1], [0], [1])
  # launch groups of 64 pictures reuse the workspace
  assert wb([8] * 65, [8] * 65, [0] * 65, [3] * 65) == wb([8] * 64, [8] * 64, [0] * 64, [3] * 64) == 64 * (3 * 128 + 3 * 64)
  assert _cabi.jpeg_decode_workspace_bytes([17], [33], [2], [3]) == wb([17], [33], [2], [3])
