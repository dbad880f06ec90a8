"""CPU: the file format of expo_png_encode_ragged and the host side of the export.  The NumPy
restatement of tests/png_host.py writes files that zlib (which also checks the Adler-32) with a NumPy unfilter, and PIL,
decode to the input's pixels; noise hits the bound to the byte; the four new names are in the header, the binding and
the library; every argument check of the export answers without a GPU; the bound and SEG follow the formula."""
import ctypes
import io
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from exposure_amd import _cabi
from tests import png_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('expo_png_segment_bytes', 'expo_png_encode_bound', 'expo_png_encode_workspace_bytes', 'expo_png_encode_ragged')
SHAPES = [(1, 1), (1, 2), (2, 1), (7, 9), (64, 64), (33, 341), (3, 21845)]  # the last: rows longer than a segment


@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_decodes_to_the_pixels(shape):
  from PIL import Image
  h, w = shape
  for name, pic in png_host.contents(h, w, seed=h * 100003 + w).items():
    for filt in range(6):
      data = png_host.encode(pic, filt)
      stream = zlib.decompress(png_host.check_structure(data, h, w))  # zlib checks the Adler-32
      assert stream == png_host.filtered_stream(pic, filt)[0].tobytes(), (name, filt)
      assert (png_host.unfilter(stream, h, w) == pic).all(), (name, filt)
      got = np.array(Image.open(io.BytesIO(data)))
      assert got.shape == pic.shape and got.dtype == np.uint8 and (got == pic).all(), (name, filt)
      assert len(data) == png_host.file_plan(pic, filt)[0] <= png_host.bound(h, w)


def test_noise_gives_exactly_the_bound():
  for h, w in ((64, 64), (33, 341), (3, 21845)):
    pic = png_host.contents(h, w, seed=5)['noise']
    data = png_host.encode(pic, 0)
    s = h * (1 + 3 * w)
    assert len(data) == 75 + 17 * (-(-s // png_host.SEG)) + s == png_host.bound(h, w)
    assert all(png_host.file_plan(pic, 0)[1])  # every segment stored


def test_the_deep_picture_needs_the_limit_and_decodes():
  from PIL import Image
  pic = png_host.deep_picture()
  data = png_host.encode(pic, 0)
  assert (np.array(Image.open(io.BytesIO(data))) == pic).all() and len(data) <= png_host.bound(1, 1925)


def test_header_binding_and_library_agree_on_the_four_names():
  header = open(os.path.join(ROOT, 'include', 'exposure_hip.h')).read()
  assert '#define EXPO_ABI_VERSION 9 ' in header and _cabi.EXPO_ABI_VERSION == 9
  code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  for name in EXPORTS:
    assert name in header.split('#define EXPO_OK')[0], name  # listed among ABI 9's added exports
    decl = re.search(r'^\w+ %s\((.*?)\);' % name, code, flags=re.M | re.S)
    assert decl is not None, name
    args = [] if decl.group(1).strip() == 'void' else decl.group(1).split(',')
    assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == len(args), name
    assert ('%s (net.py:769-772)' % name) in header, name  # each cites what it replaces
  assert _cabi.SIGNATURES['expo_png_encode_bound'][0] is ctypes.c_int64
  for binding in ('png_segment_bytes', 'png_encode_bound', 'png_encode_ragged'):
    assert callable(getattr(_cabi, binding))
  nm = shutil.which('nm')
  if nm is not None:
    syms = subprocess.check_output([nm, '-D', '--defined-only', _cabi.LIB_PATH]).decode()
    for name in EXPORTS:
      assert re.search(r' T %s$' % name, syms, flags=re.M), name
  lib = ctypes.CDLL(_cabi.LIB_PATH)
  for name in EXPORTS:
    assert hasattr(lib, name), name


def test_bound_and_segment_bytes_follow_the_formula():
  seg = _cabi.png_segment_bytes()
  assert 16384 <= seg <= 65535 and seg == png_host.SEG
  for h, w in SHAPES + [(4000, 6000), (seg // 16, 5), (seg // 16 + 1, 5), (1, 1925), (46340, 15446)]:
    s = h * (1 + 3 * w)
    assert s < 2**31
    assert _cabi.png_encode_bound(h, w) == 75 + 17 * (-(-s // seg)) + s == png_host.bound(h, w, seg), (h, w)
  lib = _cabi.load()
  for h, w in ((0, 1), (1, 0), (-3, 4), (46341, 15447), (1, 715827883)):  # the last two: S >= 2^31
    assert lib.expo_png_encode_bound(h, w) == -1 and b'2^31' in lib.expo_last_error(), (h, w)
    with pytest.raises(_cabi.ExposureHipError):
      _cabi.png_encode_bound(h, w)
  one = (ctypes.c_int * 1)
  assert lib.expo_png_encode_workspace_bytes(one(0), one(4), 1) == 0
  small, big = lib.expo_png_encode_workspace_bytes(one(4), one(4), 1), lib.expo_png_encode_workspace_bytes(one(512), one(512), 1)
  assert seg < small < big and big >= 512 * (1 + 3 * 512)  # a slot per segment


def test_arguments_are_refused_before_anything_is_enqueued():
  """EXPO_E_BADARG (-1) with a message, never EXPO_E_HIP (-3).  The device pointers are made-up addresses the host
  never reads: a call that got past the checks would be refused for its workspace, so nothing can reach a device."""
  lib = _cabi.load()
  vp = ctypes.c_void_p
  fake = 0x1000

  def call(n=1, h=4, w=6, filt=5, cap=None, ws_bytes=0, pics=True, outs=True):
    hs, ws = (ctypes.c_int * 1)(h), (ctypes.c_int * 1)(w)
    full = 75 + 17 + h * (1 + 3 * w) if h > 0 and w > 0 else 0
    caps = (ctypes.c_int64 * 1)(full if cap is None else cap)
    rc = lib.expo_png_encode_ragged((vp * 1)(fake) if pics else None, hs, ws, n, filt, (vp * 1)(fake) if outs else None, caps,
                                    vp(fake), vp(fake), ws_bytes, None)
    return rc, (lib.expo_last_error() or b'').decode()

  assert lib.expo_png_encode_ragged(None, None, None, 0, 5, None, None, None, None, 0, None) == 0  # n == 0: a no-op
  for bad, word in ((dict(n=-1), 'n >= 0'), (dict(h=0), 'h >= 1'), (dict(w=0), 'w >= 1'), (dict(h=46341, w=15447), '2^31'),
                    (dict(filt=6), 'filter'), (dict(filt=-1), 'filter'), (dict(cap=75 + 17 + 4 * 19 - 1), 'out_capacity'),
                    (dict(ws_bytes=0), 'workspace too small'), (dict(ws_bytes=1000), 'workspace too small'),
                    (dict(pics=False), 'null pointer'), (dict(outs=False), 'null pointer')):
    rc, msg = call(**bad)
    assert rc == -1 and word in msg, (bad, rc, msg)
  need = lib.expo_png_encode_workspace_bytes((ctypes.c_int * 1)(4), (ctypes.c_int * 1)(6), 1)
  hs, ws, caps = (ctypes.c_int * 1)(4), (ctypes.c_int * 1)(6), (ctypes.c_int64 * 1)(1 << 20)
  rc = lib.expo_png_encode_ragged((vp * 1)(fake), hs, ws, 1, 5, (vp * 1)(fake), caps, vp(fake), None, need, None)
  assert rc == -1 and b'workspace' in lib.expo_last_error()  # enough bytes, no buffer


def test_binding_validates_like_codes_lut_ragged():
  import torch
  assert _cabi.png_encode_ragged([]) == ([], None)
  with pytest.raises(_cabi.ExposureHipError, match='no CPU fallback'):
    _cabi.png_encode_ragged([torch.zeros((4, 4, 3), dtype=torch.uint8)])
  with pytest.raises(_cabi.ExposureHipError, match='filter'):
    _cabi.png_encode_ragged([torch.zeros((4, 4, 3), dtype=torch.uint8)], filter='best')
  with pytest.raises(_cabi.ExposureHipError, match='filter'):
    _cabi.png_encode_ragged([torch.zeros((4, 4, 3), dtype=torch.uint8)], filter=6)
  from exposure_amd import evaluate
  assert evaluate.PNG_FILTERS == _cabi.PNG_FILTERS == png_host.FILTERS
  assert evaluate.encode_png_batch([]) == []


def test_save_png_bytes_writes_the_file_as_it_is(tmp_path):
  from exposure_amd import evaluate
  pic = png_host.contents(7, 9, seed=1)['smooth']
  data = png_host.encode(pic, 5)
  path = evaluate.save_png_bytes(str(tmp_path / 'a.png'), data)
  assert open(path, 'rb').read() == data


def test_rehearsal_program_under_sanitizers(tmp_path):
  """tools/png_rehearse.cpp: the kernels' serial routines (csrc/png_deflate.h) on the host, a stand-alone program built
  with AddressSanitizer and UBSan: its self-test, and a whole file of it decoded by PIL and compared with the
  restatement's length"""
  from PIL import Image
  cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
  if cxx is None:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'png_rehearse')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(ROOT, 'tools', 'png_rehearse.cpp'), '-o', exe])
  assert subprocess.run([exe, 'selftest'], stdout=subprocess.PIPE).stdout.decode().strip() == 'selftest OK'
  for (h, w), name in (((33, 341), 'smooth'), ((7, 9), 'noise'), ((1, 1925), 'deep')):
    pic = png_host.deep_picture() if name == 'deep' else png_host.contents(h, w, seed=9)[name]
    pic.tofile(str(tmp_path / 'in.rgb'))
    for filt in ((0,) if name == 'deep' else (4, 5)):
      subprocess.check_call([exe, 'encode', str(h), str(w), str(filt), str(tmp_path / 'in.rgb'), str(tmp_path / 'out.png')],
                            stdout=subprocess.DEVNULL)
      data = open(str(tmp_path / 'out.png'), 'rb').read()
      assert np.array_equal(np.array(Image.open(io.BytesIO(data))), pic), (name, filt)
      assert zlib.decompress(png_host.check_structure(data, h, w)) == png_host.filtered_stream(pic, filt)[0].tobytes()
      if name != 'deep':
        assert len(data) == png_host.file_plan(pic, filt)[0], (name, filt)
