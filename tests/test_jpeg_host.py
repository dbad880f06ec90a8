"""CPU: the baseline JPEG file of DESIGN.md §3.34 through its NumPy restatement (tests/jpeg_host.py) and independent
judges -- PIL's own tables and decoder, the restatement's own Huffman decoder --, the committed cosine table against its
formula, the coverage the GPU test's case set must have, the quality against PIL's encoder, the host side of the four
entry points, and tools/jpeg_rehearse.cpp under the sanitizers against the restatement byte for byte."""
import ctypes
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from exposure_amd import _cabi
from tests import jpeg_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = jpeg_host.SUBSAMPLINGS
# The worst PSNR deficit against PIL's own file of the same quality and sampling over the case set, measured with this
# restatement: -1.02 dB (7 x 9 noise, quality 100, 4:4:4: 49.79 against 50.81 dB; the issue's prototype, on another
# set: -0.39 dB).  On the tiny pictures the difference is the scatter of a mean over 63 pixels -- it runs from -1.02 to
# +0.58 dB there --, so the pictures of at least 4096 pixels are held to their own worst, -0.15 dB (64 x 64 noise,
# quality 100, 4:4:4: 50.26 against 50.41 dB).  The slack of 0.1 dB covers the two differences from PIL's integer
# encoder, the 13-bit cosine table and the chroma rounding.
WORST_DEFICIT_DB = -1.02
WORST_DEFICIT_LARGE_DB = -0.15
QUALITY_BOUND_DB = WORST_DEFICIT_DB - 0.1
QUALITY_BOUND_LARGE_DB = WORST_DEFICIT_LARGE_DB - 0.1


def ri_of(sub):
  return _cabi.jpeg_restart_mcus(sub)


def all_cases():
  for sub in SUBS:
    ri = ri_of(sub)
    for q in jpeg_host.QUALITIES:
      for (shape, name, pic), full in zip(jpeg_host.case_pictures(ri), jpeg_host.case_files(q, sub, ri)):
        yield (shape, name, q, sub), pic, full, ri


def pil_file(pic, quality, sub):
  buf = io.BytesIO()
  Image.fromarray(pic, 'RGB').save(buf, 'JPEG', quality=quality, subsampling=sub)
  return buf.getvalue()


def test_huffman_tables_are_the_ones_pil_writes():
  theirs = jpeg_host.parse(pil_file(jpeg_host.contents(16, 16, 1)['smooth'], 75, 2))
  dht = b''.join(b'\xff\xc4' + (len(body) + 2).to_bytes(2, 'big') + body for m, body in theirs['segments'] if m == 0xC4)
  # PIL writes the four tables in one or several segments, in the order DC0, AC0, DC1, AC1: compare table by table
  tables, at = [], 0
  for m, body in theirs['segments']:
    if m != 0xC4:
      continue
    at = 0
    while at < len(body):
      n = sum(body[at + 1:at + 17])
      tables.append(bytes(body[at:at + 17 + n]))
      at += 17 + n
  ours = [seg[4:] for seg in jpeg_host.dht_segments()]
  assert sorted(tables) == sorted(ours) and len(dht) > 0
  assert [len(s) for s in jpeg_host.dht_segments()] == [33, 183, 33, 183]


@pytest.mark.parametrize('quality', (1, 10, 25, 49, 50, 51, 75, 90, 95, 100))
def test_quantisation_tables_are_pils(quality):
  data = pil_file(jpeg_host.contents(16, 16, 1)['smooth'], quality, 2)
  theirs = Image.open(io.BytesIO(data)).quantization
  in_file = jpeg_host.parse(data)['dqt']
  for t in range(2):
    ours = jpeg_host.quant_table(t, quality)
    assert list(ours[jpeg_host.ZIGZAG]) == in_file[t]  # the file holds them in zigzag order
    assert list(theirs[t]) in (list(ours), list(ours[jpeg_host.ZIGZAG]))  # PIL's attribute: either order, by version
  mine = jpeg_host.parse(jpeg_host.encode(jpeg_host.contents(8, 8, 1)['smooth'], quality, 0, 8))['dqt']
  assert mine == in_file


def test_pil_decodes_every_file_and_the_stream_decodes_to_the_coefficients():
  for what, pic, full, ri in all_cases():
    data = full['file']
    got = jpeg_host.pil_decode(data)
    assert got.shape == pic.shape, what
    parsed = jpeg_host.parse(data)
    h, w, _ = pic.shape
    assert (parsed['h'], parsed['w'], parsed['ri'], parsed['header_bytes']) == (h, w, ri, jpeg_host.HEADER_BYTES), what
    assert parsed['sampling'] == (0x11 if what[3] == 0 else 0x22) and parsed['intervals'] == full['intervals'], what
    assert parsed['markers'] == [0xD0 + k % 8 for k in range(len(full['intervals']) - 1)] + [0xD9], what
    coefs = jpeg_host.decode_coefficients(parsed, full['blocks'].shape[0], what[3])
    assert np.array_equal(coefs, full['blocks']), what
    assert [m for m, _ in parsed['segments']] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA], what


def test_cosine_table_of_the_header_is_the_formula():
  src = open(os.path.join(ROOT, 'exposure_amd', 'csrc', 'jpeg_codec.h')).read()
  body = re.search(r'kCos\[64\] = \{(.*?)\};', src, flags=re.S).group(1)
  table = [int(v) for v in re.findall(r'-?\d+', re.sub(r'//.*', '', body))]
  assert table == jpeg_host.COS.reshape(-1).tolist() == jpeg_host.cosine_table().reshape(-1).tolist()
  assert int(np.abs(jpeg_host.COS).sum(axis=1).max()) == 23168  # the int32 bound of DESIGN.md §3.34


def test_bound_covers_every_file_and_sizes_of_the_abi():
  for (shape, name, q, sub), pic, full, ri in all_cases():
    assert len(full['file']) <= _cabi.jpeg_encode_bound(shape[0], shape[1], sub), (shape, name, q, sub)
  bpm = {0: 3, 2: 6}
  for sub in SUBS:
    ri = ri_of(sub)
    assert 1 <= ri <= 65535
    side = 8 if sub == 0 else 16
    for h, w in ((1, 1), (17, 33), (4000, 6000), (65535, 65535)):
      mcus = -(-h // side) * -(-w // side)
      full_ints, rest = divmod(mcus, ri)
      per = lambda m: 2 * -(-(m * bpm[sub] * 1660) // 8) + 2
      assert _cabi.jpeg_encode_bound(h, w, sub) == 629 + full_ints * per(ri) + (per(rest) if rest else 0)
      nint = -(-mcus // ri)
      r16 = lambda x: (x + 15) // 16 * 16
      assert _cabi.jpeg_encode_workspace_bytes([h], [w], sub) == 16 + r16(4 * nint) + r16(8 * nint)
    # a launch group at a time uses the workspace
    one = _cabi.jpeg_encode_workspace_bytes([64] * 64, [64] * 64, sub)
    assert _cabi.jpeg_encode_workspace_bytes([64] * 65, [64] * 65, sub) == one == 64 * _cabi.jpeg_encode_workspace_bytes([64], [64], sub)
  # 16 x 24 MP: the workspace is a small fraction of the pictures' raw size
  assert _cabi.jpeg_encode_workspace_bytes([4000] * 16, [6000] * 16, 2) < 16 * 4000 * 6000 * 3 // 100


def test_entry_points_validate_before_anything_is_enqueued():
  lib = _cabi.load()
  vp = ctypes.c_void_p
  fake = 0x1000  # never dereferenced on the host

  def call(n=1, h=4, w=6, q=90, sub=2, cap=1 << 20, ws_bytes=1 << 20, pics=True, outs=True, wsp=fake + 0xFF0):
    hs, ws = (ctypes.c_int * 1)(h), (ctypes.c_int * 1)(w)
    rc = lib.expo_jpeg_encode_ragged((vp * 1)(fake) if pics else None, hs, ws, n, q, sub, (vp * 1)(fake) if outs else None,
                                     (ctypes.c_int64 * 1)(cap), vp(fake), vp(wsp) if wsp else None, ws_bytes, None)
    return rc, (lib.expo_last_error() or b'').decode()

  assert lib.expo_jpeg_encode_ragged(None, None, None, 0, 90, 2, None, None, None, None, 0, None) == 0  # n == 0: a no-op
  for bad, word in ((dict(n=-1), 'n >= 0'), (dict(h=0), '1..65535'), (dict(w=0), '1..65535'), (dict(h=65536), '1..65535'),
                    (dict(w=65536), '1..65535'), (dict(q=0), 'quality'), (dict(q=101), 'quality'), (dict(sub=1), 'subsampling'),
                    (dict(sub=3), 'subsampling'), (dict(sub=-1), 'subsampling'), (dict(cap=-1), 'out_capacity'),
                    (dict(ws_bytes=0), 'workspace too small'), (dict(ws_bytes=47), 'workspace too small'),
                    (dict(pics=False), 'null pointer'), (dict(outs=False), 'null pointer'), (dict(wsp=None), 'null workspace'),
                    (dict(wsp=fake + 8), '16-byte aligned')):
    rc, msg = call(**bad)
    assert rc == -1 and word in msg, (bad, rc, msg)
  assert lib.expo_jpeg_restart_mcus(1) == -1 and b'subsampling' in lib.expo_last_error()
  assert lib.expo_jpeg_encode_bound(0, 4, 0) == -1 and b'1..65535' in lib.expo_last_error()
  assert lib.expo_jpeg_encode_bound(4, 65536, 2) == -1 and lib.expo_jpeg_encode_bound(4, 4, 1) == -1
  assert b'subsampling' in lib.expo_last_error()
  one = (ctypes.c_int * 1)(4)
  assert lib.expo_jpeg_encode_workspace_bytes(one, one, 0, 0) == 0 and lib.expo_jpeg_encode_workspace_bytes(None, one, 1, 0) == 0
  assert lib.expo_jpeg_encode_workspace_bytes(one, one, 1, 1) == 0
  assert lib.expo_jpeg_encode_workspace_bytes((ctypes.c_int * 1)(0), one, 1, 0) == 0
  assert lib.expo_jpeg_encode_workspace_bytes(one, one, 1, 0) == 48


def test_binding_and_abi_surface():
  import torch
  from exposure_amd import evaluate
  names = ('expo_jpeg_restart_mcus', 'expo_jpeg_encode_bound', 'expo_jpeg_encode_workspace_bytes', 'expo_jpeg_encode_ragged')
  header = open(os.path.join(ROOT, 'include', 'exposure_hip.h')).read()
  lib = ctypes.CDLL(_cabi.LIB_PATH)
  for name in names:
    assert name in _cabi.SIGNATURES and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, header), name
  assert _cabi.load().expo_version() == 9  # added exports: the version is unchanged
  assert _cabi.JPEG_SUBSAMPLING == evaluate.JPEG_SUBSAMPLING == ('444', '420')
  assert _cabi.jpeg_restart_mcus('444') == _cabi.jpeg_restart_mcus(0) and _cabi.jpeg_restart_mcus('420') == _cabi.jpeg_restart_mcus(2)
  assert _cabi.jpeg_encode_ragged([]) == ([], None) and evaluate.encode_jpeg_batch([]) == []
  pic = torch.zeros((4, 4, 3), dtype=torch.uint8)
  with pytest.raises(_cabi.ExposureHipError, match='no CPU fallback'):
    _cabi.jpeg_encode_ragged([pic])
  with pytest.raises(_cabi.ExposureHipError, match='quality'):
    _cabi.jpeg_encode_ragged([pic], quality=0)
  with pytest.raises(_cabi.ExposureHipError, match='subsampling'):
    _cabi.jpeg_encode_ragged([pic], subsampling='422')
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.jpeg_encode_bound(70000, 4)


def quality_deficits():
  """per case with any error at all: PSNR of the PIL-decoded restatement file minus PSNR of PIL's own file"""
  out = []
  for what, pic, full, ri in all_cases():
    ours = jpeg_host.psnr(jpeg_host.pil_decode(full['file']), pic)
    theirs = jpeg_host.psnr(jpeg_host.pil_decode(pil_file(pic, what[2], what[3])), pic)
    out.append((ours - theirs, what, ours, theirs))
  return out


def test_quality_is_pils_within_the_measured_deficit():
  deficits = quality_deficits()
  worst = min(deficits)
  large = min(d for d in deficits if d[1][0][0] * d[1][0][1] >= 4096)
  print('worst deficit %.3f dB at %r: %.2f against %.2f dB' % worst)
  print('worst deficit of the pictures of at least 4096 pixels %.3f dB at %r: %.2f against %.2f dB' % large)
  assert worst[0] >= QUALITY_BOUND_DB, worst
  assert large[0] >= QUALITY_BOUND_LARGE_DB, large


def test_case_set_covers_every_path_of_the_entropy_coder():
  """checked on the restatement alone, so that the GPU test cannot pass on easy inputs"""
  for sub in SUBS:
    ri = ri_of(sub)
    side = 8 if sub == 0 else 16
    seen = set()
    for (shape, name, q, s), pic, full, _ in all_cases():
      if s != sub:
        continue
      h, w = shape
      mx, my = -(-w // side), -(-h // side)
      if mx * my > 8 * ri:
        seen.add('rst wraps')
        assert 0xD7 in jpeg_host.parse(full['file'])['markers'] and len(full['intervals']) > 9
      if h % side:
        seen.add('replication down')
      if w % side:
        seen.add('replication right')
      if mx % ri and my > 1:
        seen.add('interval spans two MCU rows')
      if b'\xff\x00' in full['file'][jpeg_host.HEADER_BYTES:] and any(b'\xff' in i for i in full['intervals']):
        seen.add('stuffed FF 00')
      for pad in full['paddings']:
        seen.add('padding 0' if pad == 0 else 'padding 1..7')
      for syms in full['symbols']:
        for block in syms:
          kind, cat, _, _ = block[0]
          if cat == 0:
            seen.add('DC category 0')
          if cat >= 10:
            seen.add('DC category >= 10')
          ac = [sym for k, sym, _, _ in block[1:]]
          if 0xF0 in ac:
            seen.add('ZRL')
          if 0x00 in ac:
            seen.add('EOB')
          elif ac:
            seen.add('coefficient 63, no EOB')
          if any(sym & 15 == 10 for sym in ac):
            seen.add('AC size 10')
    need = {'rst wraps', 'replication down', 'replication right', 'interval spans two MCU rows', 'stuffed FF 00',
            'padding 0', 'padding 1..7', 'DC category 0', 'DC category >= 10', 'ZRL', 'EOB', 'coefficient 63, no EOB',
            'AC size 10'}
    assert need <= seen, (sub, sorted(need - seen))


def test_rehearsal_program_under_sanitizers(tmp_path):
  """tools/jpeg_rehearse.cpp: the kernels' serial routines (csrc/jpeg_codec.h) and phases on the host, a stand-alone
  program built with AddressSanitizer and UBSan: its self-test, and whole files equal to the restatement's"""
  cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
  if cxx is None:
    pytest.skip('no host C++ compiler')
  exe = str(tmp_path / 'jpeg_rehearse')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(ROOT, 'tools', 'jpeg_rehearse.cpp'), '-o', exe])
  assert subprocess.run([exe, 'selftest'], stdout=subprocess.PIPE).stdout.decode().strip() == 'jpeg_rehearse selftest: ok'
  for sub in SUBS:
    ri = ri_of(sub)
    for q in (1, 90, 100):
      for (shape, name, pic), full in zip(jpeg_host.case_pictures(ri), jpeg_host.case_files(q, sub, ri)):
        if name not in ('smooth', 'noise', 'checker') or shape in ((8, 8), (16, 16)):
          continue
        pic.tofile(str(tmp_path / 'in.rgb'))
        subprocess.check_call([exe, 'encode', str(shape[0]), str(shape[1]), str(q), str(sub), str(tmp_path / 'in.rgb'),
                               str(tmp_path / 'out.jpg')], stdout=subprocess.DEVNULL)
        assert open(str(tmp_path / 'out.jpg'), 'rb').read() == full['file'], (shape, name, q, sub)
