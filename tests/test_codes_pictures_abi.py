"""CPU: the C-ABI and build side of DESIGN.md §3.24 -- the two added exports in include/exposure_hip.h, in
_cabi.SIGNATURES and in the built library's dynamic symbols; the flags csrc/build.sh compiles the new unit with;
and, cross-compiled with -S (nothing runs), the register and spill metadata of every new kernel: no scratch, no
spilled register."""
import os
import re
import shutil
import subprocess

import pytest

from exposure_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
EXPORTS = ('expo_codes_max_ragged', 'expo_codes_lut_ragged')
# unit -> (the flags of its build.sh line beyond the common ones, the new kernels' name, how many instantiations)
UNITS = {
    # (code width x entry width x channels x cache policy) + the LDS-staged 16-bit variant (channels x cache policy)
    'codes_lut.hip': ([], 'codes_lut_kernel', 2 * 2 * 3 * 2 + 3 * 2),
    'decode.hip': ([], 'codes_max_finish_kernel', 1),
}


def build_lines():
  sh = open(os.path.join(CSRC, 'build.sh')).read()
  lines = {}
  for unit in UNITS:
    found = [l for l in sh.splitlines() if '/%s"' % unit in l and l.lstrip().startswith('"$HIPCC"')]
    assert len(found) == 1, (unit, found)
    lines[unit] = found[0]
  return sh, lines


def test_header_declares_the_exports_as_additions_to_abi_9():
  header = open(os.path.join(ROOT, 'include', 'exposure_hip.h')).read()
  assert '#define EXPO_ABI_VERSION 9 ' in header and _cabi.EXPO_ABI_VERSION == 9
  for name in EXPORTS:
    assert re.search(r'^int %s\(' % name, header, flags=re.M), name
    assert name in header.split('#define EXPO_OK')[0], name  # listed among ABI 9's added exports


def test_signatures_match_the_declarations():
  header = open(os.path.join(ROOT, 'include', 'exposure_hip.h')).read()
  for name in EXPORTS:
    decl = re.search(r'^int %s\((.*?)\);' % name, header, flags=re.M | re.S).group(1)
    assert name in _cabi.SIGNATURES
    res, args = _cabi.SIGNATURES[name]
    assert res is _cabi._i and len(args) == len(decl.split(',')), (name, len(args), decl)
  for binding in ('codes_max_ragged', 'codes_lut_ragged'):
    assert callable(getattr(_cabi, binding))


def test_library_exports_the_symbols():
  nm = shutil.which('nm')
  if nm is None:
    pytest.skip('nm not available')
  assert os.path.exists(_cabi.LIB_PATH), 'the library is not built'
  syms = subprocess.check_output([nm, '-D', '--defined-only', _cabi.LIB_PATH]).decode()
  for name in EXPORTS:
    assert re.search(r' T %s$' % name, syms, flags=re.M), name


def test_build_script_flags_of_the_new_units():
  sh, lines = build_lines()
  for unit, (flags, _kernel, _count) in UNITS.items():
    assert [f for f in lines[unit].split() if f.startswith('-f')] == flags, unit
    assert '"$TMP/%s.o"' % unit[:-4] in sh.split('-shared')[1], unit
  assert 'Fifteen translation units' in sh


@pytest.fixture(scope='module')
def listings(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip('hipcc not available')
  out = tmp_path_factory.mktemp('isa')
  jobs = {}
  for unit, (flags, _kernel, _count) in UNITS.items():  # side by side
    dst = str(out / (unit[:-4] + '.s'))
    jobs[unit] = (dst, subprocess.Popen([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only'] +
                                        flags + [os.path.join(CSRC, unit), '-o', dst], stderr=subprocess.DEVNULL))
  texts = {}
  for unit, (dst, proc) in jobs.items():
    assert proc.wait() == 0, unit
    texts[unit] = open(dst).read()
  return texts


def test_no_new_kernel_has_scratch_or_spills(listings):
  for unit, (_flags, kernel, count) in UNITS.items():
    txt = listings[unit]
    meta = {m.group(1): m.group(2)
            for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, flags=re.S) if kernel in m.group(1)}
    assert len(meta) == count, (unit, len(meta))
    for name, body in meta.items():
      scratch = re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body)
      assert scratch is not None and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
    # the metadata notes: per kernel its name, register counts and the two spill counts
    notes = [n for n in re.findall(r'- \.agpr_count:.*?\.wavefront_size:', txt, flags=re.S) if kernel in n]
    assert len(notes) == count, (unit, len(notes))
    for n in notes:
      name = re.search(r'\.name:\s+(\S+)', n).group(1)
      assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', n).group(1)) == 0, name
      assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', n).group(1)) == 0, name
      assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', n).group(1)) == 0, name
      assert int(re.search(r'\.vgpr_count:\s+(\d+)', n).group(1)) <= 256, name


def test_arguments_are_refused_before_anything_is_enqueued():
  """the checks at the top of the exports, with EXPO_E_BADARG (-1), never EXPO_E_HIP (-3).  Every pointer is NULL, so a
  call that got past them would be refused for its NULL pointers and nothing could reach a device; the checks of the
  images themselves (alignment, sizes) need real buffers and are the GPU tests'"""
  import ctypes
  lib = _cabi.load()
  n = 1
  hs, ws = (ctypes.c_int * n)(4), (ctypes.c_int * n)(6)
  null = (ctypes.c_void_p * n)(0)  # a host array that holds one NULL device pointer

  def lut(codes=None, n=n, c=3, bits=8, stride=256, out_bits=8, outs=None, sizes=(None, None)):
    return lib.expo_codes_lut_ragged(codes, sizes[0], sizes[1], n, c, bits, None, stride, out_bits, outs, None)

  def message():
    return (lib.expo_last_error() or b'').decode()

  assert lut(n=0) == 0  # a no-op
  for bad, word in ((dict(n=-1), 'n >= 0'), (dict(c=2), 'channels'), (dict(bits=12), 'code_bits'),
                    (dict(out_bits=4), 'out_bits'), (dict(stride=255), 'lut_stride'), (dict(bits=16, stride=256), 'lut_stride'),
                    (dict(), 'null pointer'), (dict(codes=null, outs=null, sizes=(hs, ws)), 'null pointer')):
    assert lut(**bad) == -1 and word in message(), (bad, message())

  def mx(codes=None, n=n, c=3, bits=8, sizes=(None, None)):
    return lib.expo_codes_max_ragged(codes, sizes[0], sizes[1], n, c, bits, None, None, 0, None)

  assert mx(n=0) == 0
  for bad, word in ((dict(n=-1), 'n >= 0'), (dict(c=5), 'channels'), (dict(bits=9), 'code_bits'), (dict(), 'null pointer'),
                    (dict(codes=null, sizes=(hs, ws)), 'null pointer')):
    assert mx(**bad) == -1 and word in message(), (bad, message())
