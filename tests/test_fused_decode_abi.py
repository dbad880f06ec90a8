"""CPU: expo_decode_tables / expo_decode_tables_bytes, expo_bilinear_resize_ragged_codes and
expo_chain_fused_fwd_ragged_codes are exported, declared and bound, and validate everything before
anything is enqueued (every failing call below would otherwise dereference fake device pointers); the unit that holds the
new pass, chain_fused_codes.hip, passes the two ISA checks of tests/test_isa_sanity.py with the flags csrc/build.sh
gives it; the unit of the new proxy kernels, proxy_codes.hip, has no scratch and no contracted operation."""
import ctypes
import os
import shutil

import pytest

from exposure_amd import _cabi
from tests import test_isa_sanity as isa

vp = ctypes.c_void_p
FAKE = 0x1000  # never dereferenced on the host
NAMES = ('expo_decode_tables_bytes', 'expo_decode_tables', 'expo_bilinear_resize_ragged_codes',
         'expo_chain_fused_fwd_ragged_codes')


def ints(*v):
  return (ctypes.c_int * len(v))(*v)


def ptrs(*v):
  return (vp * len(v))(*v)


NOPTRS = ctypes.cast(None, ctypes.POINTER(vp))


def tables(lib, codes=None, hs=None, ws=None, n=1, channels=3, code_bits=8, table=FAKE, normalize=1, out=FAKE,
           out_bytes=1 << 30, dtype=0, workspace=FAKE, workspace_bytes=1 << 30):
  codes = ptrs(FAKE) if codes is None else codes
  hs = ints(4) if hs is None else hs
  ws = ints(4) if ws is None else ws
  return lib.expo_decode_tables(codes, hs, ws, n, channels, code_bits, vp(table), normalize, vp(out), out_bytes, dtype,
                                vp(workspace), workspace_bytes, None)


def proxy(lib, codes=None, hs=None, ws=None, n=1, channels=3, code_bits=8, tabs=FAKE, stride=256, table_dtype=0,
          windows=(0, 0, 0, 4), q=1, S=64, out=FAKE, out_dtype=0):
  codes = ptrs(FAKE) if codes is None else codes
  hs = ints(4) if hs is None else hs
  ws = ints(4) if ws is None else ws
  win = (ctypes.c_int32 * len(windows))(*windows) if windows is not None else None
  return lib.expo_bilinear_resize_ragged_codes(codes, hs, ws, n, channels, code_bits, vp(tabs), stride, table_dtype, win,
                                               q, S, vp(out), out_dtype, None)


def chain(lib, ids=FAKE, params=FAKE, steps=5, codes=None, channels=3, code_bits=8, tabs=FAKE, stride=256, ys=None,
          hs=None, ws=None, n=1, dtype=0, tap_mask=0, tap_format=0, taps=NOPTRS):
  codes = ptrs(FAKE) if codes is None else codes
  ys = ptrs(FAKE) if ys is None else ys
  hs = ints(4) if hs is None else hs
  ws = ints(4) if ws is None else ws
  return lib.expo_chain_fused_fwd_ragged_codes(vp(ids), vp(params), steps, codes, channels, code_bits, vp(tabs), stride,
                                               ys, hs, ws, n, dtype, tap_mask, tap_format, taps, None)


def test_symbols_exported_and_version():
  lib = ctypes.CDLL(_cabi.LIB_PATH)
  for name in NAMES:
    assert hasattr(lib, name) and name in _cabi.SIGNATURES, name
  # added exports, like the decode, the proxies and the taps before them: the version does not change
  assert _cabi.load().expo_version() == 9 == _cabi.EXPO_ABI_VERSION


def test_tables_validation_before_enqueue():
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  assert tables(lib, n=-1) == -1
  assert tables(lib, channels=2) == -1 and b'channels' in err()
  assert tables(lib, code_bits=12) == -1 and b'code_bits' in err()
  assert tables(lib, normalize=2) == -1 and b'normalize' in err()
  assert tables(lib, dtype=7) == -2
  assert lib.expo_decode_tables(None, None, None, 0, 3, 8, None, 1, None, 0, 0, None, 0, None) == 0  # n == 0: no-op
  assert lib.expo_decode_tables(None, None, None, 0, 3, 8, None, 1, None, 0, 9, None, 0, None) == -2
  for kw in (dict(codes=NOPTRS), dict(table=None), dict(out=None)):
    assert tables(lib, **kw) == -1 and b'null' in err(), kw
  assert lib.expo_decode_tables(ptrs(FAKE), None, ints(4), 1, 3, 8, vp(FAKE), 1, vp(FAKE), 1 << 20, 0, vp(FAKE), 1 << 20,
                                None) == -1
  assert tables(lib, codes=ptrs(FAKE, None), hs=ints(4, 4), ws=ints(4, 4), n=2) == -1 and b'null image' in err()
  assert tables(lib, hs=ints(0)) == -1 and tables(lib, ws=ints(-3)) == -1
  assert tables(lib, hs=ints(16384), ws=ints(16384), channels=4, code_bits=16) == -1 and b'2 GiB' in err()
  assert tables(lib, out=FAKE + 2) == -1 and b'aligned' in err()
  # the tables buffer: n tables with normalisation, one without
  size = lambda n, bits, norm, dt: lib.expo_decode_tables_bytes(n, bits, norm, dt)
  assert size(3, 8, 1, 0) == 3 * 256 * 2 and size(3, 8, 1, 1) == 3 * 256 * 4 and size(3, 16, 1, 0) == 3 * 65536 * 2
  assert size(3, 8, 0, 0) == 256 * 2 and size(70, 16, 0, 1) == 65536 * 4
  assert size(0, 8, 1, 0) == 0 and size(1, 12, 1, 0) == 0 and size(1, 8, 2, 0) == 0 and size(1, 8, 1, 5) == 0
  assert tables(lib, out_bytes=256 * 2 - 1) == -1 and b'tables buffer' in err()
  assert tables(lib, normalize=0, out_bytes=256 * 2 - 1) == -1 and b'tables buffer' in err()
  assert tables(lib, n=2, codes=ptrs(FAKE, FAKE), hs=ints(4, 4), ws=ints(4, 4), out_bytes=2 * 256 * 2 - 1) == -1
  # the workspace of a normalising call follows expo_decode_workspace_bytes: present, 4-byte aligned, large enough
  need = lib.expo_decode_workspace_bytes(1, ints(4), ints(4), 3, 8)
  assert tables(lib, workspace=None) == -1 and b'workspace' in err()
  assert tables(lib, workspace=FAKE + 2) == -1 and b'workspace' in err()
  assert tables(lib, workspace_bytes=need - 1) == -1 and b'workspace' in err()


def test_proxy_validation_before_enqueue():
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  assert proxy(lib, n=-1) == -1 and proxy(lib, q=-1) == -1
  assert proxy(lib, channels=2) == -1 and b'channels' in err()
  assert proxy(lib, code_bits=10) == -1 and b'code_bits' in err()
  assert proxy(lib, table_dtype=3) == -2 and proxy(lib, out_dtype=3) == -2
  assert proxy(lib, stride=255) == -1 and b'table_stride' in err()
  assert proxy(lib, code_bits=16, stride=256) == -1 and b'table_stride' in err()
  assert proxy(lib, q=0, windows=None) == 0  # q == 0: no-op
  assert proxy(lib, S=0) == -1 and proxy(lib, S=4097) == -1
  assert proxy(lib, n=0) == -1 and b'n == 0' in err()
  for kw in (dict(codes=NOPTRS), dict(tabs=None), dict(windows=None), dict(out=None)):
    assert proxy(lib, **kw) == -1 and b'null' in err(), kw
  assert proxy(lib, codes=ptrs(None)) == -1 and b'null image' in err()
  assert proxy(lib, tabs=FAKE + 2) == -1 and b'aligned' in err()
  assert proxy(lib, hs=ints(0)) == -1
  assert proxy(lib, hs=ints(16384), ws=ints(16384), channels=4, code_bits=16, stride=65536) == -1 and b'2 GiB' in err()
  assert proxy(lib, windows=(1, 0, 0, 4)) == -1 and b'index' in err()
  assert proxy(lib, windows=(0, 0, 0, 0)) == -1 and b'side' in err()
  assert proxy(lib, windows=(0, 1, 0, 4)) == -1 and b'outside' in err()
  assert proxy(lib, windows=(0, 0, -1, 2)) == -1 and b'outside' in err()


def test_chain_validation_before_enqueue():
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  taps = ptrs(FAKE)
  assert chain(lib, n=-1) == -1
  assert chain(lib, dtype=4) == -2
  assert chain(lib, channels=5) == -1 and b'channels' in err()
  assert chain(lib, code_bits=4) == -1 and b'code_bits' in err()
  assert chain(lib, stride=100) == -1 and b'table_stride' in err()
  assert chain(lib, steps=65) == -1 and chain(lib, steps=-1) == -1
  assert chain(lib, tap_mask=1, tap_format=2, taps=taps) == -1 and b'tap_format' in err()
  assert chain(lib, tap_mask=1 << 5, taps=taps) == -1 and b'tap_mask' in err()
  # nothing to write: ys NULL and no taps
  assert chain(lib, ys=NOPTRS) == -1 and b'nothing to write' in err()
  assert lib.expo_chain_fused_fwd_ragged_codes(None, None, 5, None, 3, 8, None, 0, ptrs(FAKE), None, None, 0, 0, 0, 0, None,
                                               None) == 0  # n == 0: no-op
  for kw in (dict(codes=NOPTRS), dict(tabs=None), dict(ids=None), dict(params=None), dict(tap_mask=1, taps=NOPTRS)):
    assert chain(lib, **kw) == -1 and b'null' in err(), kw
  assert lib.expo_chain_fused_fwd_ragged_codes(vp(FAKE), vp(FAKE), 5, ptrs(FAKE), 3, 8, vp(FAKE), 0, ptrs(FAKE), None,
                                               ints(4), 1, 0, 0, 0, None, None) == -1
  assert chain(lib, tabs=FAKE + 1) == -1 and b'aligned' in err()
  assert chain(lib, codes=ptrs(None)) == -1 and b'null image' in err()
  assert chain(lib, ys=ptrs(None)) == -1 and b'null image' in err()
  assert chain(lib, tap_mask=1, tap_format=1, taps=ptrs(None)) == -1 and b'null tap' in err()
  assert chain(lib, hs=ints(0)) == -1 and chain(lib, ws=ints(-1)) == -1
  assert chain(lib, hs=ints(20000), ws=ints(9000), dtype=1) == -1 and b'2 GiB' in err()
  assert chain(lib, hs=ints(16384), ws=ints(16384), channels=4, code_bits=16, stride=0) == -1 and b'2 GiB' in err()
  # the last image of a second launch is checked before the first launch
  n = 66
  assert chain(lib, n=n, codes=ptrs(*([FAKE] * (n - 1) + [None])), ys=ptrs(*([FAKE] * n)), hs=ints(*([4] * n)),
               ws=ints(*([4] * n))) == -1 and b'null image' in err()


def test_binding_refuses_cpu_tensors_and_bad_tables():
  import torch
  codes = [torch.zeros((4, 4, 3), dtype=torch.uint8)]
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.decode_tables(codes, torch.zeros(256), 1, torch.float16)
  out = torch.zeros((1, 8, 8, 3))
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.bilinear_resize_ragged_codes(codes, torch.zeros((1, 256)), 256, [(0, 0, 0, 4)], 8, out)
  ids, prm = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 2, 24))
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.chain_fused_fwd_ragged_codes(ids, prm, codes, torch.zeros((1, 256)), 256, [torch.zeros((4, 4, 3))])


def test_codes_unit_isa_sanity(tmp_path):
  if not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)):
    pytest.skip('hipcc not available')
  unit = ('chain_fused_codes.hip', ['-fno-slp-vectorize', '-fno-honor-nans'])  # as csrc/build.sh compiles it
  build = open(os.path.join(isa.CSRC, 'build.sh')).read()
  assert '-fno-slp-vectorize -fno-honor-nans "$@" -c "$HERE/chain_fused_codes.hip"' in build
  txt = isa._listing(unit, str(tmp_path))
  assert txt.count('.amdhsa_kernel') == 96  # 2 code widths x 3 channel counts x 2 dtypes x 2 cache policies x 4 tap formats
  assert 'chain_fused_fwd_ragged_codes_kernel' in txt and 'chain_fused_fwd_ragged_taps_kernel' not in txt
  isa.test_no_store_takes_its_address_from_its_own_data_registers({unit[0]: txt})
  isa.test_streaming_kernels_do_not_spill({unit[0]: txt})


def test_proxy_codes_unit_isa(tmp_path):
  """proxy.hip's contract holds for the unit that reads codes: no scratch, and every float32 operation rounded on its
  own -- no fused multiply-add in any kernel (tests/test_isa_proxy.py checks proxy.hip itself, which this unit includes
  without instantiating its kernels)"""
  if not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)):
    pytest.skip('hipcc not available')
  build = open(os.path.join(isa.CSRC, 'build.sh')).read()
  assert '-ffp-contract=off "$@" -c "$HERE/proxy_codes.hip"' in build and '"$TMP/proxy_codes.o"' in build.split('-shared')[1]
  txt = isa._listing(('proxy_codes.hip', ['-ffp-contract=off']), str(tmp_path))
  assert txt.count('.amdhsa_kernel') == 24  # 2 code widths x 3 channel counts x 2 table dtypes x 2 output dtypes
  assert 'bilinear_resize_codes_kernel' in txt and 'bilinear_resize_kernel' not in txt
  isa.test_streaming_kernels_do_not_spill({'proxy_codes.hip': txt})
  for op in ('v_fma_f32', 'v_fmac_f32', 'v_mad_f32', 'v_pk_fma_f32', 'v_fma_mix', 'v_fma_f16', 'v_mac_f32'):
    assert op not in txt, op
