"""CPU-only: expo_chain_fused_curves_fwd_ragged_codes (an added export of ABI 9) is exported, declared
and bound, and validates the union of its two parents' rules -- expo_chain_fused_curves_fwd_ragged and
expo_chain_fused_fwd_ragged_codes -- before anything is enqueued: every call here is rejected (or is the empty no-op)
with a null stream, so the fake device addresses are never touched and no GPU is needed.  The GPU counterpart is
tests/test_hip_curves_codes.py."""
import ctypes
import os

import pytest

from exposure_amd import _cabi

vp = ctypes.c_void_p
FAKE = 0x10000  # a device address that is never dereferenced
F16, F32 = _cabi.EXPO_F16, _cabi.EXPO_F32
U8, U16, STORAGE = _cabi.EXPO_TAP_U8, _cabi.EXPO_TAP_U16, _cabi.EXPO_TAP_STORAGE
NAME = 'expo_chain_fused_curves_fwd_ragged_codes'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOPTRS = ctypes.cast(None, ctypes.POINTER(vp))


def ints(*v):
  return (ctypes.c_int * len(v))(*v)


def ptrs(*v):
  return (vp * len(v))(*v)


@pytest.fixture(scope='module')
def lib():
  return _cabi.load()


def call(lib, ids=FAKE, params=FAKE, steps=5, L=12, codes=None, channels=3, code_bits=8, tabs=FAKE, stride=256, ys=None,
         hs=None, ws=None, n=1, dtype=F16, tap_mask=0, tap_format=STORAGE, taps=NOPTRS):
  codes = ptrs(*[FAKE] * max(n, 1)) if codes is None else codes
  ys = ptrs(*[FAKE] * max(n, 1)) if ys is None else ys
  hs = ints(*[4] * max(n, 1)) if hs is None else hs
  ws = ints(*[4] * max(n, 1)) if ws is None else ws
  return getattr(lib, NAME)(vp(ids), vp(params), steps, L, codes, channels, code_bits, vp(tabs), stride, ys, hs, ws, n,
                            dtype, tap_mask, tap_format, taps, None)


def test_exported_declared_bound_and_version_stays_9(lib):
  assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), NAME)
  assert lib.expo_version() == 9 == _cabi.EXPO_ABI_VERSION
  assert NAME in _cabi.SIGNATURES and callable(_cabi.chain_fused_curves_fwd_ragged_codes)
  assert len(_cabi.SIGNATURES[NAME][1]) == 18
  with open(os.path.join(ROOT, 'include', 'exposure_hip.h')) as f:
    header = f.read()
  assert 'int %s(' % NAME in header
  assert '#define EXPO_ABI_VERSION 9 ' in header


@pytest.mark.parametrize('L', [0, -1, 17, 1 << 20])
def test_curve_steps_outside_1_to_16(lib, L):
  assert call(lib, L=L) == -1
  assert b'curve_steps' in lib.expo_last_error()
  assert call(lib, L=L, n=0) == -1  # checked before the n == 0 early return


@pytest.mark.parametrize('L', [1, 8, 16])
def test_curve_steps_inside_the_range_pass_that_check(lib, L):
  assert call(lib, L=L, n=0) == 0
  assert call(lib, L=L, codes=ptrs(None)) == -1
  assert b'null image' in lib.expo_last_error()


def test_channels_code_bits_stride_and_tables(lib):
  err = lib.expo_last_error
  for c in (0, 2, 5):
    assert call(lib, channels=c) == -1 and b'channels' in err()
  for bits in (4, 12, 32):
    assert call(lib, code_bits=bits) == -1 and b'code_bits' in err()
  assert call(lib, stride=255) == -1 and b'table_stride' in err()
  assert call(lib, stride=-1) == -1 and b'table_stride' in err()
  assert call(lib, code_bits=16, stride=256) == -1 and b'table_stride' in err()
  assert call(lib, tabs=None) == -1 and b'null' in err()
  for off in (1, 2, 3):
    assert call(lib, tabs=FAKE + off) == -1 and b'aligned' in err()
  # a legal stride (0: one shared table) goes on to the later checks
  assert call(lib, stride=0, codes=ptrs(None)) == -1 and b'null image' in err()
  assert call(lib, code_bits=16, stride=65536, codes=ptrs(None)) == -1 and b'null image' in err()


def test_steps_dtype_and_n(lib):
  assert call(lib, steps=65) == -1 and b'steps' in lib.expo_last_error()
  assert call(lib, steps=-1) == -1
  assert call(lib, dtype=5) == -2 and call(lib, dtype=5, n=0) == -2
  assert call(lib, n=-1) == -1


@pytest.mark.parametrize('steps,mask', [(3, 1 << 3), (3, 0b1000 | 1), (1, 2), (0, 1), (63, 1 << 63)])
def test_tap_bits_must_be_below_steps(lib, steps, mask):
  assert call(lib, steps=steps, tap_mask=mask, taps=ptrs(FAKE)) == -1
  assert b'tap_mask' in lib.expo_last_error()
  assert call(lib, n=0, steps=steps, tap_mask=mask, taps=ptrs(FAKE)) == -1


def test_tap_format_and_buffers(lib):
  for fmt in (-1, 2, 4):
    assert call(lib, tap_mask=1, tap_format=fmt, taps=ptrs(FAKE)) == -1
    assert b'tap_format' in lib.expo_last_error()
  for fmt in (STORAGE, U8, U16):
    assert call(lib, n=0, tap_mask=1, tap_format=fmt, taps=ptrs(FAKE)) == 0
  assert call(lib, tap_mask=1, taps=NOPTRS) == -1 and b'null' in lib.expo_last_error()
  assert call(lib, tap_mask=1, tap_format=U8, taps=ptrs(None)) == -1 and b'null tap' in lib.expo_last_error()
  assert call(lib, n=2, tap_mask=1, tap_format=U16, taps=ptrs(FAKE, None)) == -1 and b'null tap' in lib.expo_last_error()


def test_nothing_to_write(lib):
  assert call(lib, ys=NOPTRS) == -1 and b'nothing to write' in lib.expo_last_error()
  assert call(lib, n=0, ys=NOPTRS) == -1
  # ys NULL as a whole with taps is legal: the call then fails only on a later check
  assert call(lib, ys=NOPTRS, tap_mask=1, taps=ptrs(FAKE), params=None) == -1
  assert b'null pointer' in lib.expo_last_error()


def test_null_pointers_and_null_image_pointers(lib):
  err = lib.expo_last_error
  for kw in (dict(codes=NOPTRS), dict(ids=None), dict(params=None)):
    assert call(lib, **kw) == -1 and b'null pointer' in err(), kw
  f = getattr(lib, NAME)
  assert f(vp(FAKE), vp(FAKE), 5, 4, ptrs(FAKE), 3, 8, vp(FAKE), 0, ptrs(FAKE), None, ints(4), 1, 0, 0, 0, None, None) == -1
  assert f(vp(FAKE), vp(FAKE), 5, 4, ptrs(FAKE), 3, 8, vp(FAKE), 0, ptrs(FAKE), ints(4), None, 1, 0, 0, 0, None, None) == -1
  # no steps: nothing reads the rows; the call then fails only on a later check
  assert call(lib, steps=0, ids=None, params=None, codes=ptrs(None)) == -1 and b'null image' in err()
  for i in range(2):
    cs, ys = [FAKE, FAKE], [FAKE, FAKE]
    cs[i] = None
    assert call(lib, n=2, codes=ptrs(*cs)) == -1 and b'null image' in err()
    ys[i] = None
    assert call(lib, n=2, ys=ptrs(*ys)) == -1 and b'null image' in err()
  # the last image of a second launch is checked before the first launch
  n = 66
  assert call(lib, n=n, codes=ptrs(*([FAKE] * (n - 1) + [None]))) == -1 and b'null image' in err()


def test_sizes(lib):
  err = lib.expo_last_error
  assert call(lib, hs=ints(0)) == -1 and call(lib, ws=ints(-1)) == -1
  assert call(lib, n=2, hs=ints(4, 0)) == -1  # the last image's size is checked too
  assert call(lib, hs=ints(20000), ws=ints(9000), dtype=F32) == -1 and b'2 GiB' in err()  # the output of one image
  # the codes of one image: 16384^2 x 4 channels x 2 bytes = 2 GiB
  assert call(lib, hs=ints(16384), ws=ints(16384), channels=4, code_bits=16, stride=0) == -1 and b'2 GiB' in err()


def test_empty_call_is_a_no_op(lib):
  assert call(lib, n=0) == 0
  assert call(lib, n=0, tap_mask=1, tap_format=U8, taps=ptrs(FAKE)) == 0
  assert getattr(lib, NAME)(None, None, 5, 4, None, 3, 8, None, 0, ptrs(FAKE), None, None, 0, F16, 0, 0, None, None) == 0


def test_binding_rejects_before_the_library_is_asked():
  import torch
  f = _cabi.chain_fused_curves_fwd_ragged_codes
  codes = [torch.zeros((4, 4, 3), dtype=torch.uint8)]
  ids, prm = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 2, 48))
  tabs, ys = torch.zeros((1, 256)), [torch.zeros((4, 4, 3))]
  for L in (0, 17):
    with pytest.raises(_cabi.ExposureHipError, match='curve_steps'):
      f(ids, prm, L, codes, tabs, 256, ys)
  with pytest.raises(_cabi.ExposureHipError, match='filter_ids'):  # host tensors: HIP path only
    f(ids, prm, 4, codes, tabs, 256, ys)
  with pytest.raises(_cabi.ExposureHipError, match='same length'):
    f(ids, prm, 4, codes, tabs, 256, ys + ys)
  with pytest.raises(_cabi.ExposureHipError, match='same length'):
    f(ids, prm, 4, codes, tabs, 256, None, 1, [])
  with pytest.raises(_cabi.ExposureHipError):
    f(ids.long(), prm, 4, codes, tabs, 256, ys)
  with pytest.raises(_cabi.ExposureHipError):
    f(ids[0], prm, 4, codes, tabs, 256, ys)
