"""CPU-only: expo_chain_fused_curves_fwd_ragged (an added export of ABI 9) is exported, bound, and validates its
arguments before anything is enqueued: every call here is rejected (or is the empty no-op), so the fake device
addresses are never touched and no GPU is needed.  The GPU counterpart is tests/test_hip_curves_chain.py."""
import ctypes
import os

import pytest

from exposure_amd import _cabi

FAKE = 0x10000  # a device address that is never dereferenced
F16, F32 = _cabi.EXPO_F16, _cabi.EXPO_F32
U8, U16, STORAGE = _cabi.EXPO_TAP_U8, _cabi.EXPO_TAP_U16, _cabi.EXPO_TAP_STORAGE
NAME = 'expo_chain_fused_curves_fwd_ragged'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
  return _cabi.load()


def curves(lib, n=2, hs=(4, 5), ws=(4, 3), steps=3, L=12, dtype=F16, mask=1, fmt=U8, ys=True, taps=True, null_x=None,
           null_y=None, null_tap=None, ids=FAKE, params=FAKE):
  ptrs = [FAKE + 0x1000 * i for i in range(n)]
  xa = (ctypes.c_void_p * max(n, 1))(*ptrs)
  ya = (ctypes.c_void_p * max(n, 1))(*[p + 0x100000 for p in ptrs]) if ys else None
  ta = (ctypes.c_void_p * max(n, 1))(*[p + 0x200000 for p in ptrs]) if taps else None
  if null_x is not None:
    xa[null_x] = None
  if null_y is not None:
    ya[null_y] = None
  if null_tap is not None:
    ta[null_tap] = None
  hs, ws = (list(hs) + [4] * n)[:max(n, 1)], (list(ws) + [4] * n)[:max(n, 1)]
  ha = (ctypes.c_int * len(hs))(*hs)
  wa = (ctypes.c_int * len(ws))(*ws)
  return getattr(lib, NAME)(ids, params, steps, L, xa, ya, ha, wa, n, dtype, mask, fmt, ta, None)


def test_exported_bound_and_version_stays_9(lib):
  assert lib.expo_version() == 9 == _cabi.EXPO_ABI_VERSION
  assert NAME in _cabi.SIGNATURES and hasattr(lib, NAME)
  assert callable(_cabi.chain_fused_curves_fwd_ragged)
  with open(os.path.join(ROOT, 'include', 'exposure_hip.h')) as f:
    header = f.read()
  assert 'int %s(' % NAME in header
  assert '#define EXPO_MAX_PARAMS_CURVES 48' in header
  assert _cabi.EXPO_MAX_PARAMS_CURVES == 48 == 3 * _cabi.EXPO_CURVE_MAX_STEPS


@pytest.mark.parametrize('L', [0, -1, 17, 1 << 20])
def test_curve_steps_outside_1_to_16(lib, L):
  assert curves(lib, L=L) == -1
  assert b'curve_steps' in lib.expo_last_error()
  assert curves(lib, L=L, mask=0) == -1
  assert curves(lib, n=0, L=L) == -1  # checked before the n == 0 early return


@pytest.mark.parametrize('L', [1, 8, 16])
def test_curve_steps_inside_the_range_pass_that_check(lib, L):
  assert curves(lib, n=0, L=L) == 0
  assert curves(lib, L=L, null_x=0) == -1
  assert b'null image pointer' in lib.expo_last_error()


def test_rows_must_be_given_when_there_are_steps(lib):
  assert curves(lib, ids=None) == -1
  assert b'null pointer' in lib.expo_last_error()
  assert curves(lib, params=None) == -1 and curves(lib, params=None, mask=0) == -1
  # no steps: nothing reads the rows; the call then fails only on a later check
  assert curves(lib, steps=0, mask=0, ids=None, params=None, null_x=1) == -1
  assert b'null image pointer' in lib.expo_last_error()


def test_steps_and_dtype(lib):
  assert curves(lib, steps=65) == -1
  assert b'steps' in lib.expo_last_error()
  assert curves(lib, steps=-1, mask=0) == -1
  assert curves(lib, dtype=5) == -2
  assert curves(lib, n=0, dtype=5) == -2
  assert curves(lib, n=-1) == -1


@pytest.mark.parametrize('steps,mask', [(3, 1 << 3), (3, 0b1000 | 1), (1, 2), (0, 1), (63, 1 << 63)])
def test_tap_bits_must_be_below_steps(lib, steps, mask):
  assert curves(lib, steps=steps, mask=mask) == -1
  assert b'tap_mask' in lib.expo_last_error()
  assert curves(lib, n=0, steps=steps, mask=mask) == -1


def test_tap_format_and_buffers(lib):
  for fmt in (-1, 2, 4):
    assert curves(lib, fmt=fmt) == -1
    assert b'tap_format' in lib.expo_last_error()
  for fmt in (STORAGE, U8, U16):
    assert curves(lib, n=0, fmt=fmt) == 0
  assert curves(lib, taps=False) == -1
  for i in range(2):
    assert curves(lib, null_tap=i) == -1
    assert b'tap' in lib.expo_last_error()


def test_nothing_to_write(lib):
  assert curves(lib, ys=False, mask=0) == -1
  assert b'nothing to write' in lib.expo_last_error()
  assert curves(lib, n=0, ys=False, mask=0, taps=False) == -1
  # ys NULL as a whole with taps is legal: the call then fails only on the null rows
  assert curves(lib, ys=False, params=None) == -1
  assert b'null pointer' in lib.expo_last_error()


def test_image_pointers_and_sizes(lib):
  for i in range(2):
    assert curves(lib, null_x=i) == -1
    assert b'null image pointer' in lib.expo_last_error()
    assert curves(lib, null_y=i) == -1
    assert b'null image pointer' in lib.expo_last_error()
  assert curves(lib, hs=(4, 0)) == -1  # the last image's size is checked too
  assert curves(lib, hs=(4, 1 << 15), ws=(4, 1 << 15), dtype=F32) == -1  # one image >= 2 GiB


def test_empty_call_is_a_no_op(lib):
  assert curves(lib, n=0) == 0
  assert curves(lib, n=0, mask=0) == 0
  assert getattr(lib, NAME)(None, None, 5, 4, None, None, None, None, 0, F16, 1, U8, None, None) == 0


def test_binding_rejects_before_the_library_is_asked():
  import torch
  ids = torch.zeros((0, 3), dtype=torch.int32)
  with pytest.raises(_cabi.ExposureHipError, match='curve_steps'):
    _cabi.chain_fused_curves_fwd_ragged(ids, torch.zeros((0, 3, 48)), 17, [], [])
  with pytest.raises(_cabi.ExposureHipError, match='nothing to write'):
    _cabi.chain_fused_curves_fwd_ragged(ids, torch.zeros((0, 3, 48)), 4, [], None)
