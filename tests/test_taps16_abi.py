"""CPU-only: EXPO_TAP_U16 (tap_format 3) in the argument validation of the three tap entry points, through ctypes.
Every call here is rejected (or is the empty no-op) before anything is enqueued, so the fake device addresses are
never touched and no GPU is needed.  The GPU counterpart is tests/test_hip_chain_taps16.py."""
import os

import pytest

from exposure_amd import _cabi
from tests.test_chain_taps_abi import dense, ragged
from tests.test_masked_chain_abi import masked

U16 = 3


@pytest.fixture(scope='module')
def lib():
  return _cabi.load()


def test_constant_and_version(lib):
  assert _cabi.EXPO_TAP_U16 == U16
  assert lib.expo_version() == 9 == _cabi.EXPO_ABI_VERSION
  with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'exposure_hip.h')) as f:
    assert '#define EXPO_TAP_U16 3\n' in f.read()


def test_format_3_is_accepted_on_all_three_entry_points(lib):
  # n == 0: the format is checked before the early return, so 0 means it was accepted
  assert dense(lib, n=0, fmt=U16) == 0
  assert ragged(lib, n=0, fmt=U16) == 0
  assert masked(lib, n=0, fmt=U16) == 0
  for dtype in (_cabi.EXPO_F16, _cabi.EXPO_F32):
    assert dense(lib, n=0, fmt=U16, dtype=dtype, mask=0b101) == 0


def test_format_3_with_a_null_tap_pointer_fails_on_the_buffer_check(lib):
  assert dense(lib, fmt=U16, taps=None) == -1
  err = lib.expo_last_error()
  assert b'null' in err and b'tap_format' not in err
  assert ragged(lib, fmt=U16, taps=False) == -1
  err = lib.expo_last_error()
  assert b'null' in err and b'tap_format' not in err
  assert masked(lib, fmt=U16, taps=False) == -1
  err = lib.expo_last_error()
  assert b'null' in err and b'tap_format' not in err
  for i in range(2):
    assert ragged(lib, fmt=U16, null_tap=i) == -1
    assert b'null tap pointer' in lib.expo_last_error()
    assert masked(lib, fmt=U16, null_tap=i) == -1
    assert b'null tap pointer' in lib.expo_last_error()


@pytest.mark.parametrize('fmt', [4, 5])
def test_formats_past_3_stay_rejected(lib, fmt):
  for call in (dense, ragged, masked):
    assert call(lib, fmt=fmt) == -1
    assert b'tap_format' in lib.expo_last_error()
    assert call(lib, n=0, fmt=fmt) == -1
    assert b'tap_format' in lib.expo_last_error()


def test_the_other_checks_hold_for_format_3(lib):
  assert dense(lib, fmt=U16, steps=3, mask=1 << 3) == -1
  assert b'tap_mask' in lib.expo_last_error()
  assert ragged(lib, fmt=U16, ys=False, mask=0) == -1
  assert b'nothing to write' in lib.expo_last_error()
  assert masked(lib, fmt=U16, mask_params=None) == -1
  assert b'null pointer' in lib.expo_last_error()
