"""CPU-only: argument validation of expo_chain_fused_fwd_taps / expo_chain_fused_fwd_ragged_taps (added exports of
ABI 9) through ctypes.  Every call here is rejected (or is the empty no-op) before anything is enqueued, so the fake
device addresses are never touched and no GPU is needed."""
import ctypes

import pytest

from exposure_amd import _cabi

FAKE = 0x10000  # a device address that is never dereferenced
F16, F32 = _cabi.EXPO_F16, _cabi.EXPO_F32
U8, STORAGE = _cabi.EXPO_TAP_U8, _cabi.EXPO_TAP_STORAGE


@pytest.fixture(scope='module')
def lib():
  return _cabi.load()


def dense(lib, n=1, h=4, w=4, steps=3, dtype=F16, x=FAKE, y=FAKE + 0x100000, mask=1, fmt=U8, taps=FAKE + 0x200000,
          ids=FAKE, params=FAKE):
  return lib.expo_chain_fused_fwd_taps(ids, params, steps, x, y, n, h, w, dtype, mask, fmt, taps, None)


def ragged(lib, n=2, hs=(4, 5), ws=(4, 3), steps=3, dtype=F16, mask=1, fmt=U8, ys=True, taps=True, null_x=None,
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
  return lib.expo_chain_fused_fwd_ragged_taps(ids, params, steps, xa, ya, ha, wa, n, dtype, mask, fmt, ta, None)


def test_version_stays_9_and_constants(lib):
  assert lib.expo_version() == 9 == _cabi.EXPO_ABI_VERSION
  assert (STORAGE, U8) == (0, 1)
  for name in ('expo_chain_fused_fwd_taps', 'expo_chain_fused_fwd_ragged_taps'):
    assert name in _cabi.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize('steps,mask', [(3, 1 << 3), (3, 0b1000 | 1), (1, 2), (0, 1), (63, 1 << 63), (5, 1 << 40)])
def test_mask_bits_must_be_below_steps(lib, steps, mask):
  assert dense(lib, n=0, steps=steps, mask=mask) == -1  # checked before the n == 0 early return
  assert dense(lib, steps=steps, mask=mask) == -1
  assert ragged(lib, n=0, steps=steps, mask=mask) == -1
  assert ragged(lib, steps=steps, mask=mask) == -1


def test_all_64_steps_may_be_tapped(lib):
  # bit 63 with 64 steps is legal: the call then fails only on the null parameter pointer, not on the mask
  assert dense(lib, n=0, steps=64, mask=(1 << 64) - 1) == 0
  assert ragged(lib, n=0, steps=64, mask=(1 << 64) - 1) == 0
  assert dense(lib, steps=64, mask=(1 << 64) - 1, params=None) == -1
  assert b'null' in lib.expo_last_error()


@pytest.mark.parametrize('fmt', [-1, 2, 7])
def test_format_must_be_one_of_the_two(lib, fmt):
  assert dense(lib, fmt=fmt) == -1
  assert dense(lib, n=0, fmt=fmt) == -1
  assert ragged(lib, fmt=fmt) == -1
  assert ragged(lib, n=0, fmt=fmt) == -1
  assert b'tap_format' in lib.expo_last_error()


def test_taps_must_be_given_when_tapping(lib):
  assert dense(lib, taps=None) == -1
  assert ragged(lib, taps=False) == -1
  for i in range(3):  # every image's buffer, the last one included, before anything is launched
    assert ragged(lib, n=3, hs=(4, 4, 4), ws=(4, 4, 4), null_tap=i) == -1
    assert b'tap' in lib.expo_last_error()


def test_nothing_to_write(lib):
  assert dense(lib, y=None, mask=0) == -1
  assert b'nothing to write' in lib.expo_last_error()
  assert dense(lib, n=0, y=None, mask=0) == -1
  assert ragged(lib, ys=False, mask=0) == -1
  assert b'nothing to write' in lib.expo_last_error()
  assert ragged(lib, n=0, ys=False, mask=0, taps=False) == -1


def test_ys_null_as_a_whole_but_not_per_image(lib):
  # ys == NULL with taps is legal (the call only fails on the later null parameter pointer)
  assert ragged(lib, ys=False, params=None) == -1
  assert b'null pointer' in lib.expo_last_error()
  for i in range(2):
    assert ragged(lib, null_y=i) == -1
    assert b'null image pointer' in lib.expo_last_error()
  assert ragged(lib, null_x=1) == -1


def test_image_checks_as_the_calls_without_taps(lib):
  assert dense(lib, h=0) == -1
  assert dense(lib, dtype=5) == -2
  assert dense(lib, steps=65, mask=1) == -1
  assert dense(lib, steps=-1, mask=0) == -1
  assert dense(lib, x=None) == -1
  assert dense(lib, h=1 << 15, w=1 << 15, dtype=F32) == -1  # one image >= 2 GiB
  assert ragged(lib, n=-1) == -1
  assert ragged(lib, dtype=5) == -2
  assert ragged(lib, hs=(4, 0)) == -1  # the last image's size is checked too
  assert ragged(lib, n=2, hs=(4, 1 << 15), ws=(4, 1 << 15), dtype=F32) == -1


def test_empty_calls_are_no_ops(lib):
  assert dense(lib, n=0) == 0
  assert dense(lib, n=0, mask=0) == 0
  assert lib.expo_chain_fused_fwd_ragged_taps(None, None, 5, None, None, None, None, 0, F16, 1, U8, None, None) == 0
  assert lib.expo_chain_fused_fwd_ragged_taps(None, None, 0, None, None, None, None, 0, F32, 0, STORAGE, None,
                                              None) == -1  # ys NULL and no taps: nothing to write, even for n == 0
