"""CPU-only: argument validation of expo_chain_fused_fwd_ragged (ABI 9) through ctypes.  Every call here is rejected
(or is the empty no-op) before anything is enqueued, so the device pointers are never touched and no GPU is needed."""
import ctypes

import pytest

from exposure_amd import _cabi

FAKE = 0x10000  # a device address that is never dereferenced: every call below fails validation first


@pytest.fixture(scope='module')
def lib():
  return _cabi.load()


def call(lib, n, hs, ws, steps=1, dtype=_cabi.EXPO_F16, ids=FAKE, params=FAKE, xs=True, ys=True, null_image=None):
  ptrs = [FAKE + 0x1000 * i for i in range(n)]
  xa = (ctypes.c_void_p * max(n, 1))(*ptrs) if xs else None
  ya = (ctypes.c_void_p * max(n, 1))(*[p + 0x100000 for p in ptrs]) if ys else None
  if null_image is not None:
    xa[null_image] = None
  ha = (ctypes.c_int * len(hs))(*hs) if hs is not None else None
  wa = (ctypes.c_int * len(ws))(*ws) if ws is not None else None
  return lib.expo_chain_fused_fwd_ragged(ids, params, steps, xa, ya, ha, wa, n, dtype, None)


def test_abi_version_is_9(lib):
  assert lib.expo_version() == 9 == _cabi.EXPO_ABI_VERSION


def test_empty_list_is_a_no_op(lib):
  assert lib.expo_chain_fused_fwd_ragged(None, None, 5, None, None, None, None, 0, _cabi.EXPO_F16, None) == 0
  assert lib.expo_chain_fused_fwd_ragged(None, None, 0, None, None, None, None, 0, _cabi.EXPO_F32, None) == 0


def test_null_host_arrays_and_image_pointers(lib):
  assert call(lib, 2, [4, 4], [4, 4], xs=False) == -1
  assert call(lib, 2, [4, 4], [4, 4], ys=False) == -1
  assert call(lib, 2, None, [4, 4]) == -1
  assert call(lib, 2, [4, 4], None) == -1
  assert call(lib, 2, [4, 4], [4, 4], ids=None) == -1
  assert call(lib, 2, [4, 4], [4, 4], params=None) == -1
  assert call(lib, 3, [4, 4, 4], [4, 4, 4], null_image=2) == -1  # the LAST image's pointer: found before any launch
  assert b'null' in lib.expo_last_error()


def test_steps_out_of_range(lib):
  assert call(lib, 1, [4], [4], steps=65) == -1
  assert b'steps' in lib.expo_last_error()
  assert call(lib, 1, [4], [4], steps=-1) == -1


def test_bad_image_sizes(lib):
  assert call(lib, 2, [4, 0], [4, 4]) == -1  # h = 0 in the second image
  assert call(lib, 2, [4, 4], [4, -3]) == -1
  assert call(lib, 2, [4, 40000], [4, 40000]) == -1  # one image >= 2 GiB
  assert b'2 GiB' in lib.expo_last_error()
  assert call(lib, 2, [4, 40000], [4, 40000], dtype=_cabi.EXPO_F32) == -1
  assert lib.expo_chain_fused_fwd_ragged(None, None, 1, None, None, None, None, -1, _cabi.EXPO_F16, None) == -1


def test_bad_dtype(lib):
  assert call(lib, 1, [4], [4], dtype=7) == -2
  assert lib.expo_chain_fused_fwd_ragged(None, None, 1, None, None, None, None, 0, 2, None) == -2
