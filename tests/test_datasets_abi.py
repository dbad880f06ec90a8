"""CPU: expo_area_resize_ragged / expo_pack_recut are exported, declared and bound, and validate everything before
anything is enqueued (every failing call below would otherwise dereference fake device pointers); the datasets unit's
ISA passes the checks of tests/test_isa_sanity.py."""
import ctypes
import os
import shutil

import pytest

from exposure_amd import _cabi
from tests import test_cabi_symbols
from tests import test_isa_sanity as isa

vp = ctypes.c_void_p
FAKE = 0x1000  # never dereferenced on the host
NAMES = ('expo_area_resize_ragged', 'expo_pack_recut')


def ints(*v):
  return (ctypes.c_int * len(v))(*v)


def ptrs(*v):
  return (vp * len(v))(*v)


def resize(lib, xs=None, hs=None, ws=None, n=1, in_dtype=1, windows=None, q=1, S=8, out=FAKE, out_dtype=1):
  xs = ptrs(FAKE) if xs is None else xs
  hs = ints(20) if hs is None else hs
  ws = ints(30) if ws is None else ws
  windows = ints(0, 1, 2, 16) if windows is None else windows
  return lib.expo_area_resize_ragged(xs, hs, ws, n, in_dtype, windows, q, S, vp(out), out_dtype, None)


def test_symbols_exported_declared_and_bound():
  lib = ctypes.CDLL(_cabi.LIB_PATH)
  for name in NAMES:
    assert hasattr(lib, name) and name in _cabi.SIGNATURES and name in test_cabi_symbols.header_symbols(), name
  assert _cabi.load().expo_version() == 9


def test_area_resize_validation_before_enqueue():
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  assert resize(lib, n=-1) == -1 and resize(lib, q=-1) == -1
  assert resize(lib, in_dtype=2) == -2 and resize(lib, out_dtype=-1) == -2
  assert resize(lib, q=0, xs=ctypes.cast(None, ctypes.POINTER(vp))) == 0  # q == 0: no-op
  assert lib.expo_area_resize_ragged(None, None, None, 0, 1, None, 0, 8, None, 1, None) == 0
  assert resize(lib, n=0) == -1 and b'n == 0' in err()
  assert resize(lib, S=0) == -1
  for kw in (dict(xs=ctypes.cast(None, ctypes.POINTER(vp))), dict(hs=ctypes.cast(None, ctypes.POINTER(ctypes.c_int))),
             dict(windows=ctypes.cast(None, ctypes.POINTER(ctypes.c_int))), dict(out=None)):
    assert resize(lib, **kw) == -1 and b'null' in err(), kw
  assert resize(lib, xs=ptrs(None)) == -1 and b'null image' in err()
  assert resize(lib, hs=ints(0)) == -1 and resize(lib, ws=ints(-1)) == -1
  assert resize(lib, hs=ints(20000), ws=ints(9000)) == -1 and b'2 GiB' in err()
  # bad windows: image index, outside the image (every edge), upscaling, a side / S too large for one tile
  assert resize(lib, windows=ints(1, 0, 0, 16)) == -1 and b'image index' in err()
  assert resize(lib, windows=ints(-1, 0, 0, 16)) == -1
  for win in ((0, 5, 0, 16), (0, 0, 15, 16), (0, -1, 0, 16), (0, 0, -1, 16), (0, 0, 0, 21)):
    assert resize(lib, windows=ints(*win)) == -1 and b'outside' in err(), win
  assert resize(lib, windows=ints(0, 0, 0, 7)) == -1 and b'upscaling' in err()
  assert resize(lib, hs=ints(5000), ws=ints(5000), windows=ints(0, 0, 0, 4095), S=1) == -1 and b'tile' in err()
  # the LAST window of several is checked before anything is enqueued
  assert resize(lib, windows=ints(0, 0, 0, 16, 0, 0, 0, 16, 0, 4, 0, 17), q=3) == -1 and b'outside' in err()


def test_pack_recut_validation_before_enqueue():
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  call = lambda master=FAKE, m=4, S=80, rec=FAKE, count=3, C=64, out=FAKE, dtype=1: lib.expo_pack_recut(
      vp(master), m, S, vp(rec), count, C, vp(out), dtype, None)
  assert call(dtype=3) == -2
  assert call(count=-1) == -1
  assert call(C=81) == -1 and call(C=0) == -1 and call(S=0) == -1
  assert call(master=None, rec=None, out=None, count=0) == 0  # count == 0: no-op
  assert call(m=0) == -1
  for kw in (dict(master=None), dict(rec=None), dict(out=None)):
    assert call(**kw) == -1 and b'null' in err(), kw


def test_datasets_unit_isa_sanity(tmp_path):
  if not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)):
    pytest.skip('hipcc not available')
  txt = isa._listing(('datasets.hip', []), str(tmp_path))
  assert 'area_resize_kernel' in txt and 'pack_recut_kernel' in txt
  isa.test_streaming_kernels_do_not_spill({'datasets.hip': txt})
  # (its stores are global stores of one register each: the buffer-store pattern has nothing to inspect here)
  assert 'buffer_store_dwordx' not in txt
