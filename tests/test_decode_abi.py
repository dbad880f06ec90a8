"""CPU: expo_decode_ragged / expo_decode_workspace_bytes are exported and validate everything before anything is
enqueued (every failing call below would otherwise dereference fake device pointers); the decode unit's ISA passes the
checks of tests/test_isa_sanity.py (that file's UNITS list is the build's first seven units)."""
import ctypes
import os
import shutil

import pytest

from exposure_amd import _cabi
from tests import test_isa_sanity as isa

vp = ctypes.c_void_p
FAKE = 0x1000  # never dereferenced on the host


def ints(*v):
  return (ctypes.c_int * len(v))(*v)


def ptrs(*v):
  return (vp * len(v))(*v)


def call(lib, codes=None, hs=None, ws=None, n=1, channels=3, code_bits=8, table=FAKE, normalize=1, outs=None,
         dtype=0, workspace=FAKE, workspace_bytes=1 << 30):
  codes = ptrs(FAKE) if codes is None else codes
  outs = ptrs(FAKE) if outs is None else outs
  hs = ints(4) if hs is None else hs
  ws = ints(4) if ws is None else ws
  return lib.expo_decode_ragged(codes, hs, ws, n, channels, code_bits, vp(table), normalize, outs, dtype, vp(workspace),
                                workspace_bytes, None)


def test_symbols_exported():
  lib = ctypes.CDLL(_cabi.LIB_PATH)
  assert hasattr(lib, 'expo_decode_ragged') and hasattr(lib, 'expo_decode_workspace_bytes')
  assert 'expo_decode_ragged' in _cabi.SIGNATURES and 'expo_decode_workspace_bytes' in _cabi.SIGNATURES
  assert _cabi.load().expo_version() == 9


def test_validation_before_enqueue():
  lib = _cabi.load()
  err = lambda: lib.expo_last_error()
  assert call(lib, n=-1) == -1
  assert call(lib, channels=2) == -1 and b'channels' in err()
  assert call(lib, code_bits=12) == -1 and b'code_bits' in err()
  assert call(lib, normalize=2) == -1 and b'normalize' in err()
  assert call(lib, dtype=7) == -2
  assert lib.expo_decode_ragged(None, None, None, 0, 3, 8, None, 1, None, 0, None, 0, None) == 0  # n == 0: no-op
  assert lib.expo_decode_ragged(None, None, None, 0, 3, 8, None, 1, None, 9, None, 0, None) == -2
  for kw in (dict(codes=ctypes.cast(None, ctypes.POINTER(vp))), dict(outs=ctypes.cast(None, ctypes.POINTER(vp))),
             dict(table=None)):
    assert call(lib, **kw) == -1 and b'null' in err(), kw
  assert lib.expo_decode_ragged(ptrs(FAKE), None, ints(4), 1, 3, 8, vp(FAKE), 0, ptrs(FAKE), 0, None, 0, None) == -1
  assert call(lib, codes=ptrs(FAKE, None), outs=ptrs(FAKE, FAKE), hs=ints(4, 4), ws=ints(4, 4), n=2) == -1
  assert b'null image' in err()
  assert call(lib, outs=ptrs(None)) == -1 and b'null image' in err()
  assert call(lib, hs=ints(0)) == -1 and call(lib, ws=ints(-3)) == -1
  assert call(lib, hs=ints(4, 0), ws=ints(4, 4), n=2, codes=ptrs(FAKE, FAKE), outs=ptrs(FAKE, FAKE)) == -1
  # an output of 2 GiB or more (fp32: 12 B/px), codes of 2 GiB or more (16-bit RGBA: 8 B/px against fp16's 6)
  assert call(lib, hs=ints(20000), ws=ints(9000), dtype=1) == -1 and b'2 GiB' in err()
  assert call(lib, hs=ints(16384), ws=ints(16384), channels=4, code_bits=16) == -1 and b'2 GiB' in err()
  # the workspace of a normalising call: present, 4-byte aligned, large enough
  need = lib.expo_decode_workspace_bytes(1, ints(4), ints(4), 3, 8)
  assert call(lib, workspace=None) == -1 and b'workspace' in err()
  assert call(lib, workspace=FAKE + 2) == -1 and b'workspace' in err()
  assert call(lib, workspace_bytes=need - 1) == -1 and b'workspace' in err()


def test_workspace_bytes():
  lib = _cabi.load()
  wb = lambda hs, ws, c=3, bits=8: lib.expo_decode_workspace_bytes(len(hs), ints(*hs), ints(*ws), c, bits)
  assert lib.expo_decode_workspace_bytes(0, None, None, 3, 8) == 0
  assert lib.expo_decode_workspace_bytes(1, None, ints(4), 3, 8) == 0
  assert wb([0], [4]) == 0 and wb([4], [-1]) == 0 and wb([4], [4], c=2) == 0 and wb([4], [4], bits=10) == 0
  assert wb([4, 4], [4, 0]) == 0
  one = wb([4], [4])
  assert one >= 256 * 4  # the normalised table of one 8-bit image
  assert wb([4000], [6000]) > one and wb([4000], [6000], bits=16) >= 65536 * 4
  assert wb([4000], [6000], c=4) >= wb([4000], [6000], c=3)
  assert wb([8] * 64, [8] * 64) >= 64 * 256 * 4
  # launches of 64 images reuse the workspace: 65 small images need no more than 64 + room for one more record set
  assert wb([8] * 65, [8] * 65) == wb([8] * 64, [8] * 64)
  assert _cabi.decode_workspace_bytes([4000, 17], [6000, 9], 3, 16) == wb([4000, 17], [6000, 9], bits=16)


def test_decode_unit_isa_sanity(tmp_path):
  if not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)):
    pytest.skip('hipcc not available')
  txt = isa._listing(('decode.hip', []), str(tmp_path))
  assert 'v_div_fixup_f32' in txt  # the normalising division is the IEEE one, not a reciprocal multiply
  isa.test_no_store_takes_its_address_from_its_own_data_registers({'decode.hip': txt})
  isa.test_streaming_kernels_do_not_spill({'decode.hip': txt})
