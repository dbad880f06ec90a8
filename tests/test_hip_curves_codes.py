"""GPU: expo_chain_fused_curves_fwd_ragged_codes -- the fused inference pass for any cfg.curve_steps
straight from the integer codes -- against the pair it replaces on the same inputs: decode_ragged, then
chain_fused_curves_fwd_ragged on the decoded tensors with the same ids, rows, L and taps.  That pair is held to the
float64 oracle by tests/test_hip_decode.py and tests/test_hip_curves_chain.py; agreement with it is bit for bit, no
tolerance: the new kernel performs the same rounded operations on the same values.  Every comparison is of raw bytes
(uint16 has no comparison kernels of its own).  Then evaluate.retouch_batch_raw(curves='fused') and the CLI's
--fused-decode-curves against the decoded path."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate
from exposure_amd import agent as xagent
from exposure_amd.config import make_cfg
from tests.test_hip_curves_chain import SEQUENCES, make_rows
from tests.test_hip_decode import codes_of
from tests.test_hip_fused_decode import (DEV, DTYPES, KINDS, PASS_SIZES, TAP_DTYPES, _mixed_raws, _same_result,
                                         _write_files, decoded, guarded, guards_intact, same, tables_of, upload)

pytestmark = pytest.mark.gpu

LS = (1, 5, 8, 16)
W24, W48 = _cabi.EXPO_MAX_PARAMS, _cabi.EXPO_MAX_PARAMS_CURVES
# (1, 1): one pixel; (3, 5): an odd pixel count (fp16: element-wise path); (61, 94), (67, 129): partial last chunks, more
# than one block; (40, 56): whole vectors only
assert PASS_SIZES == [(1, 1), (3, 5), (61, 94), (67, 129), (40, 56)]
NO_CURVE = np.array([[0, 1, 2, 3, 5, 6, 8], [8, 6, 5, -1, 3, 2, 1], [3, 3, 0, 8, 6, 2, 5], [1, 5, 8, 0, 2, 6, 3],
                     [2, 0, 6, 5, 1, 8, -1]], dtype=np.int32)


def rows(rng, L, steps, n=5):
  """ids (n, steps) and rows (n, steps, 48) on the device: tests/test_hip_curves_chain.py's sequences -- Tone and Color
  at several steps and back to back, -1 at the start, in the middle and (image 4) at the end -- with the oracle's
  regressors' values and 1e30 in every entry a filter does not use"""
  ids = SEQUENCES[np.arange(n) % 5, :steps].copy()
  if steps:
    ids[4::5, steps - 1] = -1
  p = make_rows(rng, ids, L)
  return torch.from_numpy(np.ascontiguousarray(ids)).to(DEV), torch.from_numpy(p).to(DEV)


def reference_pass(xs, ids, p, L, mask, tap_dtype, with_y):
  ys = [torch.empty_like(x) for x in xs] if with_y else None
  t = bin(mask).count('1')
  taps = [torch.empty((t,) + tuple(x.shape[-3:]), dtype=tap_dtype or x.dtype, device=DEV) for x in xs] if t else None
  _cabi.chain_fused_curves_fwd_ragged(ids, p, L, xs, ys, mask, taps)
  return ys, taps


def codes_pass(cs, tables, stride, ids, p, L, mask, tap_dtype, with_y, dtype, y_off=0, tap_off=0):
  """the pass from codes into guarded buffers; the guards are checked"""
  t = bin(mask).count('1')
  tdt = tap_dtype or dtype
  yb = [guarded((1, c.shape[0], c.shape[1], 3), dtype, y_off) for c in cs] if with_y else None
  tb = [guarded((t, c.shape[0], c.shape[1], 3), tdt, tap_off) for c in cs] if t else None
  ys = [y for _b, y in yb] if with_y else None
  taps = [tp for _b, tp in tb] if t else None
  _cabi.chain_fused_curves_fwd_ragged_codes(ids, p, L, cs, tables, stride, ys, mask, taps)
  torch.cuda.synchronize()
  for b, y in yb or ():
    assert guards_intact(b, y, dtype), 'y guards'
  for b, tp in tb or ():
    assert guards_intact(b, tp, tdt), 'tap guards'
  return ys, taps


def compare(cs, xs, tables, stride, ids, p, L, mask, tdt, with_y, dtype, what, **off):
  want_y, want_t = reference_pass(xs, ids, p, L, mask, tdt, with_y)
  got_y, got_t = codes_pass(cs, tables, stride, ids, p, L, mask, tdt, with_y, dtype, **off)
  for i in range(len(cs)):
    if with_y:
      same(got_y[i], want_y[i], '%s: y[%d]' % (what, i))
    if mask:
      same(got_t[i], want_t[i], '%s: taps[%d]' % (what, i))
  return got_y, got_t


_INPUTS = {}


def inputs(kind, c, dtype):
  """the codes of PASS_SIZES, their decoded tensors and their tables, made once per (kind, channels, dtype)"""
  key = (kind, c, dtype)
  if key not in _INPUTS:
    rng = np.random.default_rng(170 + 10 * KINDS.index(kind) + c)
    cs = upload([np.maximum(codes_of(rng, kind, h, w, c), 1) for h, w in PASS_SIZES])
    _INPUTS[key] = (cs, decoded(cs, kind, dtype)) + tuple(tables_of(cs, kind, dtype))
  return _INPUTS[key]


# ---------------------------------------------------------------------------------------------------- main grid
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', (1, 3, 4))
@pytest.mark.parametrize('dtype', DTYPES)
def test_pass_from_codes_equals_pass_of_decoded(kind, c, dtype, L):
  """8 steps; 5 and 1 (odd: the loop ends on the identity half-trip); 0 (the output is the gathered input)"""
  cs, xs, tables, stride = inputs(kind, c, dtype)
  assert (stride == 0) == (kind == 'prophoto16')  # the one shared table / a normalised table per image
  rng = np.random.default_rng(1000 * L + c)
  for steps in (8, 5, 1, 0):
    ids, p = rows(rng, L, steps)
    got_y, _ = compare(cs, xs, tables, stride, ids, p, L, 0, None, True, dtype, 'L %d, %d steps' % (L, steps))
    if steps == 0:
      for y, x in zip(got_y, xs):
        same(y, x, 'no steps')
    elif steps > 1:
      assert not got_y[4].view(-1).view(torch.uint8).any()  # after a trailing -1: exactly +0


# ---------------------------------------------------------------------------------------------------- taps
@pytest.mark.parametrize('L', (5, 16))
@pytest.mark.parametrize('kind,c', [('srgb8', 3), ('srgb8', 1), ('srgb16', 4), ('prophoto16', 3)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_taps(kind, c, dtype, L):
  cs, xs, tables, stride = inputs(kind, c, dtype)
  steps = 7
  ids, p = rows(np.random.default_rng(L), L, steps)
  for fmt, tdt in TAP_DTYPES.items():
    for mask in (0b1010101, 0b0001100, 1 << (steps - 1)):  # sparse; around adjacent curve steps; the last step alone
      for with_y in (True, False):
        compare(cs, xs, tables, stride, ids, p, L, mask, tdt, with_y, dtype,
                '%s mask 0x%x ys %s' % (fmt, mask, with_y))


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize('bits', (8, 16))
def test_pass_reads_every_table_entry(bits):
  """every code below the largest appears (the image of tests/test_hip_decode.py)"""
  hi = 1 << bits
  ct = np.uint8 if bits == 8 else np.uint16
  rng = np.random.default_rng(hi)
  h, w = (16, 16) if bits == 8 else (128, 171)
  img = rng.permutation(np.arange(h * w * 3) % (hi - 1)).astype(ct).reshape(h, w, 3)
  img[h // 2, w // 3, 2] = hi - 1
  cs = upload([img])
  L, steps = 5, 5
  ids, p = rows(rng, L, steps)
  ids, p = ids[1:2].contiguous(), p[1:2].contiguous()  # Level, Tone, Color, Tone, Exposure
  for kind in (('srgb8',) if bits == 8 else ('srgb16', 'prophoto16')):
    for dt in DTYPES:
      xs = decoded(cs, kind, dt)
      tables, stride = tables_of(cs, kind, dt)
      compare(cs, xs, tables, stride, ids, p, L, 1 << (steps - 1), torch.uint16, True, dt, '%s %s' % (kind, dt))
      compare(cs, xs, tables, stride, ids[:, :0].contiguous(), p[:, :0].contiguous(), L, 0, None, True, dt, 'gather')


# ---------------------------------------------------------------------------------------------------- ragged counts
@pytest.mark.parametrize('n', (1, 64, 65))
def test_ragged_counts_equal_single_calls(n):
  """the launch split at 64 images: the tables, ids and params of the second launch start at image 64"""
  rng = np.random.default_rng(n)
  L, steps = 5, 3
  for kind, c, dt in (('srgb8', 3, torch.float16), ('srgb16', 4, torch.float32)):
    sizes = [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(n)]
    cs = upload([np.maximum(codes_of(rng, kind, h, w, c), 1) for h, w in sizes])
    tables, stride = tables_of(cs, kind, dt)
    ids, p = rows(rng, L, 8, n)
    ids, p = ids[:, 2:2 + steps].contiguous(), p[:, 2:2 + steps].contiguous()  # columns 2..4: Tone / Color in most rows
    mask = 1 << (steps - 1)
    ys, taps = compare(cs, decoded(cs, kind, dt), tables, stride, ids, p, L, mask, torch.uint8, True, dt, 'n %d' % n)
    for i in range(n):
      t1 = tables[i * stride // tables.shape[1]][None].contiguous()
      y1, tp1 = codes_pass(cs[i:i + 1], t1, stride, ids[i:i + 1].contiguous(), p[i:i + 1].contiguous(), L, mask,
                           torch.uint8, True, dt)
      same(ys[i], y1[0], 'y[%d]' % i)
      same(taps[i], tp1[0], 'taps[%d]' % i)


# ---------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize('kind', KINDS)
def test_odd_offsets_and_guards(kind):
  """codes at odd element offsets inside one buffer, outputs and u8 / u16 tap planes at odd offsets inside guard-filled
  buffers: the element-wise path per image; values equal, guards intact"""
  rng = np.random.default_rng(3 + KINDS.index(kind))
  ct = torch.uint8 if kind == 'srgb8' else torch.uint16
  sizes = [(7, 9), (16, 32), (5, 5), (40, 56)]
  L = 16
  for c in (1, 3, 4):
    codes = [np.maximum(codes_of(rng, kind, h, w, c), 1) for h, w in sizes]
    buf = torch.zeros(sum(cd.size for cd in codes) + 16, dtype=ct, device=DEV)
    views, at = [], 1
    for cd in codes:
      v = buf[at:at + cd.size].view(cd.shape)
      v.copy_(torch.from_numpy(cd).to(DEV))
      views.append(v)
      at += cd.size + 2 - (cd.size % 2)  # every view starts at an odd element
    assert all((v.data_ptr() // v.element_size()) % 2 == 1 for v in views)
    aligned = upload(codes)
    ids, p = rows(rng, L, 5, len(codes))
    mask = 0b10101
    for dt in DTYPES:
      xs = decoded(aligned, kind, dt)
      tables, stride = tables_of(aligned, kind, dt)
      for tdt in (torch.uint8, torch.uint16):
        for src, y_off, tap_off in ((views, 1, 1), (aligned, 1, 1), (aligned, 0, 1), (views, 0, 0)):
          compare(src, xs, tables, stride, ids, p, L, mask, tdt, True, dt,
                  'C %d %s %s offsets %d %d' % (c, dt, tdt, y_off, tap_off), y_off=y_off, tap_off=tap_off)
    assert bool((buf[at:] == 0).all()) and int(buf[0]) == 0


# ---------------------------------------------------------------------------------------------------- no-curve rows
@pytest.mark.parametrize('L', (3, 16))
@pytest.mark.parametrize('kind,c', [('srgb8', 4), ('srgb16', 1), ('prophoto16', 3)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_without_a_curve_step_the_bits_are_the_8_step_pass_from_codes(kind, c, dtype, L):
  """the promise chain_fused_curves.hip makes for the steps that are no curve, from codes: the same values in 24-wide
  rows through chain_fused_fwd_ragged_codes"""
  cs, _xs, tables, stride = inputs(kind, c, dtype)
  p48 = make_rows(np.random.default_rng(17 + L), NO_CURVE, L)
  ids = torch.from_numpy(NO_CURVE).to(DEV)
  p24 = torch.from_numpy(np.ascontiguousarray(p48[:, :, :W24])).to(DEV)
  mask = 0b1000101
  got_y, got_t = codes_pass(cs, tables, stride, ids, torch.from_numpy(p48).to(DEV), L, mask, torch.uint16, True, dtype)
  want_y = [torch.empty_like(y) for y in got_y]
  want_t = [torch.empty_like(t) for t in got_t]
  _cabi.chain_fused_fwd_ragged_codes(ids, p24, cs, tables, stride, want_y, mask, want_t)
  torch.cuda.synchronize()
  for i in range(len(cs)):
    same(got_y[i], want_y[i], 'y[%d]' % i)
    same(got_t[i], want_t[i], 'taps[%d]' % i)


# ---------------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize('dtype,side,kind,c', [(torch.float16, 1200, 'srgb16', 3), (torch.float32, 840, 'srgb8', 4)])
def test_streaming_instantiations_every_pixel(dtype, side, kind, c):
  """one image of at least 8 MiB of output (stream_min_bytes): the IoStream kernels, without taps and with a u8 tap of
  the last step; L = 12, 5 steps with Tone and Color"""
  assert side * side * 3 * (2 if dtype == torch.float16 else 4) >= 8 << 20
  rng = np.random.default_rng(77)
  L = 12
  cs = upload([np.maximum(codes_of(rng, kind, side, side, c), 1)])
  ids = torch.tensor([[1, 4, 7, 5, 4]], dtype=torch.int32, device=DEV)
  p = torch.from_numpy(make_rows(rng, ids.cpu().numpy(), L)).to(DEV)
  xs = decoded(cs, kind, dtype)
  tables, stride = tables_of(cs, kind, dtype)
  compare(cs, xs, tables, stride, ids, p, L, 0, None, True, dtype, 'streaming')
  compare(cs, xs, tables, stride, ids, p, L, 1 << 4, torch.uint8, True, dtype, 'streaming, u8 tap')


# ---------------------------------------------------------------------------------------------------- Python level
@pytest.mark.parametrize('dispatch', (False, True))
@pytest.mark.parametrize('L', (4, 16))
def test_retouch_batch_raw_fused_curves_equals_retouch_batch_of_decoded(L, dispatch):
  torch.manual_seed(11)
  rng = np.random.default_rng(11)
  cfg = make_cfg()
  cfg.curve_steps = L
  agent = xagent.Agent(cfg).to(DEV)
  agent.curve_dispatch = dispatch
  raws = _mixed_raws(rng)
  n = len(raws)
  z = torch.rand((n, cfg.z_dim), device=DEV)
  g = torch.Generator().manual_seed(42)
  drops = [[(torch.rand(n, 4096, generator=g) < 0.5).float().to(DEV) for _ in range(2)] for _ in range(cfg.test_steps)]
  names = ('outputs', 'low', 'states', 'trace', 'intermediates', 'pictures')
  for dtype, code in ((torch.float16, 'u8'), (torch.float32, 'u16')):
    images = evaluate.decode_images(raws, dtype, DEV)
    kw = dict(z=z, dropout_masks=drops, return_trace='full', intermediates=code, picture=code)
    want = evaluate.retouch_batch(agent, images, proxy='device', curves='fused', **kw)
    got = evaluate.retouch_batch_raw(agent, raws, dtype, DEV, curves='fused', **kw)
    assert len(got) == len(want) == 6 and got[3]['params48'].shape == (n, cfg.test_steps, W48)
    for name, a, b in zip(names, got, want):
      _same_result(a, b, '%s %s' % (dtype, name))
    bare = evaluate.retouch_batch_raw(agent, raws, dtype, DEV, outputs=False, curves='fused', **kw)
    assert bare[0] == [None] * n
    _same_result(bare[-1], want[-1], 'pictures without outputs')
    _same_result(bare[-2], want[-2], 'intermediates without outputs')
  with pytest.raises(ValueError, match='curve_steps'):
    evaluate.retouch_batch_raw(agent, raws, torch.float16, DEV)


# ---------------------------------------------------------------------------------------------------- CLI
def test_cli_fused_decode_curves_writes_the_same_files(tmp_path):
  paths = _write_files(tmp_path)
  common = ['--curve-steps', '4', '--device-png', '--step-by-step', '--batch', '4', '--seed', '3']
  runs = {}
  for name, extra in (('parent', ['--device-decode', '--device-proxy', '--fused-curves']),
                      ('fused', ['--fused-decode-curves']), ('pictures', ['--fused-decode-curves', '--pictures-only'])):
    out = str(tmp_path / name) + os.sep
    runs[name] = evaluate.main(common + extra + ['--out', out] + paths)
  assert len(runs['parent']) == len(runs['fused']) == len(runs['pictures']) == len(paths)
  for a, b, c in zip(runs['parent'], runs['fused'], runs['pictures']):
    assert a['filters'] == b['filters'] and a['states'] == b['states'] and a['abi_filter_ids'] == b['abi_filter_ids']
    assert open(a['output'], 'rb').read() == open(b['output'], 'rb').read() and c['output'] is None
    assert sorted(a['png']) == sorted(b['png']) == sorted(c['png']) and len(a['png']) == 5
    for k in a['png']:
      want = open(a['png'][k], 'rb').read()
      assert open(b['png'][k], 'rb').read() == want, k
      assert open(c['png'][k], 'rb').read() == want, k
  assert sorted(os.listdir(str(tmp_path / 'parent'))) == sorted(os.listdir(str(tmp_path / 'fused')))
  assert not [f for f in os.listdir(str(tmp_path / 'pictures')) if f.endswith('.npy')]
