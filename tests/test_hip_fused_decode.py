"""GPU: inference straight from the integer codes -- expo_decode_tables,
expo_bilinear_resize_ragged_codes and expo_chain_fused_fwd_ragged_codes against the path they replace on the same
inputs: decode_ragged, then bilinear_resize_ragged / chain_fused_fwd_ragged[_taps].  That path is held to the float64
oracle by the rest of the suite; agreement with it is bit for bit, no tolerance: the new kernels perform the same rounded
operations on the same values.  No comparison feeds a NaN table (an all-zero sRGB image) to the pass or the proxy: only
the tables export is checked on one.  uint16 tensors are compared through their bytes."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate
from exposure_amd import agent as xagent
from exposure_amd.config import make_cfg
from exposure_amd.tiff16 import write_tiff
from tests.test_hip_chain_taps import GUARD
from tests.test_hip_decode import codes_of
from tests.test_hip_ragged_chain import make_sequences

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
KINDS = ('srgb8', 'srgb16', 'prophoto16')
DTYPES = (torch.float16, torch.float32)
# (1, 1): one pixel; (3, 5): an odd pixel count (fp16: element-wise path); (61, 94), (40, 56): the vector path with a
# partial last chunk; (67, 129): more than one block per image, odd again
SIZES = [(1, 1), (3, 5), (61, 94), (67, 129)]
PASS_SIZES = SIZES + [(40, 56)]
STEPS = 5
SENTINEL = {torch.uint8: 0xA5, torch.uint16: 0x5A5B, torch.float16: 1234.0, torch.float32: -777.0}
TAP_DTYPES = {'storage': None, 'u8': torch.uint8, 'u16': torch.uint16}


def raw(t):
  """a tensor's bytes (uint16 has no comparison kernels of its own)"""
  return t.contiguous().view(-1).view(torch.uint8)


def same(got, want, what=''):
  assert got.shape == want.shape and got.dtype == want.dtype, what
  bad = int((raw(got) != raw(want)).sum())
  assert bad == 0, '%s: %d bytes differ' % (what, bad)


def upload(codes):
  return [torch.from_numpy(np.ascontiguousarray(c)).to(DEV) for c in codes]


def decoded(cs, kind, dtype):
  """the yardstick's first stage: the float tensors decode_ragged makes of the codes"""
  ys = [torch.empty((1, c.shape[0], c.shape[1], 3), dtype=dtype, device=DEV) for c in cs]
  _cabi.decode_ragged(cs, evaluate.decode_table(kind, DEV), evaluate.DECODE_NORMALIZE[kind], ys)
  return ys


def tables_of(cs, kind, dtype):
  return _cabi.decode_tables(cs, evaluate.decode_table(kind, DEV), evaluate.DECODE_NORMALIZE[kind], dtype)


def guarded(shape, dtype, off=0):
  """a contiguous tensor of `shape` inside a buffer with GUARD sentinel elements on both sides, `off` elements in"""
  numel = int(np.prod(shape))
  store = torch.int16 if dtype is torch.uint16 else dtype
  buf = torch.full((GUARD + off + numel + GUARD,), SENTINEL[dtype], dtype=store, device=DEV)
  t = buf[GUARD + off:GUARD + off + numel].view(*shape)
  return buf, (t.view(torch.uint16) if dtype is torch.uint16 else t)


def guards_intact(buf, t, dtype):
  start = (t.data_ptr() - buf.data_ptr()) // buf.element_size()
  head, tail = buf[:start], buf[start + t.numel():]
  s = SENTINEL[dtype]
  return head.numel() >= GUARD and tail.numel() >= GUARD and bool((head == s).all()) and bool((tail == s).all())


def sequences(rng, n):
  ids, p = make_sequences(rng, max(n, 5), STEPS)  # ids 0..8 and -1: image 0 starts with -1, image 2 ends with it
  return torch.from_numpy(ids[:n]).to(DEV), torch.from_numpy(p[:n]).to(DEV)


def reference_pass(xs, ids, p, mask, tap_dtype, with_y):
  ys = [torch.empty_like(x) for x in xs] if with_y else None
  t = bin(mask).count('1')
  taps = [torch.empty((t,) + tuple(x.shape[-3:]), dtype=tap_dtype or x.dtype, device=DEV) for x in xs] if t else None
  _cabi.chain_fused_fwd_ragged_taps(ids, p, xs, ys, mask, taps)
  return ys, taps


def codes_pass(cs, tables, stride, ids, p, mask, tap_dtype, with_y, dtype, y_off=0, tap_off=0):
  """the pass from codes into guarded buffers; the guards are checked"""
  t = bin(mask).count('1')
  tdt = tap_dtype or dtype
  yb = [guarded((1, c.shape[0], c.shape[1], 3), dtype, y_off) for c in cs] if with_y else None
  tb = [guarded((t, c.shape[0], c.shape[1], 3), tdt, tap_off) for c in cs] if t else None
  ys = [y for _b, y in yb] if with_y else None
  taps = [tp for _b, tp in tb] if t else None
  _cabi.chain_fused_fwd_ragged_codes(ids, p, cs, tables, stride, ys, mask, taps)
  torch.cuda.synchronize()
  for b, y in yb or ():
    assert guards_intact(b, y, dtype), 'y guards'
  for b, tp in tb or ():
    assert guards_intact(b, tp, tdt), 'tap guards'
  return ys, taps


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_tables_gathered_on_the_host_reproduce_decode(kind, dtype):
  rng = np.random.default_rng(31 + KINDS.index(kind))
  hi = 256 if kind == 'srgb8' else 65536
  codes = [codes_of(rng, kind, 9, 14, 3) // 2, codes_of(rng, kind, 33, 20, 4) // 3, codes_of(rng, kind, 5, 7, 1)]
  codes[1][16, 10, 3] = hi - 1  # only alpha holds the largest code: it must not count
  for cd in codes:  # one call per channel count
    cs = upload([cd])
    tables, stride = tables_of(cs, kind, dtype)
    norm = evaluate.DECODE_NORMALIZE[kind]
    assert stride == (hi if norm else 0) and tuple(tables.shape) == (1, hi) and tables.dtype == dtype
    c3 = np.repeat(cd, 3, axis=2) if cd.shape[2] == 1 else cd[:, :, :3]
    got = tables[0].cpu()[torch.from_numpy(c3.astype(np.int64))]
    same(got, decoded(cs, kind, dtype)[0][0].cpu(), 'C = %d' % cd.shape[2])
  # several images in one call: image i's table in row i (or the one shared table)
  same_c = [np.maximum(codes_of(rng, kind, h, w, 3) // (i + 1), 1) for i, (h, w) in enumerate(SIZES)]
  cs = upload(same_c)
  tables, stride = tables_of(cs, kind, dtype)
  for i, (cd, want) in enumerate(zip(same_c, decoded(cs, kind, dtype))):
    row = tables[i * stride // hi].cpu()
    same(row[torch.from_numpy(cd.astype(np.int64))], want[0].cpu(), 'image %d' % i)


@pytest.mark.parametrize('kind', ('srgb8', 'srgb16'))
def test_tables_of_an_all_zero_image_are_nan(kind):
  ct = np.uint8 if kind == 'srgb8' else np.uint16
  img4 = np.zeros((33, 17, 4), dtype=ct)
  img4[..., 3] = 200  # alpha does not count
  live = np.full((4, 4, 4), 9, dtype=ct)
  for dt in DTYPES:
    tables, _stride = tables_of(upload([live, img4]), kind, dt)
    assert torch.isnan(tables[1].float()).all() and not torch.isnan(tables[0].float()).any()


# ---------------------------------------------------------------------------------------------------- proxy
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', (1, 3, 4))
def test_proxy_from_codes_equals_proxy_of_decoded(kind, c):
  rng = np.random.default_rng(50 + 10 * KINDS.index(kind) + c)
  codes = [np.maximum(codes_of(rng, kind, h, w, c), 1) for h, w in SIZES]
  cs = upload(codes)
  windows = evaluate.center_windows(SIZES) + [(3, 5, 60, 23), (2, 0, 0, 61)]  # (3, ...): a window smaller than S
  S = 64
  for dt in DTYPES:
    tables, stride = tables_of(cs, kind, dt)
    want = torch.empty((len(windows), S, S, 3), dtype=dt, device=DEV)
    _cabi.bilinear_resize_ragged(decoded(cs, kind, dt), windows, S, want)
    got = torch.empty_like(want)
    _cabi.bilinear_resize_ragged_codes(cs, tables, stride, windows, S, got)
    torch.cuda.synchronize()
    same(got, want, str(dt))


# ---------------------------------------------------------------------------------------------------- pass
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', (1, 3, 4))
@pytest.mark.parametrize('dtype', DTYPES)
def test_pass_from_codes_equals_pass_of_decoded(kind, c, dtype):
  rng = np.random.default_rng(70 + 10 * KINDS.index(kind) + c)
  codes = [np.maximum(codes_of(rng, kind, h, w, c), 1) for h, w in PASS_SIZES]
  cs = upload(codes)
  xs = decoded(cs, kind, dtype)
  tables, stride = tables_of(cs, kind, dtype)
  ids, p = sequences(rng, len(codes))
  assert int((ids[0] == -1).sum()) == 1
  for fmt, tdt in [('none', None)] + list(TAP_DTYPES.items()):
    for mask in ((0,) if fmt == 'none' else (0b10101, 1 << (STEPS - 1))):
      for with_y in ((True,) if fmt == 'none' else (True, False)):
        what = '%s mask 0x%x ys %s' % (fmt, mask, with_y)
        want_y, want_t = reference_pass(xs, ids, p, mask, tdt, with_y)
        got_y, got_t = codes_pass(cs, tables, stride, ids, p, mask, tdt, with_y, dtype)
        for i in range(len(codes)):
          if with_y:
            same(got_y[i], want_y[i], '%s: y[%d]' % (what, i))
          if mask:
            same(got_t[i], want_t[i], '%s: taps[%d]' % (what, i))


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
  ids, p = sequences(rng, 5)
  ids, p = ids[3:4].contiguous(), p[3:4].contiguous()
  for kind in (('srgb8',) if bits == 8 else ('srgb16', 'prophoto16')):
    for dt in DTYPES:
      xs = decoded(cs, kind, dt)
      tables, stride = tables_of(cs, kind, dt)
      want_y, want_t = reference_pass(xs, ids, p, 1 << (STEPS - 1), torch.uint16, True)
      got_y, got_t = codes_pass(cs, tables, stride, ids, p, 1 << (STEPS - 1), torch.uint16, True, dt)
      same(got_y[0], want_y[0], 'y %s %s' % (kind, dt))
      same(got_t[0], want_t[0], 'tap %s %s' % (kind, dt))
      S = 64
      low_w = torch.empty((1, S, S, 3), dtype=dt, device=DEV)
      _cabi.bilinear_resize_ragged(xs, evaluate.center_windows([(h, w)]), S, low_w)
      low = torch.empty_like(low_w)
      _cabi.bilinear_resize_ragged_codes(cs, tables, stride, evaluate.center_windows([(h, w)]), S, low)
      same(low, low_w, 'proxy %s %s' % (kind, dt))


@pytest.mark.parametrize('n', (1, 64, 65))
def test_ragged_counts_equal_single_calls(n):
  """the launch split at 64 images: the tables, ids and params of the second launch start at image 64"""
  rng = np.random.default_rng(n)
  for kind, c, dt in (('srgb8', 3, torch.float16), ('srgb16', 4, torch.float32)):
    sizes = [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(n)]
    cs = upload([np.maximum(codes_of(rng, kind, h, w, c), 1) for h, w in sizes])
    tables, stride = tables_of(cs, kind, dt)
    ids5, p5 = sequences(rng, 5)
    sel = torch.arange(n, device=DEV) % 5
    ids, p = ids5[sel].contiguous(), p5[sel].contiguous()
    mask = 1 << (STEPS - 1)
    ys, taps = codes_pass(cs, tables, stride, ids, p, mask, torch.uint8, True, dt)
    for i in range(n):
      t1, s1 = tables_of(cs[i:i + 1], kind, dt)
      same(t1[0], tables[i * stride // tables.shape[1]], 'table %d' % i)
      y1, tp1 = codes_pass(cs[i:i + 1], t1, s1, ids[i:i + 1].contiguous(), p[i:i + 1].contiguous(), mask, torch.uint8,
                           True, dt)
      same(ys[i], y1[0], 'y[%d]' % i)
      same(taps[i], tp1[0], 'taps[%d]' % i)


@pytest.mark.parametrize('kind', KINDS)
def test_odd_offsets_and_guards(kind):
  """codes at odd element offsets inside one buffer, outputs and u8 / u16 tap planes at odd offsets inside guard-filled
  buffers: the element-wise path per image; values equal, guards intact"""
  rng = np.random.default_rng(3 + KINDS.index(kind))
  ct = torch.uint8 if kind == 'srgb8' else torch.uint16
  sizes = [(7, 9), (16, 32), (5, 5), (40, 56)]
  for c in (1, 3, 4):
    codes = [np.maximum(codes_of(rng, kind, h, w, c), 1) for h, w in sizes]
    total = sum(cd.size for cd in codes) + 16
    buf = torch.zeros(total, dtype=ct, device=DEV)
    views, at = [], 1
    for cd in codes:
      v = buf[at:at + cd.size].view(cd.shape)
      v.copy_(torch.from_numpy(cd).to(DEV))
      views.append(v)
      at += cd.size + 2 - (cd.size % 2)  # every view starts at an odd element
    assert all((v.data_ptr() // v.element_size()) % 2 == 1 for v in views)
    aligned = upload(codes)
    ids, p = sequences(rng, len(codes))
    mask = 0b10101
    for dt in DTYPES:
      xs = decoded(aligned, kind, dt)
      tables, stride = tables_of(views, kind, dt)
      same(tables, tables_of(aligned, kind, dt)[0], 'tables')
      S = 64
      windows = evaluate.center_windows(sizes)
      low_w = torch.empty((len(sizes), S, S, 3), dtype=dt, device=DEV)
      _cabi.bilinear_resize_ragged(xs, windows, S, low_w)
      low = torch.empty_like(low_w)
      _cabi.bilinear_resize_ragged_codes(views, tables, stride, windows, S, low)
      same(low, low_w, 'proxy')
      for tdt in (torch.uint8, torch.uint16):
        want_y, want_t = reference_pass(xs, ids, p, mask, tdt, True)
        for src, y_off, tap_off in ((views, 1, 1), (aligned, 1, 1), (aligned, 0, 1), (views, 0, 0)):
          got_y, got_t = codes_pass(src, tables, stride, ids, p, mask, tdt, True, dt, y_off, tap_off)
          for i in range(len(codes)):
            what = 'C %d %s %s image %d offsets %d %d' % (c, dt, tdt, i, y_off, tap_off)
            same(got_y[i], want_y[i], 'y ' + what)
            same(got_t[i], want_t[i], 'taps ' + what)


# ---------------------------------------------------------------------------------------------------- Python level
def _mixed_raws(rng):
  return [(codes_of(rng, 'srgb8', 40, 56, 3), 'srgb8'), (codes_of(rng, 'srgb8', 33, 21, 4), 'srgb8'),
          (codes_of(rng, 'srgb16', 25, 37, 1), 'srgb16'), (codes_of(rng, 'prophoto16', 30, 44, 3), 'prophoto16'),
          (codes_of(rng, 'srgb8', 64, 48, 3), 'srgb8')]


def _same_result(got, want, what):
  if isinstance(want, dict):
    assert sorted(got) == sorted(want), what
    for k in want:
      same(got[k], want[k], '%s[%s]' % (what, k))
  elif isinstance(want, (list, tuple)):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
      same(g, w, '%s[%d]' % (what, i))
  else:
    same(got, want, what)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('code', ('u8', 'u16'))
def test_retouch_batch_raw_equals_retouch_batch_of_decoded(dtype, code):
  torch.manual_seed(11)
  rng = np.random.default_rng(11)
  cfg = make_cfg()
  agent = xagent.Agent(cfg).to(DEV)
  raws = _mixed_raws(rng)
  n = len(raws)
  z = torch.rand((n, cfg.z_dim), device=DEV)
  g = torch.Generator().manual_seed(42)
  drops = [[(torch.rand(n, 4096, generator=g) < 0.5).float().to(DEV) for _ in range(2)] for _ in range(cfg.test_steps)]
  images = evaluate.decode_images(raws, dtype, DEV)
  kw = dict(z=z, dropout_masks=drops, return_trace='full', intermediates=code, picture=code)
  want = evaluate.retouch_batch(agent, images, proxy='device', **kw)
  got = evaluate.retouch_batch_raw(agent, raws, dtype, DEV, **kw)
  assert len(got) == len(want) == 6
  for name, g, w in zip(('outputs', 'low', 'states', 'trace', 'intermediates', 'pictures'), got, want):
    _same_result(g, w, name)
  bare = evaluate.retouch_batch_raw(agent, raws, dtype, DEV, outputs=False, **kw)
  assert bare[0] == [None] * n
  _same_result(bare[-1], want[-1], 'pictures without outputs')
  _same_result(bare[-2], want[-2], 'intermediates without outputs')
  # storage intermediates next to a picture: the pictures are encoded from the outputs
  kw.update(intermediates='storage')
  want = evaluate.retouch_batch(agent, images, proxy='device', **kw)
  got = evaluate.retouch_batch_raw(agent, raws, dtype, DEV, **kw)
  for name, g, w in zip(('outputs', 'low', 'states', 'trace', 'intermediates', 'pictures'), got, want):
    _same_result(g, w, 'storage: ' + name)


def test_retouch_batch_raw_refuses_masking():
  cfg = make_cfg()
  cfg.masking = True
  agent = xagent.Agent(cfg).to(DEV)
  with pytest.raises(ValueError, match='masking'):
    evaluate.retouch_batch_raw(agent, _mixed_raws(np.random.default_rng(1)), torch.float16, DEV)


# ---------------------------------------------------------------------------------------------------- CLI
def _write_files(tmp_path):
  from PIL import Image
  rng = np.random.default_rng(21)
  paths = []
  for i, (h, w, mode) in enumerate([(40, 56, 'RGB'), (33, 21, 'RGBA'), (64, 48, 'RGB')]):
    p = str(tmp_path / ('in%d.png' % i))
    Image.fromarray(rng.integers(1, 256, (h, w, len(mode)), dtype=np.uint8), mode).save(p)
    paths.append(p)
  p = str(tmp_path / 'grey16.png')
  Image.fromarray(rng.integers(1, 65536, (25, 37), dtype=np.uint16)).save(p)
  paths.append(p)
  for i, (h, w, c) in enumerate([(30, 44, 3), (25, 19, 4)]):
    p = str(tmp_path / ('in%d.tif' % i))
    write_tiff(p, rng.integers(1, 65536, (h, w, c), dtype=np.uint16))
    paths.append(p)
  return paths


def test_cli_fused_decode_writes_the_same_files(tmp_path):
  paths = _write_files(tmp_path)
  common = ['--device-png', '--step-by-step', '--batch', '4', '--seed', '3']
  runs = {}
  for name, extra in (('parent', ['--device-decode', '--device-proxy']), ('fused', ['--fused-decode']),
                      ('pictures', ['--fused-decode', '--pictures-only'])):
    out = str(tmp_path / name) + os.sep
    runs[name] = evaluate.main(common + extra + ['--out', out] + paths)
  assert len(runs['parent']) == len(runs['fused']) == len(runs['pictures']) == len(paths)
  for a, b, c in zip(runs['parent'], runs['fused'], runs['pictures']):
    assert a['filters'] == b['filters'] and a['states'] == b['states'] and a['abi_filter_ids'] == b['abi_filter_ids']
    assert np.array_equal(a['params24'], b['params24']) and np.array_equal(a['params24'], c['params24'])
    assert os.path.basename(a['output']) == os.path.basename(b['output'])
    assert open(a['output'], 'rb').read() == open(b['output'], 'rb').read()
    assert c['output'] is None
    assert sorted(a['png']) == sorted(b['png']) == sorted(c['png']) and len(a['png']) == STEPS
    for k in a['png']:
      want = open(a['png'][k], 'rb').read()
      assert open(b['png'][k], 'rb').read() == want, k
      assert open(c['png'][k], 'rb').read() == want, k
  assert sorted(os.listdir(str(tmp_path / 'parent'))) == sorted(os.listdir(str(tmp_path / 'fused')))
  assert not [f for f in os.listdir(str(tmp_path / 'pictures')) if f.endswith('.npy')]
