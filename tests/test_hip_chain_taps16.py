"""GPU: EXPO_TAP_U16, the 16-bit tap format of the fused inference pass (dense, ragged and masked ragged kernels).
Every comparison is bit for bit: a u16 tap is clip(rint(float32(s) * 65535), 0, 65535) of the storage value s that the
truncated sequence writes, y is what the call without taps writes, ragged taps are the dense taps image by image, and
the sentinels around every buffer stay untouched.  Then picture='u16' / intermediates='u16' of retouch / retouch_batch
and the CLI's --tiff16.  uint16 tensors are made, filled and compared through their int16 views.  No input holds a NaN
(the host reference's cast of NaN is undefined)."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate, synthetic, tiff16
from exposure_amd import agent as xagent
from exposure_amd.config import make_cfg
from tests.test_hip_chain_taps import MASKS, fused, guarded, guards_intact, inputs
from tests.test_hip_ragged_chain import NP_DT, ODD, SIZES, carve, make_sequences

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL16 = 0x5A5B


def host_u16(a):
  """the definition of EXPO_TAP_U16 on storage values (a tensor or an array)"""
  if isinstance(a, torch.Tensor):
    a = a.cpu().numpy()
  return np.clip(np.rint(a.astype(np.float32) * np.float32(65535)), 0, 65535).astype(np.uint16)


def u16(t):
  """a uint16 device tensor as a NumPy array"""
  assert t.dtype == torch.uint16
  return t.view(torch.int16).cpu().numpy().view(np.uint16)


def guarded16(shape, dev, off=0):
  """a contiguous uint16 tensor of `shape` inside a buffer with GUARD sentinel elements on both sides, starting `off`
  elements past the guard (the allocation is at least 4-byte aligned: off = 1 puts the tensor at 2 mod 4 bytes)"""
  numel = int(np.prod(shape))
  buf = torch.full((GUARD + off + numel + GUARD,), SENTINEL16, dtype=torch.int16, device=dev)
  t = buf[GUARD + off:GUARD + off + numel].view(*shape).view(torch.uint16)
  assert t.data_ptr() % 4 == 2 * (off % 2)
  return buf, t


def guards16_intact(buf, t):
  start = (t.data_ptr() - buf.data_ptr()) // 2
  head, tail = buf[:start], buf[start + t.numel():]
  return bool((head == SENTINEL16).all()) and bool((tail == SENTINEL16).all()) and head.numel() >= GUARD and \
      tail.numel() >= GUARD


def inputs16(rng, shape, dtype):
  """the pictures of the u8 test (values past 1, below 0, on .5/255 ties) with (k + 0.5)/65535 ties mixed in"""
  x = inputs(rng, shape, torch.float32).numpy().reshape(-1)
  m = len(x[1::17])
  k = (np.arange(m, dtype=np.int64) * 2654435761) % 65536
  x[1::17] = ((k + 0.5) / 65535.0).astype(np.float32)
  x[2::19] = rng.uniform(1.0, 2.5, len(x[2::19]))
  x[4::23] = rng.uniform(-1.5, 0.0, len(x[4::23]))
  return torch.from_numpy(x.reshape(shape).astype(NP_DT[dtype]))


def dense_u16(ids, p, x, mask, with_y=True, off=0):
  """one dense call with u16 taps in guarded buffers -> (y or None, taps); the guards are checked"""
  dev = x.device
  n, h, w, _ = x.shape
  t = bin(mask).count('1')
  ybuf, y = guarded(tuple(x.shape), x.dtype, dev) if with_y else (None, None)
  tbuf, taps = guarded16((t, n, h, w, 3), dev, off) if t else (None, None)
  _cabi.chain_fused_fwd_taps(ids, p, x, y, mask, taps)
  torch.cuda.synchronize()
  if with_y:
    assert guards_intact(ybuf, y), 'y guards'
  if t:
    assert guards16_intact(tbuf, taps), 'tap guards'
  return y, taps


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('steps', [1, 2, 5, 8])
# (32, 48): whole 12-byte vectors, a partial block.  (37, 53) = 1961 pixels: fp16 the element-wise path; fp32 the vector
# path with planes at 2 mod 4 bytes (odd plane size) and a last dword that straddles the plane's end
@pytest.mark.parametrize('hw', [(32, 48), (37, 53)])
def test_dense_taps_bit_for_bit(dtype, steps, hw, gpu_device):
  rng = np.random.default_rng(300 + steps)
  n = 5
  x = inputs16(rng, (n,) + hw + (3,), dtype).to(gpu_device)
  ids_np, p_np = make_sequences(rng, n, steps)  # -1 in the middle (image 4) and at the end (image 2)
  ids, p = torch.from_numpy(ids_np).to(gpu_device), torch.from_numpy(p_np).to(gpu_device)
  y_ref = fused(ids, p, x).view(torch.uint8)
  want = [host_u16(fused(ids[:, :k + 1], p[:, :k + 1], x)) for k in range(steps)]  # once, for every mask below
  for name, mk in MASKS.items():
    mask = mk(steps)
    kept = [k for k in range(steps) if (mask >> k) & 1]
    for with_y in (True, False):
      if not with_y and not mask:
        continue  # nothing to write
      for off in (0, 1):
        y, taps = dense_u16(ids, p, x, mask, with_y, off)
        what = '%s, y %s, offset %d' % (name, with_y, off)
        if with_y:
          assert torch.equal(y.view(torch.uint8), y_ref), what
        for j, k in enumerate(kept):
          np.testing.assert_array_equal(u16(taps[j]), want[k], err_msg='%s: tap %d (step %d)' % (what, j, k))


def _identity_tap(v, dtype, shape, off, dev):
  """the u16 tap of step 0 = Exposure at 0 EV over the values v laid out as `shape`, and the image the call wrote"""
  x = torch.from_numpy(v.reshape(shape)).to(dev)
  assert x.dtype == dtype
  ids = torch.zeros((1, 1), dtype=torch.int32, device=dev)
  p = torch.zeros((1, 1, 24), dtype=torch.float32, device=dev)
  y, taps = dense_u16(ids, p, x, 1, True, off)
  assert torch.equal(y.view(torch.uint8), x.view(torch.uint8))  # x * 2^0: the input's bits
  return u16(taps[0]).reshape(-1)


def test_every_finite_fp16_value(gpu_device):
  bits = np.concatenate([np.arange(0x0000, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)
  assert bits.size == 63488
  for pad, shape in ((4, (1, 2, 10582, 3)), (7, (1, 1, 21165, 3))):  # the vector path / an odd pixel count: element-wise
    v = np.concatenate([bits, np.zeros(pad, dtype=np.uint16)]).view(np.float16)
    assert np.isfinite(v).all() and v.size == int(np.prod(shape))
    for off in (0, 1):  # (a 2-byte aligned plane sends the first shape down the element-wise path too)
      got = _identity_tap(v, torch.float16, shape, off, gpu_device)
      np.testing.assert_array_equal(got, host_u16(v), err_msg='%s offset %d' % (shape, off))
      assert got.min() == 0 and got.max() == 65535


def test_fp32_ties_and_range(gpu_device):
  ties = ((np.arange(65536, dtype=np.float64) + 0.5) / 65535.0).astype(np.float32)
  base = np.concatenate([ties, np.linspace(-2, 3, 4000).astype(np.float32),
                         np.array([0.0, -0.0, 1.0], dtype=np.float32)])
  # 23 180 pixels; with one more the pixel count is odd: a plane one element in sits at 2 mod 4 bytes, every dword of it
  # leaves as two shorts, and an aligned plane's last dword straddles its end
  for pad, shape in ((1, (1, 1, 23180, 3)), (4, (1, 1, 23181, 3)), (1, (1, 20, 1159, 3))):
    v = np.concatenate([base, np.zeros(pad, dtype=np.float32)])
    assert v.size == int(np.prod(shape))
    for off in (0, 1):
      got = _identity_tap(v, torch.float32, shape, off, gpu_device)
      np.testing.assert_array_equal(got, host_u16(v), err_msg='%s offset %d' % (shape, off))
      assert got.min() == 0 and got.max() == 65535
      assert got[:65536].tolist() == host_u16(ties).tolist()


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_ragged_taps_equal_dense_taps(dtype, gpu_device):
  rng = np.random.default_rng(17)
  steps = 5
  xs = carve(SIZES, dtype, gpu_device, odd=ODD)  # incl. a 1-element-offset image and a call over 8 MiB
  for x in xs:
    x.copy_(inputs16(rng, tuple(x.shape), dtype))
  ids_np, p_np = make_sequences(rng, len(SIZES), steps)
  ids, p = torch.from_numpy(ids_np).to(gpu_device), torch.from_numpy(p_np).to(gpu_device)
  for mask in ((1 << steps) - 1, 0b10010):
    t = bin(mask).count('1')
    # the dense taps and outputs of every image, once per mask
    ref = [dense_u16(ids[i:i + 1], p[i:i + 1], x, mask) for i, x in enumerate(xs)]
    ref = [(y.view(torch.uint8).clone(), u16(tp[:, 0])) for y, tp in ref]
    for with_y in (True, False):
      for flip in (0, 1):  # every image's planes at element offsets 0 and 1, both kinds in each launch
        ys = [guarded(tuple(x.shape), dtype, gpu_device) for x in xs] if with_y else None
        taps = [guarded16((t,) + tuple(x.shape[1:]), gpu_device, (i + flip) % 2) for i, x in enumerate(xs)]
        _cabi.chain_fused_fwd_ragged_taps(ids, p, xs, None if ys is None else [y for _, y in ys], mask,
                                          [tp for _, tp in taps])
        torch.cuda.synchronize()
        for i in range(len(xs)):
          what = 'image %d %s, mask %x, y %s, offset %d' % (i, SIZES[i], mask, with_y, (i + flip) % 2)
          np.testing.assert_array_equal(u16(taps[i][1]), ref[i][1], err_msg=what)
          assert guards16_intact(*taps[i]), what
          if with_y:
            assert torch.equal(ys[i][1].view(torch.uint8), ref[i][0]), what
            assert guards_intact(*ys[i]), what


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_masked_ragged_taps(dtype, gpu_device):
  """(96, 128) the vector path; (7, 9) = 63 pixels, odd: element-wise for fp16, for fp32 the straddling last dword (and,
  one element in, planes at 2 mod 4 bytes)"""
  from tests.test_hip_masked_chain import bits, parity_case, run
  ids, p, mp, xs_np, _ = parity_case(5)
  ids, p, mp, xs_np = ids[:2], p[:2], mp[:2], xs_np[:2]
  xs = [torch.from_numpy(x.astype(NP_DT[dtype])).to(gpu_device) for x in xs_np]
  mask = 0b10101
  st = [torch.empty((3,) + tuple(x.shape), dtype=dtype, device=gpu_device) for x in xs]
  ys_ref = run(ids, p, mp, xs, mask, st)  # the same call with storage taps
  want = [host_u16(s) for s in st]
  for out in (True, False):
    for flip in (0, 1):
      taps = [guarded16((3,) + tuple(x.shape), gpu_device, (i + flip) % 2) for i, x in enumerate(xs)]
      ys = run(ids, p, mp, xs, mask, [tp for _, tp in taps], out=out)
      for i in range(2):
        np.testing.assert_array_equal(u16(taps[i][1]), want[i], err_msg='image %d, y %s, offset %d' % (i, out, (i + flip) % 2))
        assert guards16_intact(*taps[i])
        if out:
          assert torch.equal(bits(ys[i]), bits(ys_ref[i]))


def _agent(masking=False, seed=3):
  torch.manual_seed(seed)
  cfg = make_cfg()
  cfg.masking = masking
  return cfg, xagent.Agent(cfg).to('cuda')


def _same(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                   b.contiguous().view(torch.uint8))


@pytest.mark.parametrize('masking', [False, True])
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_retouch_and_retouch_batch_u16(dtype, masking, gpu_device):
  cfg, ag = _agent(masking)
  rng = np.random.default_rng(5)
  sizes = [(96, 128), (65, 33), (128, 96)]
  imgs = [torch.from_numpy(synthetic.make_images(rng, (1, h, w, 3), NP_DT[dtype])).to(gpu_device) for h, w in sizes]
  z = torch.rand((3, cfg.z_dim), device=gpu_device)
  g = torch.Generator(device=gpu_device).manual_seed(8)
  drop = [[(torch.rand(3, 4096, device=gpu_device, generator=g) < 0.5).float() for _ in range(2)]
          for _ in range(cfg.test_steps)]
  kw = dict(z=z, dropout_masks=drop, masks='fused')
  ref = evaluate.retouch_batch(ag, imgs, **kw)
  st = evaluate.retouch_batch(ag, imgs, intermediates='storage', **kw)
  pic = evaluate.retouch_batch(ag, imgs, picture='u16', **kw)
  inter = evaluate.retouch_batch(ag, imgs, intermediates='u16', **kw)
  both = evaluate.retouch_batch(ag, imgs, picture='u16', intermediates='u16', **kw)
  mixed = evaluate.retouch_batch(ag, imgs, picture='u16', intermediates='storage', **kw)
  for r in (st, pic, inter, both, mixed):
    assert all(_same(u, v) for u, v in zip(r[0], ref[0])) and _same(r[1], ref[1]) and _same(r[2], ref[2])
  for r in (pic, both, mixed):
    for t, o in zip(r[-1], ref[0]):
      assert t.dtype == torch.uint16 and t.shape == o.shape[1:]
      np.testing.assert_array_equal(u16(t), host_u16(o[0]))
      np.testing.assert_array_equal(u16(t), u16(evaluate.encode_u16(o[0])))
  for r in (inter, both):
    for t, s in zip(r[3], st[3]):
      assert t.dtype == torch.uint16 and t.shape == s.shape and t.shape[0] == cfg.test_steps - 1
      np.testing.assert_array_equal(u16(t), host_u16(s))
  assert all(_same(u, v) for u, v in zip(mixed[3], st[3]))
  with pytest.raises(ValueError):
    evaluate.retouch_batch(ag, imgs, picture='u16', intermediates='u8', **kw)
  with pytest.raises(ValueError):
    evaluate.retouch_batch(ag, imgs, picture='u8', intermediates='u16', **kw)
  # retouch on a same-size stack
  hi = torch.cat([imgs[0], imgs[0].flip(1)])
  kw = dict(z=z[:2], dropout_masks=[[m[:2] for m in s] for s in drop], masks='fused')
  ref = evaluate.retouch(ag, hi, **kw)
  st = evaluate.retouch(ag, hi, intermediates='storage', **kw)
  both = evaluate.retouch(ag, hi, picture='u16', intermediates='u16', **kw)
  pic = evaluate.retouch(ag, hi, picture='u16', **kw)
  inter = evaluate.retouch(ag, hi, intermediates='u16', **kw)
  for r in (st, both, pic, inter):
    assert all(_same(u, v) for u, v in zip(r[:3], ref))
  for r in (both, pic):
    assert r[-1].shape == hi.shape
    np.testing.assert_array_equal(u16(r[-1]), host_u16(ref[0]))
    np.testing.assert_array_equal(u16(r[-1]), u16(evaluate.encode_u16(ref[0])))
  for r in (both, inter):
    assert r[3].shape == (cfg.test_steps - 1,) + tuple(hi.shape)
    np.testing.assert_array_equal(u16(r[3]), host_u16(st[3]))
  with pytest.raises(ValueError):
    evaluate.retouch(ag, hi, picture=True, intermediates='u16', **kw)


def _write_tiffs(tmp_path, sizes):
  rng = np.random.default_rng(12)
  paths = []
  for i, (h, w) in enumerate(sizes):
    pth = str(tmp_path / ('in%d.tif' % i))
    tiff16.write_tiff(pth, (rng.random((h, w, 3))**1.5 * 60000).astype(np.uint16))
    paths.append(pth)
  return paths


@pytest.mark.parametrize('mode', [['--dtype', 'f16', '--batch', '3'], ['--dtype', 'f32', '--batch', '3'],
                                  ['--dtype', 'f16', '--batch', '3', '--masking', '--fused-masks', '--device-decode',
                                   '--device-proxy'],
                                  ['--dtype', 'f32', '--batch', '1', '--device-decode'], ['--dtype', 'f16', '--stepwise']])
def test_cli_tiff16(tmp_path, mode, gpu_device):
  sizes = [(40, 64), (37, 21), (64, 64)]
  paths = _write_tiffs(tmp_path, sizes)
  out = str(tmp_path / 'o') + os.sep
  recs = evaluate.main(['--seed', '4', '--tiff16', '--step-by-step', '--out', out, *mode, *paths])
  keys = ['intermediate%02d' % k for k in range(4)]
  for rec, (h, w) in zip(recs, sizes):
    assert rec['png'] == {} and sorted(rec['tiff']) == sorted(['retouched'] + keys)
    for f in rec['tiff'].values():
      a = tiff16.read_tiff(f)
      assert a.dtype == np.uint16 and a.shape == (h, w, 3), f
    # the last tap rounds to the storage dtype exactly as y does: the file is the encoding of the .npy output
    result = np.load(rec['output'])
    stored = result.astype(np.float16) if 'f16' in mode else result
    np.testing.assert_array_equal(tiff16.read_tiff(rec['tiff']['retouched']), host_u16(stored), err_msg=rec['image'])
  if '--stepwise' not in mode and '--masking' not in mode:  # the intermediates are the record's truncated sequences
    dt = torch.float16 if 'f16' in mode else torch.float32
    for rec, pth in zip(recs, paths):
      x = torch.from_numpy(np.ascontiguousarray(evaluate.load_image(pth))).to(gpu_device).to(dt)[None]
      ids = torch.tensor([rec['abi_filter_ids']], dtype=torch.int32, device=gpu_device)
      prm = torch.from_numpy(rec['params24'])[None].float().to(gpu_device)
      for k in range(4):
        np.testing.assert_array_equal(tiff16.read_tiff(rec['tiff'][keys[k]]),
                                      host_u16(fused(ids[:, :k + 1], prm[:, :k + 1], x))[0], err_msg=keys[k])
  names = os.listdir(out)
  assert not [f for f in names if f.endswith('.png')] and len([f for f in names if f.endswith('.tif')]) == 15


@pytest.mark.parametrize('flags', [['--png'], ['--device-png'], ['--score', 'targets']])
def test_cli_tiff16_rejects_the_8_bit_outputs(tmp_path, flags, gpu_device):
  paths = _write_tiffs(tmp_path, [(8, 8)])
  with pytest.raises(SystemExit) as e:
    evaluate.main(['--tiff16', *flags, *paths])
  assert e.value.code == 2 and os.listdir(str(tmp_path)) == ['in0.tif']
