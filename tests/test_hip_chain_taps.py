"""GPU: the tap kernels (expo_chain_fused_fwd_taps / _ragged_taps) -- the image after chosen steps of the fused
inference pass.  y is bit-identical to expo_chain_fused_fwd, storage tap k to expo_chain_fused_fwd on ids[:, :k+1],
the u8 tap to save_png's host encoding of the storage tap, ragged taps to dense taps image by image; guard bytes around
every plane stay untouched.  Then retouch / retouch_batch intermediates and the CLI's --step-by-step PNGs."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate, synthetic
from exposure_amd import agent as xagent
from exposure_amd.config import make_cfg
from tests.test_hip_ragged_chain import NP_DT, ODD, SIZES, carve, make_sequences

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = {torch.uint8: 0xA5, torch.float16: 1234.0, torch.float32: -777.0}


def host_u8(t):
  """evaluate.save_png's encoding of the storage values"""
  a = t.float().cpu().numpy()
  return np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8)


def guarded(shape, dtype, dev, off=0):
  """a contiguous tensor of `shape` inside a buffer with GUARD sentinel elements on both sides, starting `off`
  elements past the guard (u8: any byte offset)"""
  numel = int(np.prod(shape))
  buf = torch.full((GUARD + off + numel + GUARD,), SENTINEL[dtype], dtype=dtype, device=dev)
  return buf, buf[GUARD + off:GUARD + off + numel].view(*shape)


def guards_intact(buf, t):
  s = SENTINEL[buf.dtype]
  start = (t.data_ptr() - buf.data_ptr()) // buf.element_size()
  head, tail = buf[:start], buf[start + t.numel():]
  return bool((head == s).all()) and bool((tail == s).all()) and head.numel() >= GUARD and tail.numel() >= GUARD


def fused(ids, params, x):
  y = torch.empty_like(x)
  _cabi.chain_fused_fwd(ids.contiguous(), params.contiguous(), x, y)
  return y


MASKS = {'none': lambda s: 0, 'first': lambda s: 1, 'last': lambda s: 1 << (s - 1), 'all': lambda s: (1 << s) - 1,
         'alternate': lambda s: sum(1 << k for k in range(0, s, 2))}


def inputs(rng, shape, dtype):
  """synthetic pictures with values past 1, below 0 and on .5/255 ties mixed in"""
  x = synthetic.make_images(rng, shape, np.float32).reshape(-1)
  m = x.size
  x[0:m:7] = ((np.arange(len(x[0:m:7])) % 256) + 0.5) / 255.0
  x[3:m:11] = rng.uniform(1.0, 1.8, len(x[3:m:11]))
  x[5:m:13] = rng.uniform(-0.4, 0.0, len(x[5:m:13]))
  return torch.from_numpy(x.reshape(shape).astype(NP_DT[dtype]))


def check_dense(ids, p, x, mask, fmt_dtype, with_y, off):
  dev = x.device
  n, h, w, _ = x.shape
  steps = ids.shape[1]
  t = bin(mask).count('1')
  ybuf, y = guarded(tuple(x.shape), x.dtype, dev) if with_y else (None, None)
  tbuf, taps = guarded((t, n, h, w, 3), fmt_dtype, dev, off) if t else (None, None)
  _cabi.chain_fused_fwd_taps(ids, p, x, y, mask, taps)
  if with_y:
    assert torch.equal(y.view(torch.uint8), fused(ids, p, x).view(torch.uint8)), 'y'
    assert guards_intact(ybuf, y)
  if t:
    assert guards_intact(tbuf, taps)
  j = 0
  for k in range(steps):
    if (mask >> k) & 1:
      ref = fused(ids[:, :k + 1], p[:, :k + 1], x)
      if fmt_dtype == torch.uint8:
        np.testing.assert_array_equal(taps[j].cpu().numpy(), host_u8(ref), err_msg='u8 tap %d (step %d)' % (j, k))
      else:
        assert torch.equal(taps[j].view(torch.uint8), ref.view(torch.uint8)), 'storage tap %d (step %d)' % (j, k)
      j += 1
  return y, taps


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('steps', [1, 2, 5, 8])
@pytest.mark.parametrize('hw', [(32, 48), (37, 53)])  # fp16: the dwordx3 path / an odd pixel count (element-wise)
def test_dense_taps_bit_for_bit(dtype, steps, hw, gpu_device):
  rng = np.random.default_rng(100 + steps)
  n = 5
  x = inputs(rng, (n,) + hw + (3,), dtype).to(gpu_device)
  ids_np, p_np = make_sequences(rng, n, steps)  # -1 in the middle (image 4) and at the end (image 2)
  ids, p = torch.from_numpy(ids_np).to(gpu_device), torch.from_numpy(p_np).to(gpu_device)
  for name, mk in MASKS.items():
    mask = mk(steps)
    for fmt in (torch.uint8, dtype):
      offs = range(4) if (fmt == torch.uint8 and name == 'all') else [1 if fmt == torch.uint8 else 0]
      for off in offs:
        check_dense(ids, p, x, mask, fmt, True, off)
        if mask:
          check_dense(ids, p, x, mask, fmt, False, off)  # y NULL: taps only


def test_exposure_ties_and_range(gpu_device):
  """Step 0 = Exposure at 0 EV keeps the inputs: the u8 tap of values on .5/255 ties, past 1 and below 0."""
  for dtype in (torch.float32, torch.float16):
    v = np.concatenate([(np.arange(256) + 0.5) / 255.0, np.linspace(-2, 3, 510), [1.0, 0.0]]).astype(np.float32)
    x = torch.from_numpy(v.reshape(1, 16, 16, 3).astype(NP_DT[dtype])).to(gpu_device)
    ids = torch.zeros((1, 2), dtype=torch.int32, device=gpu_device)
    p = torch.zeros((1, 2, 24), dtype=torch.float32, device=gpu_device)
    p[0, 1, 0] = 0.7
    _, taps = check_dense(ids, p, x, 3, torch.uint8, True, 2)
    a = taps[0].cpu().numpy().reshape(-1)
    assert a[:256].tolist() == host_u8(x).reshape(-1)[:256].tolist()
    assert a.min() == 0 and a.max() == 255


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('fmt', ['u8', 'storage'])
def test_ragged_taps_equal_dense_taps(dtype, fmt, gpu_device):
  rng = np.random.default_rng(7)
  steps = 5
  xs = carve(SIZES, dtype, gpu_device, odd=ODD)  # incl. a 1-element-offset image and a call over 8 MiB
  for x in xs:
    x.copy_(inputs(rng, tuple(x.shape), dtype))
  ids_np, p_np = make_sequences(rng, len(SIZES), steps)
  ids, p = torch.from_numpy(ids_np).to(gpu_device), torch.from_numpy(p_np).to(gpu_device)
  tdt = torch.uint8 if fmt == 'u8' else dtype
  for mask in (1, 1 << (steps - 1), (1 << steps) - 1, 0b10101):
    t = bin(mask).count('1')
    for with_y in (True, False):
      ys = [guarded(tuple(x.shape), dtype, gpu_device) for x in xs] if with_y else None
      # u8 planes starting at every byte offset 0-3; a storage buffer one element in for the odd image
      taps = [guarded((t,) + tuple(x.shape[1:]), tdt, gpu_device, (i % 4) if fmt == 'u8' else int(i == ODD))
              for i, x in enumerate(xs)]
      _cabi.chain_fused_fwd_ragged_taps(ids, p, xs, None if ys is None else [y for _, y in ys], mask,
                                        [tp for _, tp in taps])
      for i, x in enumerate(xs):
        y_ref, t_ref = check_dense(ids[i:i + 1], p[i:i + 1], x, mask, tdt, True, 0)
        assert torch.equal(taps[i][1].view(torch.uint8), t_ref[:, 0].reshape(taps[i][1].shape).view(torch.uint8)), i
        assert guards_intact(*taps[i])
        if with_y:
          assert torch.equal(ys[i][1].view(torch.uint8), y_ref.view(torch.uint8)), i
          assert guards_intact(*ys[i])


def test_ragged_taps_over_64_images(gpu_device):
  rng = np.random.default_rng(9)
  n, steps = 70, 3
  sizes = [(1 + i % 7, 2 + i % 5) for i in range(n)]
  xs = carve(sizes, torch.float16, gpu_device, odd=66)
  for x in xs:
    x.copy_(inputs(rng, tuple(x.shape), torch.float16))
  ids_np, p_np = make_sequences(rng, n, steps)
  ids, p = torch.from_numpy(ids_np).to(gpu_device), torch.from_numpy(p_np).to(gpu_device)
  taps = [guarded((2,) + tuple(x.shape[1:]), torch.uint8, gpu_device, i % 4) for i, x in enumerate(xs)]
  _cabi.chain_fused_fwd_ragged_taps(ids, p, xs, None, 0b101, [tp for _, tp in taps])
  for i, x in enumerate(xs):
    for j, k in enumerate((0, 2)):
      ref = fused(ids[i:i + 1, :k + 1], p[i:i + 1, :k + 1], x)
      np.testing.assert_array_equal(taps[i][1][j].cpu().numpy(), host_u8(ref)[0], err_msg='image %d tap %d' % (i, j))
    assert guards_intact(*taps[i])


def _agent(seed=3):
  torch.manual_seed(seed)
  cfg = make_cfg()
  return cfg, xagent.Agent(cfg).to('cuda')


def test_retouch_and_retouch_batch_intermediates(gpu_device):
  cfg, ag = _agent()
  rng = np.random.default_rng(5)
  sizes = [(96, 128), (65, 33), (128, 96)]
  imgs = [torch.from_numpy(synthetic.make_images(rng, (1, h, w, 3), np.float16)).to(gpu_device) for h, w in sizes]
  z = torch.rand((3, cfg.z_dim), device=gpu_device)
  outs, _, _, ops, inter = evaluate.retouch_batch(ag, imgs, z=z, return_trace='full', intermediates='u8')
  _, _, _, ops2, st = evaluate.retouch_batch(ag, imgs, z=z, return_trace='full', intermediates='storage')
  for i, im in enumerate(imgs):
    ids, prm = ops['abi_filter_ids'][i:i + 1].int(), ops['params24'][i:i + 1].float()
    assert inter[i].shape == (cfg.test_steps - 1,) + tuple(im.shape[1:]) and inter[i].dtype == torch.uint8
    assert torch.equal(outs[i], fused(ids, prm, im))
    for k in range(cfg.test_steps - 1):
      np.testing.assert_array_equal(inter[i][k].cpu().numpy(), host_u8(fused(ids[:, :k + 1], prm[:, :k + 1], im))[0])
    ids2, prm2 = ops2['abi_filter_ids'][i:i + 1].int(), ops2['params24'][i:i + 1].float()
    for k in range(cfg.test_steps - 1):
      assert torch.equal(st[i][k], fused(ids2[:, :k + 1], prm2[:, :k + 1], im)[0])
  hi = torch.cat([imgs[0], imgs[0]])
  out, _, _, ops, inter = evaluate.retouch(ag, hi, z=z[:2], return_trace='full', intermediates='u8')
  assert inter.shape == (cfg.test_steps - 1, 2, 96, 128, 3)
  ids, prm = ops['abi_filter_ids'].int(), ops['params24'].float()
  for k in range(cfg.test_steps - 1):
    np.testing.assert_array_equal(inter[k].cpu().numpy(), host_u8(fused(ids[:, :k + 1], prm[:, :k + 1], hi)))


@pytest.mark.parametrize('mode', [['--batch', '3'], ['--batch', '1'], ['--stepwise']])
def test_cli_step_by_step_pngs(tmp_path, mode, gpu_device):
  from PIL import Image
  rng = np.random.default_rng(12)
  paths = []
  for i, (h, w) in enumerate([(40, 64), (37, 21), (64, 64)]):
    pth = str(tmp_path / ('in%d.png' % i))
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'RGB').save(pth)
    paths.append(pth)
  out = str(tmp_path / 'o') + os.sep
  recs = evaluate.main(['--seed', '4', '--step-by-step', '--out', out, *mode, *paths])
  for rec, pth in zip(recs, paths):
    x = torch.from_numpy(np.ascontiguousarray(evaluate.load_image(pth))).to(gpu_device).to(torch.float16)[None]
    ids = torch.tensor([rec['abi_filter_ids']], dtype=torch.int32, device=gpu_device)
    prm = torch.from_numpy(rec['params24'])[None].float().to(gpu_device)
    keys = sorted(k for k in rec['png'] if k.startswith('intermediate'))
    assert keys == ['intermediate%02d' % k for k in range(4)]
    for k in range(4):
      got = np.asarray(Image.open(rec['png']['intermediate%02d' % k]))
      want = host_u8(fused(ids[:, :k + 1], prm[:, :k + 1], x))[0]
      if mode == ['--stepwise']:  # fp16 between steps (the reference's schedule): close to the one-pass chain
        assert got.shape == want.shape and np.abs(got.astype(int) - want.astype(int)).mean() < 0.5, k
      else:
        np.testing.assert_array_equal(got, want, err_msg=rec['png']['intermediate%02d' % k])
