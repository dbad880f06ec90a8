"""GPU: expo_chain_fused_curves_fwd_ragged -- the fused inference pass for any cfg.curve_steps L -- against
oracle/filters_np.py::process_packed applied step by step in float64 with no rounding between steps (a -1 step makes
the image zero), every step's storage tap and the output within tests/_tol.py::assert_image_close of the storage dtype.
Parameters come from the oracle's regressors on seeded features (cfg.curve_steps = L); the entries of a 48-wide row its
filter does not use are 1e30.  The inputs hold negatives, values above 1 and the knots j / L.  Then the bit identities
(no curve step: expo_chain_fused_fwd_ragged's bits; batch invariance; split launches; the taps), the streaming
instantiations, and retouch / retouch_batch / the CLIs end to end.

Measured on the MI355X (worst err / tol over the five images, every step's tap and the output; the bound is
tests/_tol.py's, unchanged): see DESIGN.md §3.25."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate, synthetic
from exposure_amd import agent as xagent
from exposure_amd.config import make_cfg
from oracle import filters_np as fnp
from tests._tol import assert_image_close, image_tol

pytestmark = pytest.mark.gpu

NP_DT = {torch.float16: np.float16, torch.float32: np.float32}
W48 = _cabi.EXPO_MAX_PARAMS_CURVES
UNUSED = np.float32(1e30)
# (96,128): the vector path, several waves; (7,9): an odd pixel count, element-wise for fp16; (17,23) / (40,24): H < W and
# H > W; (33,100): more than one block
SIZES = [(96, 128), (7, 9), (17, 23), (40, 24), (33, 100)]
# per image: all of 0..7 | Level and Tone, Color, Tone back to back | -1 at the start | -1 in the middle | (-1 at the
# end: written into the last step of the truncated row below)
SEQUENCES = np.array([[0, 1, 2, 3, 4, 5, 6, 7],
                      [8, 4, 7, 4, 0, 5, 3, 6],
                      [-1, 2, 4, 7, 4, 1, 8, 5],
                      [1, 6, 3, -1, 4, 7, 4, 0],
                      [5, 8, 2, 4, 7, 4, 1, 3]], dtype=np.int32)
LS = [1, 3, 8, 12, 16]


def row_len(fid, L):
  return L if fid == 4 else 3 * L if fid == 7 else fnp.NUM_PARAMS[fid]


def make_rows(rng, ids, L, width=W48):
  """(n, S, width) float32 rows: the oracle's regressors on standard-normal features; unused entries 1e30"""
  cfg = dict(fnp.DEFAULT_CFG, curve_steps=L)
  n, steps = ids.shape
  p = np.full((n, steps, width), UNUSED, dtype=np.float32)
  for i in range(n):
    for k in range(steps):
      fid = int(ids[i, k])
      if fid >= 0:
        m = row_len(fid, L)
        p[i, k, :m] = fnp.regress_packed(fid, rng.standard_normal((1, m)), cfg)[0]
  return p


def make_input(rng, h, w, L):
  """fp16 values in about [-0.03, 1.3] with the knots j / L (and 0, 1, values just outside) written over the first
  pixels"""
  x = synthetic.make_images(rng, (h, w, 3), np.float32) * np.float32(1.3) - np.float32(0.03)
  flat = x.reshape(-1)
  special = [j / L for j in range(L + 1)] + [-0.25, 1.5, 0.0, 1.0]
  flat[:len(special)] = np.asarray(special, dtype=np.float32)[:flat.size]
  x = x.astype(np.float16)
  assert (x < 0).any() and (x > 1).any()
  return x


def oracle_steps(x, ids, p, L):
  """the float64 image after every step of one image's sequence: x (H, W, 3), ids (S,), p (S, 48)"""
  cur = np.asarray(x, dtype=np.float64)[None]
  out = []
  for k in range(len(ids)):
    fid = int(ids[k])
    if fid < 0:
      cur = np.zeros_like(cur)
    else:
      cur = fnp.process_packed(fid, cur, p[k:k + 1, :row_len(fid, L)].astype(np.float64))
    out.append(cur[0])
  return out


def dev_rows(ids, p, dev):
  return (torch.from_numpy(np.ascontiguousarray(ids)).to(dev), torch.from_numpy(np.ascontiguousarray(p)).to(dev))


def run(ids, p, L, xs, tap_mask=0, taps=None, out=True):
  dev = xs[0].device
  ys = [torch.empty_like(x) for x in xs] if out else None
  _cabi.chain_fused_curves_fwd_ragged(*dev_rows(ids, p, dev), L, xs, ys, tap_mask, taps)
  torch.cuda.synchronize()
  return ys


def bits(t):
  return t.contiguous().view(torch.uint8)


def to_dev(xs_np, dtype, dev):
  return [torch.from_numpy(x.astype(NP_DT[dtype])).to(dev) for x in xs_np]


_CASES = {}


def parity_case(L, steps):
  """inputs and the float64 reference of the parity tests, made once per (L, steps) and shared by both dtypes: the
  images are fp16 values, which the fp32 runs take as they are"""
  if (L, steps) not in _CASES:
    rng = np.random.default_rng(1000 * L + steps)
    ids = SEQUENCES[:, :steps].copy()
    ids[4, steps - 1] = -1
    p = make_rows(rng, ids, L)
    xs = [make_input(rng, h, w, L) for h, w in SIZES]
    refs = [oracle_steps(x, ids[i], p[i], L) for i, x in enumerate(xs)]
    _CASES[(L, steps)] = (ids, p, xs, refs)
  return _CASES[(L, steps)]


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('steps', [8, 5, 1])
@pytest.mark.parametrize('L', LS)
def test_every_step_matches_the_float64_oracle(L, steps, dtype, gpu_device):
  ids, p, xs_np, refs = parity_case(L, steps)
  xs = to_dev(xs_np, dtype, gpu_device)
  taps = [torch.empty((steps,) + tuple(x.shape), dtype=dtype, device=gpu_device) for x in xs]
  ys = run(ids, p, L, xs, (1 << steps) - 1, taps)
  got = [[t[k].float().cpu().numpy() for k in range(steps)] + [y.float().cpu().numpy()] for t, y in zip(taps, ys)]
  worst = max(float((np.abs(g - r) / image_tol(r, NP_DT[dtype])).max())
              for gs, ref in zip(got, refs) for g, r in zip(gs, ref + [ref[-1]]))
  print('curves chain L=%d %s, %d steps: worst err / tol = %.3f' % (L, dtype, steps, worst))
  for i, (gs, ref) in enumerate(zip(got, refs)):
    for k, (g, r) in enumerate(zip(gs, ref + [ref[-1]])):
      assert_image_close(g, r, NP_DT[dtype], 'L %d image %d %s after step %d' % (L, i, SIZES[i], min(k, steps - 1)))
  assert not bits(ys[4]).any()  # after a trailing -1: exactly +0
  assert ids[2, 0] == -1 and (steps < 4 or ids[3, 3] == -1)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_tone_with_one_knot_is_the_clamp(dtype, gpu_device):
  rng = np.random.default_rng(3)
  ids = np.full((2, 1), 4, dtype=np.int32)
  p = make_rows(rng, ids, 1)
  xs_np = [make_input(rng, h, w, 1) for h, w in SIZES[:2]]
  ys = run(ids, p, 1, to_dev(xs_np, dtype, gpu_device))
  for x, y in zip(xs_np, ys):
    assert_image_close(y.float().cpu().numpy(), np.clip(x.astype(np.float64), 0.0, 1.0), NP_DT[dtype], 'L = 1')


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('L', [3, 16])
def test_without_a_curve_step_the_bits_are_the_8_step_passes(L, dtype, gpu_device):
  """the filter bodies are the same inline functions under the same flags"""
  rng = np.random.default_rng(17)
  ids = np.array([[0, 1, 2, 3, 5, 6, 8], [8, 6, 5, -1, 3, 2, 1], [3, 3, 0, 8, 6, 2, 5], [1, 5, 8, 0, 2, 6, 3],
                  [2, 0, 6, 5, 1, 8, -1]], dtype=np.int32)
  p48 = make_rows(rng, ids, L)
  p24 = np.ascontiguousarray(p48[:, :, :_cabi.EXPO_MAX_PARAMS])
  xs = to_dev([make_input(rng, h, w, L) for h, w in SIZES], dtype, gpu_device)
  ys = run(ids, p48, L, xs)
  ref = [torch.empty_like(x) for x in xs]
  _cabi.chain_fused_fwd_ragged(*dev_rows(ids, p24, gpu_device), xs, ref)
  torch.cuda.synchronize()
  for i, (y, r) in enumerate(zip(ys, ref)):
    assert torch.equal(bits(y), bits(r)), i


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_every_image_is_the_image_alone_and_no_step_is_the_input(dtype, gpu_device):
  L = 12
  ids, p, xs_np, _ = parity_case(L, 8)
  xs = to_dev(xs_np, dtype, gpu_device)
  ys = run(ids, p, L, xs)
  for i, x in enumerate(xs):
    alone, = run(ids[i:i + 1], p[i:i + 1], L, [x])
    assert torch.equal(bits(ys[i]), bits(alone)), i
  same = run(ids[:, :0], p[:, :0], L, xs)
  for x, y in zip(xs, same):
    assert torch.equal(bits(y), bits(x))  # steps == 0: the input's bits


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_more_than_64_images_split_into_launches(dtype, gpu_device):
  """65 images: the second launch's rows of ids and params start at image 64"""
  rng = np.random.default_rng(41)
  n, steps, L = 65, 3, 5
  sizes = [(5 + i % 5, 7 + (i // 5) % 5) for i in range(n)]
  ids = rng.integers(0, 9, (n, steps)).astype(np.int32)
  ids[64] = (4, 7, 4)
  p = make_rows(rng, ids, L)
  xs_np = [make_input(rng, h, w, L) for h, w in sizes]
  xs = to_dev(xs_np, dtype, gpu_device)
  ys = run(ids, p, L, xs)
  for i in range(n):
    ref = oracle_steps(xs_np[i], ids[i], p[i], L)[-1]
    assert_image_close(ys[i].float().cpu().numpy(), ref, NP_DT[dtype], 'image %d %s' % (i, sizes[i]))
  for i in (0, 63, 64):
    alone, = run(ids[i:i + 1], p[i:i + 1], L, [xs[i]])
    assert torch.equal(bits(ys[i]), bits(alone)), i


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_taps(dtype, gpu_device):
  """(96,128) the vector path, (7,9) element-wise for fp16; image 1's u8 planes start at an odd byte address, its u16
  planes at 2 mod 4"""
  L = 12
  ids, p, xs_np, _ = parity_case(L, 5)
  ids, p, xs_np = ids[:2], p[:2], xs_np[:2]
  dev = gpu_device
  xs = to_dev(xs_np, dtype, dev)
  steps = ids.shape[1]
  mask = 0b10101
  kept = [k for k in range(steps) if (mask >> k) & 1]
  truncated = {k: run(ids[:, :k + 1], p[:, :k + 1], L, xs) for k in kept}
  full = run(ids, p, L, xs)
  st = [torch.empty((len(kept),) + tuple(x.shape), dtype=dtype, device=dev) for x in xs]
  ys = run(ids, p, L, xs, mask, st)
  bufs = [torch.full((1 + len(kept) * x.numel() + 64,), 0xA5, dtype=torch.uint8, device=dev) for x in xs]
  u8 = [b[off:off + len(kept) * x.numel()].view((len(kept),) + tuple(x.shape)) for b, x, off in zip(bufs, xs, (0, 1))]
  assert u8[1].data_ptr() % 2 == 1
  assert run(ids, p, L, xs, mask, u8, out=False) is None  # ys=None: the taps only
  # (uint16 tensors are made and filled through their int16 views)
  bufs16 = [torch.full((1 + len(kept) * x.numel() + 32,), 0x2525, dtype=torch.int16, device=dev) for x in xs]
  u16 = [b[off:off + len(kept) * x.numel()].view((len(kept),) + tuple(x.shape)).view(torch.uint16)
         for b, x, off in zip(bufs16, xs, (0, 1))]
  assert u16[1].data_ptr() % 4 == 2
  y16 = run(ids, p, L, xs, mask, u16)
  st_only = [torch.empty_like(t) for t in st]
  run(ids, p, L, xs, mask, st_only, out=False)
  for i in range(2):
    assert torch.equal(bits(ys[i]), bits(full[i])) and torch.equal(bits(y16[i]), bits(full[i]))  # taps do not change y
    for j, k in enumerate(kept):
      assert torch.equal(bits(st[i][j]), bits(truncated[k][i])), (i, k)  # what the truncated sequence writes
      assert torch.equal(bits(st_only[i][j]), bits(st[i][j])), (i, k)
      assert torch.equal(u8[i][j], evaluate.encode_u8(st[i][j])), (i, k)
      assert torch.equal(bits(u16[i][j]), bits(evaluate.encode_u16(st[i][j]))), (i, k)
    assert torch.equal(bits(st[i][-1]), bits(ys[i]))  # the tap of the last step is y
    tail = bufs[i][(0, 1)[i] + u8[i].numel():]
    assert bool((tail == 0xA5).all()) and (i == 0 or int(bufs[i][0]) == 0xA5)  # nothing written around the planes
    tail16 = bufs16[i][(0, 1)[i] + u16[i].numel():]
    assert bool((tail16 == 0x2525).all()) and (i == 0 or int(bufs16[i][0]) == 0x2525)


@pytest.mark.parametrize('dtype,side', [(torch.float16, 1200), (torch.float32, 840)])
def test_streaming_instantiations_every_pixel(dtype, side, gpu_device):
  """one call of at least 8 MiB (stream_min_bytes): the large image on the vector path, 7x9 beside it (element-wise for
  fp16); L = 12, 5 steps with Tone and Color"""
  L = 12
  rng = np.random.default_rng(77)
  sizes = [(side, side), (7, 9)]
  assert sum(h * w for h, w in sizes) * 3 * (2 if dtype == torch.float16 else 4) >= 8 << 20
  ids = np.array([[1, 4, 7, 5, 4], [7, 4, 0, 7, 8]], dtype=np.int32)
  p = make_rows(rng, ids, L)
  xs_np = [make_input(rng, h, w, L) for h, w in sizes]
  ys = run(ids, p, L, to_dev(xs_np, dtype, gpu_device))
  for i, x in enumerate(xs_np):
    ref = oracle_steps(x, ids[i], p[i], L)[-1]
    assert_image_close(ys[i].float().cpu().numpy(), ref, NP_DT[dtype], '%s %s' % (dtype, sizes[i]))


@pytest.mark.parametrize('L', [4, 16])
def test_retouch_and_retouch_batch_fused_curves_end_to_end(L, gpu_device):
  """The agent sees only the proxies either way: the same selected filters as the default (stepwise) call; in fp32 storage
  the two schedules' outputs agree within the bound, and the 'full' trace replays to the same bits."""
  dev = gpu_device
  cfg = make_cfg()
  cfg.curve_steps = L
  torch.manual_seed(5)
  ag = xagent.Agent(cfg).to(dev)
  rng = np.random.default_rng(6)
  sizes = [(96, 128), (57, 41), (64, 200)]
  imgs = [torch.from_numpy(synthetic.make_images(rng, (h, w, 3), np.float32)).to(dev) for h, w in sizes]
  z = torch.rand(3, cfg.z_dim, device=dev)
  masks = [[(torch.rand(3, 4096, device=dev) < 0.5).float() for _ in range(2)] for _ in range(cfg.test_steps)]
  outs, low, states, ops, inter = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full',
                                                         intermediates='storage', curves='fused')
  routs, rlow, rstates, rops, rinter = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full',
                                                              intermediates='storage')
  assert torch.equal(ops['selected'], rops['selected']) and torch.equal(ops['abi_filter_ids'], rops['abi_filter_ids'])
  assert ops['params48'].shape == (3, cfg.test_steps, W48) and 'params48' not in rops
  for i, im in enumerate(imgs):
    assert outs[i].shape == im.shape
    assert_image_close(outs[i].cpu().numpy(), routs[i].double().cpu().numpy(), np.float32, 'image %d' % i)
    assert_image_close(routs[i].cpu().numpy(), outs[i].double().cpu().numpy(), np.float32, 'image %d' % i)
    assert inter[i].shape == rinter[i].shape == (cfg.test_steps - 1,) + tuple(im.shape)
    assert_image_close(inter[i].cpu().numpy(), rinter[i].double().cpu().numpy(), np.float32, 'intermediates %d' % i)
  again, _ = evaluate.fused_curves_chain_ragged(imgs, ops['abi_filter_ids'], ops['params48'], L)
  for a, o in zip(again, outs):
    assert torch.equal(bits(a), bits(o))
  # retouch on a dense tensor: one ragged call over its views
  hi = torch.stack([imgs[0], imgs[0].flip(0)])
  zz = [[m[:2] for m in s] for s in masks]
  out, _, _, dops = evaluate.retouch(ag, hi, z=z[:2], dropout_masks=zz, return_trace='full', curves='fused')
  ref, _, _, dref = evaluate.retouch(ag, hi, z=z[:2], dropout_masks=zz, return_trace='full')
  assert torch.equal(dops['selected'], dref['selected'])
  assert_image_close(out.cpu().numpy(), ref.double().cpu().numpy(), np.float32, 'retouch')
  replay, _ = evaluate.fused_curves_chain(hi, dops['abi_filter_ids'], dops['params48'], L)
  assert torch.equal(bits(replay), bits(out))


def test_cli_round_trip(gpu_device, tmp_path):
  from PIL import Image
  from exposure_amd import train
  weights = str(tmp_path / 'm.pt')
  train.main(['--curve-steps', '4', '--iters', '2', '--no-graphs', '--save', weights])
  rng = np.random.default_rng(11)
  paths = []
  for i, (h, w) in enumerate([(40, 64), (37, 21), (64, 64)]):
    pth = str(tmp_path / ('in%d.png' % i))
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'RGB').save(pth)
    paths.append(pth)
  out = str(tmp_path / 'o') + os.sep
  common = ['--weights', weights, '--fused-curves', '--batch', '3', '--step-by-step', '--device-png', '--out', out]
  recs = evaluate.main(common + ['--curve-steps', '4'] + paths)
  assert len(recs) == 3
  for rec in recs:
    assert os.path.exists(rec['output'])
    assert sorted(rec['png']) == ['intermediate%02d' % k for k in range(4)] + ['retouched']
    assert all(os.path.exists(f) for f in rec['png'].values())
    shape = np.load(rec['output']).shape
    for f in rec['png'].values():
      assert np.asarray(Image.open(f)).shape == shape
  assert len(os.listdir(out)) == 3 * (1 + 1 + 4)
  with pytest.raises(RuntimeError, match='size mismatch'):
    evaluate.main(common + ['--curve-steps', '8'] + paths)
