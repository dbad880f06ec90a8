"""GPU: expo_chain_fused_fwd_ragged (ABI 9) -- the fused inference chain over a list of images of different sizes in
one launch -- against the one-image kernel (bit for bit), against the float64 chain, for bounds and for table
chunking; evaluate.retouch_batch against retouch; the CLI's --batch."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate, synthetic
from exposure_amd import agent as xagent
from exposure_amd.config import make_cfg
from oracle import filters_np as fnp
from tests._tol import assert_image_close

pytestmark = pytest.mark.gpu

NP_DT = {torch.float16: np.float16, torch.float32: np.float32}
# 1x5: an odd fp16 pixel count (element-wise path); index 5 sits at an odd element offset (fp16: a 2-byte aligned
# base, element-wise path); 1000x1400 takes the call past EXPO_STREAM_MIN_BYTES (8 MiB) on its own
SIZES = [(1, 1), (1, 5), (7, 9), (64, 64), (200, 304), (33, 47), (1000, 1400)]
ODD = 5


def carve(sizes, dtype, dev, odd=None, fill=None):
  """One device tensor (1, H, W, 3) per size, each in its own allocation; image `odd` starts one element in."""
  out = []
  for i, (h, w) in enumerate(sizes):
    off = 1 if i == odd else 0
    buf = torch.empty(off + h * w * 3, dtype=dtype, device=dev)
    if fill is not None:
      buf.fill_(fill)
    out.append(buf[off:].view(1, h, w, 3))
  return out


def make_sequences(rng, n, steps):
  """ids covering 0..8 and -1 (in the middle and at the end of a sequence) over the set, and their parameters."""
  ids = np.array([[(i * 3 + st) % 10 - 1 for st in range(steps)] for i in range(n)], dtype=np.int32).reshape(n, steps)
  if steps >= 1:
    ids[2, steps - 1] = -1
  if steps >= 3:
    ids[4, 1] = -1
  p = np.zeros((n, steps, 24), dtype=np.float32)
  for i in range(n):
    for st in range(steps):
      fid = int(ids[i, st])
      if fid >= 0:
        p[i, st, :fnp.NUM_PARAMS[fid]] = synthetic.make_params(rng, fid, 1)[0]
  return ids, p


def dense(ids, params, xs):
  """the one-image kernel, image by image"""
  ys = []
  for i, x in enumerate(xs):
    y = torch.empty_like(x)
    _cabi.chain_fused_fwd(ids[i:i + 1].contiguous(), params[i:i + 1].contiguous(), x, y)
    ys.append(y)
  return ys


def ragged_case(dtype, steps, dev, seed, with_inf):
  rng = np.random.default_rng(seed)
  xs = carve(SIZES, dtype, dev, odd=ODD)
  for x in xs:
    x.copy_(torch.from_numpy(synthetic.make_images(rng, tuple(x.shape), NP_DT[dtype])))
  if with_inf:
    xs[3][0, 5, 7, :] = float('inf')
  ids, p = make_sequences(rng, len(SIZES), steps)
  return xs, torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev), ids, p


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('steps', [0, 1, 5, 8])
def test_ragged_equals_the_one_image_kernel_bit_for_bit(dtype, steps, gpu_device):
  xs, ids, p, _, _ = ragged_case(dtype, steps, gpu_device, 11 + steps, with_inf=True)
  ys = carve(SIZES, dtype, gpu_device, odd=ODD)
  if dtype == torch.float16:
    assert xs[ODD].data_ptr() % 4 == 2 and ys[ODD].data_ptr() % 4 == 2
  _cabi.chain_fused_fwd_ragged(ids, p, xs, ys)
  ref = dense(ids, p, xs)
  for i, (y, r) in enumerate(zip(ys, ref)):
    assert torch.equal(y.view(torch.int16 if dtype == torch.float16 else torch.int32),
                       r.view(torch.int16 if dtype == torch.float16 else torch.int32)), (i, SIZES[i])
  if steps >= 1:  # image 2 ends on -1: exactly +0
    assert float(ys[2].abs().max()) == 0.0 and not bool(torch.signbit(ys[2]).any())


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('steps', [0, 1, 5, 8])
def test_ragged_matches_the_float64_chain(dtype, steps, gpu_device):
  xs, ids_t, p_t, ids, p = ragged_case(dtype, steps, gpu_device, 23 + steps, with_inf=False)
  outs = evaluate.fused_chain_ragged(xs, ids_t, p_t)
  for i, (x, y) in enumerate(zip(xs, outs)):
    assert y.shape == x.shape
    ref = x.double().cpu().numpy()
    for st in range(steps):
      fid = int(ids[i, st])
      ref = np.zeros_like(ref) if fid < 0 else fnp.process_packed(fid, ref, p[i:i + 1, st, :fnp.NUM_PARAMS[fid]].astype(
          np.float64))
    if dtype == torch.float16:
      np.clip(ref, -65504.0, 65504.0, out=ref)
    assert_image_close(y.double().cpu().numpy(), ref, NP_DT[dtype], 'ragged image %d %s' % (i, SIZES[i]))


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_ragged_writes_nothing_outside_its_images(dtype, gpu_device):
  """All outputs carved from ONE flat buffer with sentinel gaps between them (odd gaps: fp16 images at 2-byte aligned
  bases, odd pixel counts); after the call every gap element still holds the sentinel, and the images are right."""
  dev = gpu_device
  rng = np.random.default_rng(5)
  sizes = [(1, 1), (3, 5), (64, 64), (17, 31), (200, 304), (1, 7), (96, 128)]
  gaps = [37, 1, 64, 3, 130, 2, 5, 41]
  total = sum(gaps) + sum(h * w * 3 for h, w in sizes)
  flat = torch.empty(total, dtype=dtype, device=dev)
  bits = flat.view(torch.int16 if dtype == torch.float16 else torch.int32)
  bits.fill_(0x5A5B if dtype == torch.float16 else 0x5A5B5C5D)
  sentinel = bits.clone()
  ys, spans, off = [], [], gaps[0]
  for (h, w), gap in zip(sizes, gaps[1:]):
    ys.append(flat[off:off + h * w * 3].view(1, h, w, 3))
    spans.append((off, off + h * w * 3))
    off += h * w * 3 + gap
  xs = [torch.from_numpy(synthetic.make_images(rng, (1, h, w, 3), NP_DT[dtype])).to(dev) for h, w in sizes]
  ids, p = make_sequences(rng, len(sizes), 8)
  ids, p = torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev)
  _cabi.chain_fused_fwd_ragged(ids, p, xs, ys)
  torch.cuda.synchronize()
  inside = torch.zeros(total, dtype=torch.bool, device=dev)
  for a, b in spans:
    inside[a:b] = True
  assert torch.equal(bits[~inside], sentinel[~inside]), 'a gap element was overwritten'
  for y, r in zip(ys, dense(ids, p, xs)):
    assert torch.equal(y, r)


def test_more_images_than_one_launch_table(gpu_device):
  """150 small images of varied sizes (three launches of the 64-image table) == the one-image kernel per image."""
  dev = gpu_device
  rng = np.random.default_rng(9)
  sizes = [(int(rng.integers(1, 41)), int(rng.integers(1, 41))) for _ in range(150)]
  sizes[70] = (64, 64)
  sizes[130] = (130, 70)
  xs = carve(sizes, torch.float16, dev, odd=97)
  for x in xs:
    x.copy_(torch.from_numpy(synthetic.make_images(rng, tuple(x.shape), np.float16)))
  ids, p = make_sequences(rng, len(sizes), 5)
  ids, p = torch.from_numpy(ids).to(dev), torch.from_numpy(p).to(dev)
  ys = evaluate.fused_chain_ragged(xs, ids, p)
  for i, (y, r) in enumerate(zip(ys, dense(ids, p, xs))):
    assert torch.equal(y, r), (i, sizes[i])


def _agent_inputs(cfg, n, dev, seed):
  g = torch.Generator(device=dev).manual_seed(seed)
  z = torch.rand(n, cfg.z_dim, device=dev, generator=g)
  masks = [[(torch.rand(n, 4096, device=dev, generator=g) < 0.5).float() for _ in range(2)]
           for _ in range(cfg.test_steps)]
  return z, masks


def test_retouch_batch_same_size_equals_retouch_on_the_stack(gpu_device):
  dev = gpu_device
  torch.manual_seed(3)
  cfg = make_cfg()
  ag = xagent.Agent(cfg).to(dev)
  x = torch.from_numpy(synthetic.make_images(np.random.default_rng(8), (3, 200, 304, 3), np.float16)).to(dev)
  z, masks = _agent_inputs(cfg, 3, dev, 4)
  outs, low, states, ops = evaluate.retouch_batch(ag, [x[i:i + 1].clone() for i in range(3)], z=z,
                                                  dropout_masks=masks, return_trace='full')
  ref, rlow, rstates, rops = evaluate.retouch(ag, x, z=z, dropout_masks=masks, return_trace='full')
  for i in range(3):
    assert torch.equal(outs[i], ref[i:i + 1]), i
  assert torch.equal(low, rlow) and torch.equal(states, rstates)
  for k in rops:
    assert torch.equal(ops[k], rops[k]), k


def test_retouch_batch_mixed_sizes_against_retouch_per_image(gpu_device):
  """Each image against retouch of that image alone with its rows of z and the masks.  The agent runs at N = 3 in one
  case and N = 1 in the other; where its kernels pick batch-dependent decompositions the regressed parameters may
  differ in the last bits, so the outputs are compared within the image tolerance (fp32 storage), while the
  selections and states must be equal."""
  dev = gpu_device
  torch.manual_seed(5)
  cfg = make_cfg()
  ag = xagent.Agent(cfg).to(dev)
  rng = np.random.default_rng(12)
  sizes = [(96, 160), (128, 80), (67, 67)]
  imgs = [torch.from_numpy(synthetic.make_images(rng, (1, h, w, 3), np.float32)).to(dev) for h, w in sizes]
  z, masks = _agent_inputs(cfg, 3, dev, 6)
  outs, low, states, trace = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace=True)
  for i, im in enumerate(imgs):
    mi = [[m[i:i + 1] for m in step] for step in masks]
    ref, rlow, rstates, rtrace = evaluate.retouch(ag, im, z=z[i:i + 1], dropout_masks=mi, return_trace=True)
    assert torch.equal(trace[i:i + 1], rtrace) and torch.equal(states[i:i + 1], rstates), i
    assert outs[i].shape == im.shape
    assert_image_close(outs[i].cpu().numpy(), ref.cpu().numpy(), np.float32, 'retouch_batch image %d' % i)
    assert_image_close(low[i:i + 1].cpu().numpy(), rlow.cpu().numpy(), np.float32, 'proxy %d' % i)


def test_cli_batch_writes_what_retouch_batch_computes(gpu_device, tmp_path):
  from PIL import Image
  from exposure_amd.tiff16 import write_tiff
  dev = gpu_device
  rng = np.random.default_rng(14)
  tif = str(tmp_path / 'a.tif')
  write_tiff(tif, (rng.random((64, 64, 3))**1.5 * 40000).astype(np.uint16))
  paths = [tif]
  for k, (h, w) in enumerate([(96, 160), (121, 75)]):
    paths.append(str(tmp_path / ('p%d.png' % k)))
    Image.fromarray((rng.random((h, w, 3)) * 255).astype(np.uint8), 'RGB').save(paths[-1])
  out_dir = str(tmp_path / 'out') + os.sep
  recs = evaluate.main(['--batch', '3', '--seed', '21', '--out', out_dir] + paths)
  assert [r['image'] for r in recs] == paths
  assert sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) + '.retouched.npy' for p in paths)
  # the same run in-process: seed, random-init agent, images as the CLI loads them (fp16), one batch
  torch.manual_seed(21)
  ag = xagent.Agent(make_cfg()).to(dev)
  his = [torch.from_numpy(np.ascontiguousarray(evaluate.load_image(p))).to(dev).to(torch.float16)[None] for p in paths]
  outs, _low, states, ops = evaluate.retouch_batch(ag, his, return_trace='full')
  for i, (rec, out) in enumerate(zip(recs, outs)):
    got = np.load(rec['output'])
    assert got.shape == tuple(his[i].shape[1:])
    assert np.array_equal(got, out[0].float().cpu().numpy()), rec['image']
    assert rec['abi_filter_ids'] == ops['abi_filter_ids'][i].cpu().tolist()
    assert rec['states'] == states[i].cpu().tolist()
