"""CPU: evaluate.retouch_batch (images of different sizes retouched at once) with the C-ABI binding mocked by the
oracle (tests/_fake_hip.py), plus a ragged stand-in defined here as a per-image loop over the fake's one-image fused
chain.  The GPU counterpart is tests/test_hip_ragged_chain.py."""
import contextlib
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import agent as xagent
from exposure_amd import evaluate
from exposure_amd.config import make_cfg
from oracle import filters_np as fnp
from tests import _fake_hip
from tests._fake_hip import fake_hip


def _ragged_fwd(ids, params, xs, ys):
  assert ids.shape[0] == params.shape[0] == len(xs) == len(ys)
  for i, (x, y) in enumerate(zip(xs, ys)):
    x4, y4 = (x, y) if x.dim() == 4 else (x[None], y[None])
    _fake_hip._chain_fused_fwd(ids[i:i + 1], params[i:i + 1], x4, y4)


@contextlib.contextmanager
def fake_ragged():
  with fake_hip(), mock.patch('exposure_amd._cabi.chain_fused_fwd_ragged', _ragged_fwd):
    yield


def images(sizes, seed):
  rng = np.random.default_rng(seed)
  return [torch.from_numpy(rng.random((1, h, w, 3), dtype=np.float32)**2.2) for h, w in sizes]


def inputs(cfg, n, seed):
  g = torch.Generator().manual_seed(seed)
  z = torch.rand(n, cfg.z_dim, generator=g)
  masks = [[(torch.rand(n, 4096, generator=g) < 0.5).float() for _ in range(2)] for _ in range(cfg.test_steps)]
  return z, masks


def rows(z, masks, idx):
  return z[idx], [[m[idx] for m in step] for step in masks]


def agent(cfg, seed=4):
  torch.manual_seed(seed)
  return xagent.Agent(cfg)


def test_same_size_equals_retouch_on_the_stacked_tensor():
  cfg = make_cfg()
  ag = agent(cfg)
  imgs = images([(40, 56)] * 3, 1)
  z, masks = inputs(cfg, 3, 2)
  with fake_ragged():
    outs, low, states, ops = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full')
    ref, rlow, rstates, rops = evaluate.retouch(ag, torch.cat(imgs), z=z, dropout_masks=masks, return_trace='full')
  assert len(outs) == 3
  for i, o in enumerate(outs):
    assert o.shape == imgs[i].shape and torch.equal(o, ref[i:i + 1])
  assert torch.equal(low, rlow) and torch.equal(states, rstates)
  for k in ('selected', 'abi_filter_ids', 'params24'):
    assert torch.equal(ops[k], rops[k]), k


def test_mixed_sizes_give_each_image_its_own_sequence():
  cfg = make_cfg()
  ag = agent(cfg)
  sizes = [(40, 56), (23, 17), (64, 64)]
  imgs = images(sizes, 3)
  imgs[1] = imgs[1][0]  # (H, W, 3) is accepted as well and comes back in that shape
  z, masks = inputs(cfg, 3, 4)
  with fake_ragged():
    outs, low, states, trace = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace=True)
    _, _, _, ops = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full')
  assert [tuple(o.shape) for o in outs] == [(1, 40, 56, 3), (23, 17, 3), (1, 64, 64, 3)]
  assert low.shape == (3, 64, 64, 3) and states.shape == (3, cfg.num_state_dim) and trace.shape == (3, 5)
  assert states[:, 2].tolist() == [5.0, 5.0, 5.0]
  for i, (im, o) in enumerate(zip(imgs, outs)):  # the recorded sequence of image i, replayed by the oracle on image i
    ref = im.reshape(1, *im.shape[-3:]).double().numpy()
    for fid, p24 in zip(ops['abi_filter_ids'][i].tolist(), ops['params24'][i].numpy()):
      ref = fnp.process_packed(fid, ref, p24[None, :fnp.NUM_PARAMS[fid]].astype(np.float64))
    np.testing.assert_allclose(o.reshape(ref.shape).numpy(), ref, rtol=2e-6, atol=1e-7)


def test_z_and_mask_rows_reach_their_image():
  """Permuting the images together with their rows of z and of every mask permutes the results."""
  cfg = make_cfg()
  ag = agent(cfg)
  imgs = images([(40, 56), (23, 17), (64, 48)], 5)
  z, masks = inputs(cfg, 3, 6)
  perm = [2, 0, 1]
  pz, pmasks = rows(z, masks, perm)
  with fake_ragged():
    a, la, sa, ta = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace=True)
    b, lb, sb, tb = evaluate.retouch_batch(ag, [imgs[j] for j in perm], z=pz, dropout_masks=pmasks, return_trace=True)
  assert torch.equal(ta[perm], tb)
  np.testing.assert_allclose(sa[perm].numpy(), sb.numpy(), rtol=1e-6, atol=1e-7)
  for k, j in enumerate(perm):
    np.testing.assert_allclose(b[k].numpy(), a[j].numpy(), rtol=1e-5, atol=1e-6)
  # and the rows are not interchangeable: another image's z and masks change what an image gets
  sz, smasks = rows(z, masks, [1, 2, 0])
  with fake_ragged():
    _, _, _, tc = evaluate.retouch_batch(ag, imgs, z=sz, dropout_masks=smasks, return_trace=True)
  assert not torch.equal(ta, tc)


def test_generic_curves_fall_back_to_retouch_per_image():
  """cfg.curve_steps = 4 has no one-pass kernel: every image runs through retouch alone with its rows."""
  cfg = make_cfg()
  cfg.curve_steps = 4
  ag = agent(cfg)
  imgs = images([(24, 40), (33, 21)], 7)
  z, masks = inputs(cfg, 2, 8)
  called = []
  with fake_ragged(), mock.patch('exposure_amd._cabi.chain_fused_fwd_ragged', lambda *a: called.append(a)):
    outs, low, states, ops = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full')
  assert not called
  with fake_ragged():
    for i, im in enumerate(imgs):
      zi, mi = rows(z, masks, slice(i, i + 1))
      ref, rlow, rstates, rops = evaluate.retouch(ag, im, z=zi, dropout_masks=mi, return_trace='full')
      assert torch.equal(outs[i], ref) and torch.equal(low[i:i + 1], rlow) and torch.equal(states[i:i + 1], rstates)
      for k in rops:
        assert torch.equal(ops[k][i:i + 1], rops[k]), k
