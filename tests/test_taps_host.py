"""CPU: the step-by-step intermediates of evaluate.retouch / retouch_batch and of the CLI's --step-by-step, with the
C-ABI binding mocked by the oracle (tests/_fake_hip.py) and tap stand-ins defined here by what the tap kernels
promise: storage tap k is the fused chain of the truncated sequence ids[:, :k+1], the u8 tap is save_png's encoding of
it.  The GPU counterpart is tests/test_hip_chain_taps.py."""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import agent as xagent
from exposure_amd import evaluate
from exposure_amd.config import make_cfg
from tests import _fake_hip
from tests._fake_hip import fake_hip


def host_u8(a):
  """evaluate.save_png's encoding of a float array"""
  return np.clip(np.rint(np.asarray(a, dtype=np.float32) * 255.0), 0, 255).astype(np.uint8)


def _truncated(ids, params, x, k):
  s = torch.empty_like(x)
  _fake_hip._chain_fused_fwd(ids[:, :k + 1], params[:, :k + 1], x, s)
  return s


def _taps_fwd(ids, params, x, y, tap_mask, taps):
  if y is not None:
    _fake_hip._chain_fused_fwd(ids, params, x, y)
  j = 0
  for k in range(ids.shape[1]):
    if (tap_mask >> k) & 1:
      s = _truncated(ids, params, x, k)
      taps[j].copy_(torch.from_numpy(host_u8(s.float().numpy())) if taps.dtype == torch.uint8 else s)
      j += 1
  assert taps is None or j == taps.shape[0]


def _ragged_fwd(ids, params, xs, ys):
  for i, (x, y) in enumerate(zip(xs, ys)):
    x4, y4 = (x, y) if x.dim() == 4 else (x[None], y[None])
    _fake_hip._chain_fused_fwd(ids[i:i + 1], params[i:i + 1], x4, y4)


calls = []


def _ragged_taps_fwd(ids, params, xs, ys, tap_mask, taps):
  calls.append(len(xs))
  for i, x in enumerate(xs):
    x4 = x if x.dim() == 4 else x[None]
    y4 = None if ys is None else ys[i].reshape(x4.shape)
    _taps_fwd(ids[i:i + 1], params[i:i + 1], x4, y4, tap_mask, None if taps is None else taps[i][:, None])


@contextlib.contextmanager
def fake_taps():
  with fake_hip(), mock.patch.multiple('exposure_amd._cabi', chain_fused_fwd_ragged=_ragged_fwd,
                                       chain_fused_fwd_taps=_taps_fwd, chain_fused_fwd_ragged_taps=_ragged_taps_fwd):
    yield


def images(sizes, seed):
  rng = np.random.default_rng(seed)
  return [torch.from_numpy(rng.random((1, h, w, 3), dtype=np.float32)**2.2 * 1.6) for h, w in sizes]


def inputs(cfg, n, seed):
  g = torch.Generator().manual_seed(seed)
  z = torch.rand(n, cfg.z_dim, generator=g)
  masks = [[(torch.rand(n, 4096, generator=g) < 0.5).float() for _ in range(2)] for _ in range(cfg.test_steps)]
  return z, masks


def agent(cfg, seed=4):
  torch.manual_seed(seed)
  return xagent.Agent(cfg)


def test_retouch_intermediates_are_the_truncated_chains():
  cfg = make_cfg()
  ag = agent(cfg)
  hi = torch.cat(images([(24, 40)] * 2, 1))
  z, masks = inputs(cfg, 2, 2)
  with fake_taps():
    out, low, states, ops, st = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace='full',
                                                 intermediates='storage')
    out8, low8, states8, ops8, u8 = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace='full',
                                                     intermediates='u8')
    ref, rlow, rstates, rops = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace='full')
  # every step but the last: the shipped agent stops the images after step cfg.test_steps - 1
  assert st.shape == (cfg.test_steps - 1, 2, 24, 40, 3) and st.dtype == hi.dtype
  assert u8.shape == st.shape and u8.dtype == torch.uint8
  # the outputs and traces without intermediates are unchanged
  for o in (out, out8):
    assert torch.equal(o, ref)
  assert torch.equal(states, rstates) and torch.equal(low8, rlow)
  for k in rops:
    assert torch.equal(ops[k], rops[k]) and torch.equal(ops8[k], rops[k])
  ids, prm = ops['abi_filter_ids'].int(), ops['params24']
  for k in range(cfg.test_steps - 1):
    assert torch.equal(st[k], _truncated(ids, prm, hi, k)), k
    np.testing.assert_array_equal(u8[k].numpy(), host_u8(st[k].numpy()))


def test_fewer_steps_than_test_steps_keep_every_step():
  """Stopping follows the step counter: a 3-step run never stops, so all 3 steps have a picture."""
  cfg = make_cfg()
  ag = agent(cfg)
  hi = images([(16, 24)], 3)[0]
  z, masks = inputs(cfg, 1, 4)
  with fake_taps():
    res = evaluate.retouch(ag, hi, steps=3, z=z, dropout_masks=masks, intermediates='u8')
  assert len(res) == 4 and res[3].shape == (3, 1, 16, 24, 3)


def test_stepwise_intermediates_are_the_per_step_tensors():
  cfg = make_cfg()
  ag = agent(cfg)
  hi = images([(20, 28)], 5)[0]
  z, masks = inputs(cfg, 1, 6)
  with fake_taps():
    _, _, _, trace, fused8 = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace=True, intermediates='u8')
    _, _, _, trace2, step8 = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace=True, fused=False,
                                              intermediates='u8')
    _, _, _, _, stepst = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace=True, fused=False,
                                          intermediates='storage')
  assert torch.equal(trace, trace2)
  assert step8.shape == fused8.shape == (cfg.test_steps - 1, 1, 20, 28, 3) and step8.dtype == torch.uint8
  np.testing.assert_array_equal(step8.numpy(), host_u8(stepst.numpy()))  # the device encode is save_png's
  # same maths, fp32 between steps either way: at most one level apart at a rounding boundary
  assert int((step8.int() - fused8.int()).abs().max()) <= 1


def test_bad_intermediates_value():
  cfg = make_cfg()
  ag = agent(cfg)
  with pytest.raises(ValueError):
    evaluate.retouch(ag, images([(8, 8)], 0)[0], intermediates='png')
  with pytest.raises(ValueError):
    evaluate.retouch_batch(ag, images([(8, 8)], 0), intermediates=True)


def test_retouch_batch_intermediates_per_image():
  cfg = make_cfg()
  ag = agent(cfg)
  sizes = [(40, 56), (23, 17), (64, 48)]
  imgs = images(sizes, 7)
  imgs[1] = imgs[1][0]
  z, masks = inputs(cfg, 3, 8)
  del calls[:]
  with fake_taps():
    outs, low, states, ops, inter = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full',
                                                           intermediates='u8')
    ref, _, _, rops = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full')
    _, _, _, st = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, intermediates='storage')
  assert calls == [3, 3]  # one ragged call with taps for the whole list (per format)
  assert [tuple(t.shape) for t in inter] == [(4, h, w, 3) for h, w in sizes]
  assert all(t.dtype == torch.uint8 for t in inter) and all(t.dtype == torch.float32 for t in st)
  for i, im in enumerate(imgs):
    assert torch.equal(outs[i], ref[i])
    im4 = im.reshape(1, *im.shape[-3:])
    for k in range(4):
      s = _truncated(ops['abi_filter_ids'][i:i + 1].int(), ops['params24'][i:i + 1], im4, k)
      assert torch.equal(st[i][k], s[0]), (i, k)
      np.testing.assert_array_equal(inter[i][k].numpy(), host_u8(s[0].numpy()))


def test_retouch_batch_generic_curves_fall_back_with_intermediates():
  cfg = make_cfg()
  cfg.curve_steps = 4
  ag = agent(cfg)
  imgs = images([(24, 40), (33, 21)], 9)
  z, masks = inputs(cfg, 2, 10)
  with fake_taps():
    outs, _, _, inter = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, intermediates='u8')
    for i, im in enumerate(imgs):
      r = evaluate.retouch(ag, im, z=z[i:i + 1], dropout_masks=[[m[i:i + 1] for m in s] for s in masks],
                           intermediates='u8')
      assert torch.equal(outs[i], r[0]) and torch.equal(inter[i], r[3][:, 0])
  assert [tuple(t.shape) for t in inter] == [(4, 24, 40, 3), (4, 33, 21, 3)]


def _write_inputs(tmp_path, sizes):
  from PIL import Image
  rng = np.random.default_rng(11)
  paths = []
  for i, (h, w) in enumerate(sizes):
    p = str(tmp_path / ('in%d.png' % i))
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'RGB').save(p)
    paths.append(p)
  return paths


@pytest.mark.parametrize('mode', [['--batch', '1'], ['--batch', '3'], ['--stepwise']])
def test_cli_step_by_step_files_and_records(tmp_path, mode):
  from PIL import Image
  sizes = [(20, 30), (17, 9), (32, 32)]
  paths = _write_inputs(tmp_path, sizes)
  out = str(tmp_path / 'out') + os.sep
  with fake_taps(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    recs = evaluate.main(['--seed', '3', '--dtype', 'f32', '--step-by-step', '--out', out, *mode, *paths])
  assert len(recs) == 3
  for rec, p, (h, w) in zip(recs, paths, sizes):
    stem = os.path.join(out, os.path.basename(p)) + '.retouched'
    keys = ['intermediate%02d' % i for i in range(4)]
    assert sorted(rec['png']) == sorted(['retouched'] + keys)  # --step-by-step implies --png
    for k in keys:
      assert rec['png'][k] == '%s.%s.png' % (stem, k) and os.path.exists(rec['png'][k])
      a = np.asarray(Image.open(rec['png'][k]))
      assert a.shape == (h, w, 3) and a.dtype == np.uint8
    assert not os.path.exists('%s.intermediate04.png' % stem)
  # the last intermediate and the retouched picture come from different sequences: step 4 ran in between
  # (and each PNG is the replayed truncated chain of the record's own sequence)
  rec = recs[0]
  x = torch.from_numpy(np.ascontiguousarray(evaluate.load_image(paths[0]))).float()[None]
  ids = torch.tensor([rec['abi_filter_ids']], dtype=torch.int32)
  prm = torch.from_numpy(rec['params24'])[None].float()
  for k in range(4):
    want = host_u8(_truncated(ids, prm, x, k)[0].numpy())
    got = np.asarray(Image.open(rec['png']['intermediate%02d' % k]))
    assert int(np.abs(got.astype(int) - want.astype(int)).max()) <= (1 if mode == ['--stepwise'] else 0), k
