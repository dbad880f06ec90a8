"""CPU: evaluate.retouch / retouch_batch and the CLI with cfg.masking and masks='fused', with the C-ABI binding mocked by
the oracle (tests/_fake_hip.py) and a stand-in for chain_fused_masked_fwd_ragged defined here by what the kernel
promises: oracle/filters_torch.py::apply_masked step by step in float64, no rounding between steps, storage tap k the
running image after step k, the u8 tap save_png's encoding of it.  The GPU counterpart is
tests/test_hip_masked_chain.py."""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import agent as xagent
from exposure_amd import evaluate
from exposure_amd.config import make_cfg
from exposure_amd.util import tanh_range
from oracle import filters_torch as ft
from tests import _fake_hip
from tests.test_taps_host import _write_inputs, fake_taps, host_u8, images, inputs

calls = []  # the number of images of every call of the stand-in


def _masked_ragged(ids, params, mask_params, xs, ys, maximum_sharpness, minimum_strength, tap_mask=0, taps=None):
  calls.append(len(xs))
  assert mask_params.shape == (len(xs), ids.shape[1], 6) and mask_params.dtype == torch.float32
  assert ys is not None or tap_mask
  for i, x in enumerate(xs):
    cur = x.reshape(1, *x.shape[-3:]).double()
    j = 0
    for k in range(ids.shape[1]):
      fid = int(ids[i, k])
      if fid < 0:
        cur = torch.zeros_like(cur)
      else:
        cur = ft.apply_masked(fid, cur, params[i:i + 1, k, :_fake_hip.NUM_PARAMS[fid]].double(),
                              _fake_hip._raw_mask(mask_params[i:i + 1, k]), maximum_sharpness, minimum_strength)
      if (tap_mask >> k) & 1:
        s = cur[0].to(x.dtype)
        taps[i][j].copy_(torch.from_numpy(host_u8(s.float().numpy())) if taps[i].dtype == torch.uint8 else s)
        j += 1
    assert taps is None or j == taps[i].shape[0]
    if ys is not None:
      ys[i].copy_(cur.reshape(x.shape).to(x.dtype))


@contextlib.contextmanager
def fake_masked():
  with fake_taps(), mock.patch.multiple('exposure_amd._cabi', chain_fused_masked_fwd_ragged=_masked_ragged):
    yield


def masked_agent(seed=4):
  cfg = make_cfg()
  cfg.masking = True
  torch.manual_seed(seed)
  return cfg, xagent.Agent(cfg)


def close(a, b, what=''):
  """both schedules are the same float64 maths on the stand-ins; only the float32 storage rounding between the steps of
  the stepwise one differs"""
  assert a.shape == b.shape and a.dtype == b.dtype, what
  assert float((a.double() - b.double()).abs().max()) <= 1e-6, what


SIZES = [(40, 56), (23, 17), (64, 48)]


def test_defaults_do_not_reach_the_new_binding():
  cfg, ag = masked_agent()
  imgs = images(SIZES, 7)
  z, masks = inputs(cfg, 3, 8)
  del calls[:]
  with fake_masked():
    hi = imgs[0]
    a = evaluate.retouch(ag, hi, z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], return_trace=True,
                         intermediates='storage', picture=True)
    b = evaluate.retouch(ag, hi, z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], return_trace=True,
                         fused=False, intermediates='storage', picture=True)
    for u, v in zip(a, b):  # cfg.masking without masks= is the reference's schedule, as before
      assert torch.equal(u, v)
    outs, low, states, trace = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace=True)
    for i, im in enumerate(imgs):  # ... and every image alone
      r = evaluate.retouch(ag, im, z=z[i:i + 1], dropout_masks=[[m[i:i + 1] for m in s] for s in masks],
                           return_trace=True, fused=False)
      assert torch.equal(outs[i], r[0]) and torch.equal(low[i:i + 1], r[1]) and torch.equal(trace[i:i + 1], r[3])
  assert calls == []


def test_fused_masks_without_masking_is_the_existing_fused_path():
  cfg = make_cfg()
  torch.manual_seed(4)
  ag = xagent.Agent(cfg)
  imgs = images(SIZES, 7)
  z, masks = inputs(cfg, 3, 8)
  del calls[:]
  with fake_masked():
    a = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full', masks='fused')
    b = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full')
    c = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], masks='fused')
    d = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks])
  assert calls == [] and sorted(a[3]) == sorted(b[3]) == ['abi_filter_ids', 'params24', 'selected']
  assert all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and torch.equal(c[0], d[0])
  with pytest.raises(ValueError):
    evaluate.retouch(ag, imgs[0], masks='both')
  with pytest.raises(ValueError):
    evaluate.retouch_batch(ag, imgs, masks=True)


@pytest.mark.parametrize('kind', ['u8', 'storage'])
def test_retouch_batch_fused_masks_equal_the_stepwise_schedule(kind):
  cfg, ag = masked_agent()
  imgs = images(SIZES, 7)
  imgs[1] = imgs[1][0]
  z, masks = inputs(cfg, 3, 8)
  del calls[:]
  with fake_masked(), mock.patch.object(ag, 'forward', wraps=ag.forward) as fwd:
    outs, low, states, ops, inter, pics = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full',
                                                                 intermediates=kind, picture=True, masks='fused')
    batch_sizes = [c.args[0][0].shape[0] for c in fwd.call_args_list]
    routs, rlow, rstates, rops, rinter, rpics = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks,
                                                                      return_trace='full', intermediates=kind, picture=True)
  assert batch_sizes == [3] * cfg.test_steps  # the agent ran once on the stacked proxies, not once per image
  assert calls == [3]  # one ragged call: outputs, pictures and intermediates
  assert torch.equal(ops['selected'], rops['selected']) and torch.equal(ops['abi_filter_ids'], rops['abi_filter_ids'])
  close(ops['params24'], rops['params24'], 'params24')
  assert ops['mask6'].shape == (3, cfg.test_steps, 6)
  close(ops['mask6'], rops['mask6'], 'mask6')
  close(low, rlow, 'low')
  assert torch.equal(states, rstates)
  for i, im in enumerate(imgs):
    close(outs[i], routs[i], 'out %d' % i)
    assert inter[i].shape == (cfg.test_steps - 1,) + tuple(im.shape[-3:])
    if kind == 'storage':
      close(inter[i], rinter[i], 'intermediates %d' % i)
    else:  # 8-bit values: the same picture up to one level where a value sits on a rounding boundary
      assert inter[i].dtype == torch.uint8 and int((inter[i].int() - rinter[i].int()).abs().max()) <= 1
      assert float((inter[i] != rinter[i]).float().mean()) < 1e-3
    assert pics[i].shape == tuple(im.shape[-3:]) and pics[i].dtype == torch.uint8
    np.testing.assert_array_equal(pics[i].numpy(), host_u8(outs[i].reshape(im.shape[-3:]).numpy()))
    assert int((pics[i].int() - rpics[i].int()).abs().max()) <= 1


def test_retouch_fused_masks_dense_batch():
  """a dense (N, H, W, 3) tensor goes in as N views of one ragged call"""
  cfg, ag = masked_agent()
  hi = torch.cat(images([(24, 40)] * 2, 1))
  z, masks = inputs(cfg, 2, 2)
  del calls[:]
  with fake_masked():
    out, low, states, ops, st, pic = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace='full',
                                                      intermediates='storage', picture=True, masks='fused')
    out8, _, _, trace, u8, pic8 = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace=True,
                                                   intermediates='u8', picture=True, masks='fused')
    plain = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, masks='fused')
    ref, rlow, rstates, rops, rst, rpic = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace='full',
                                                           intermediates='storage', picture=True)
    stepwise_wins = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, fused=False, masks='fused')
  assert calls == [2, 2, 2]
  assert torch.equal(stepwise_wins[0], ref)
  close(out, ref, 'out')
  assert torch.equal(out8, out) and torch.equal(plain[0], out) and torch.equal(trace, rops['selected'])
  assert st.shape == (cfg.test_steps - 1, 2, 24, 40, 3) and st.dtype == hi.dtype
  close(st, rst, 'intermediates')
  np.testing.assert_array_equal(u8.numpy(), host_u8(st.numpy()))
  np.testing.assert_array_equal(pic.numpy(), host_u8(out.numpy()))
  assert torch.equal(pic8, pic) and int((pic.int() - rpic.int()).abs().max()) <= 1
  assert sorted(ops) == sorted(rops) == ['abi_filter_ids', 'mask6', 'params24', 'selected']
  close(ops['mask6'], rops['mask6'], 'mask6')


def test_debug_info_mask6_is_the_selected_heads_squashed_rows():
  cfg, ag = masked_agent()
  n = 4
  low = torch.cat(images([(64, 64)] * n, 3))
  z, masks = inputs(cfg, n, 5)
  states = torch.zeros((n, cfg.num_state_dim))
  with fake_masked(), torch.no_grad():
    _, dbg, _ = ag((low, z, states), is_train=0, progress=0.0, dropout_masks=masks[0])
    feats = ag.filter_features(xagent.enrich_image_input(cfg, low, states), masks[0][0])
    want = torch.stack([tanh_range(-5, 5, initial=0)(ag.filters[int(j)].extract_parameters(feats)[1][i].float())
                        for i, j in enumerate(dbg['selected_filter_ids'])])
  assert dbg['mask6'].shape == (n, 6) and torch.equal(dbg['mask6'], want)
  cfg2 = make_cfg()
  torch.manual_seed(4)
  with fake_masked(), torch.no_grad():
    _, dbg2, _ = xagent.Agent(cfg2)((low, z, states), is_train=0, progress=0.0, dropout_masks=masks[0])
  assert 'mask6' not in dbg2 and sorted(set(dbg) - set(dbg2)) == ['mask6']


def test_cli_fused_masks_writes_the_unmasked_clis_files(tmp_path):
  paths = _write_inputs(tmp_path, [(20, 30), (17, 9), (32, 32)])
  common = ['--seed', '3', '--dtype', 'f32', '--batch', '3', '--step-by-step', '--device-png']
  del calls[:]
  with fake_masked(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    plain = evaluate.main(common + ['--out', str(tmp_path / 'plain') + os.sep] + paths)
    assert calls == []
    recs = evaluate.main(common + ['--masking', '--fused-masks', '--out', str(tmp_path / 'masked') + os.sep] + paths)
    assert calls == [3]
    stepwise = evaluate.main(common + ['--masking', '--fused-masks', '--stepwise', '--out',
                                       str(tmp_path / 'stepwise') + os.sep] + paths)
    assert calls == [3]  # --stepwise wins
  assert sorted(os.listdir(tmp_path / 'masked')) == sorted(os.listdir(tmp_path / 'plain')) == \
      sorted(os.listdir(tmp_path / 'stepwise'))
  assert len(os.listdir(tmp_path / 'masked')) == 3 * (1 + 1 + 4)  # .npy, .png, four intermediates
  for rec, ref in zip(recs, plain):
    assert sorted(rec['png']) == sorted(ref['png']) and all(os.path.exists(f) for f in rec['png'].values())
