"""CPU: evaluate.retouch / retouch_batch and the CLIs with a generic cfg.curve_steps and curves='fused', with the C-ABI
binding mocked by the oracle (tests/_fake_hip.py) and a stand-in for chain_fused_curves_fwd_ragged defined here by what
the kernel promises: oracle/filters_np.py::process_packed step by step in float64, no rounding between steps, storage
tap k the running image after step k, the u8 tap save_png's encoding of it.  The GPU counterpart is
tests/test_hip_curves_chain.py."""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import agent as xagent
from exposure_amd import evaluate, train
from exposure_amd.config import make_cfg
from oracle import filters_np as fnp
from tests.test_taps_host import _write_inputs, fake_taps, host_u8, images, inputs

calls = []  # (the number of images, L) of every call of the stand-in


def row_len(fid, L):
  return L if fid == 4 else 3 * L if fid == 7 else fnp.NUM_PARAMS[fid]


def _curves_ragged(ids, params48, curve_steps, xs, ys, tap_mask=0, taps=None):
  calls.append((len(xs), curve_steps))
  assert params48.shape == (len(xs), ids.shape[1], 48) and params48.dtype == torch.float32
  assert ys is not None or tap_mask
  for i, x in enumerate(xs):
    cur = x.reshape(1, *x.shape[-3:]).double().numpy()
    j = 0
    for k in range(ids.shape[1]):
      fid = int(ids[i, k])
      if fid < 0:
        cur = np.zeros_like(cur)
      else:
        cur = fnp.process_packed(fid, cur, params48[i:i + 1, k, :row_len(fid, curve_steps)].double().numpy())
      if (tap_mask >> k) & 1:
        s = torch.from_numpy(cur[0]).to(x.dtype)
        taps[i][j].copy_(torch.from_numpy(host_u8(s.float().numpy())) if taps[i].dtype == torch.uint8 else s)
        j += 1
    assert taps is None or j == taps[i].shape[0]
    if ys is not None:
      ys[i].copy_(torch.from_numpy(cur).reshape(x.shape).to(x.dtype))


@contextlib.contextmanager
def fake_curves():
  with fake_taps(), mock.patch.multiple('exposure_amd._cabi', chain_fused_curves_fwd_ragged=_curves_ragged):
    yield


def generic_agent(L, seed=4, masking=False):
  cfg = make_cfg()
  cfg.curve_steps = L
  cfg.masking = masking
  torch.manual_seed(seed)
  return cfg, xagent.Agent(cfg)


def close(a, b, what=''):
  """both schedules are the same float64 maths on the stand-ins; only the float32 storage rounding between the steps of
  the stepwise one differs (the figure of tests/test_masked_chain_host.py for the same comparison)"""
  assert a.shape == b.shape and a.dtype == b.dtype, what
  assert float((a.double() - b.double()).abs().max()) <= 1e-6, what


SIZES = [(40, 56), (23, 17), (64, 48)]


@pytest.mark.parametrize('L', [4, 16])
def test_defaults_do_not_reach_the_new_binding(L):
  cfg, ag = generic_agent(L)
  imgs = images(SIZES, 7)
  z, masks = inputs(cfg, 3, 8)
  del calls[:]
  with fake_curves():
    one = [[m[:1] for m in s] for s in masks]
    a = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=one, return_trace='full', intermediates='storage',
                         picture=True)
    b = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=one, return_trace='full', fused=False,
                         intermediates='storage', picture=True, curves='stepwise')
    assert sorted(a[3]) == sorted(b[3]) == ['abi_filter_ids', 'params24', 'selected']
    for u, v in zip(a[:3] + a[4:], b[:3] + b[4:]):  # generic curves without curves= are the reference's schedule
      assert torch.equal(u, v)
    outs, low, states, trace = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace=True)
    for i, im in enumerate(imgs):  # ... and every image alone
      r = evaluate.retouch(ag, im, z=z[i:i + 1], dropout_masks=[[m[i:i + 1] for m in s] for s in masks],
                           return_trace=True, fused=False)
      assert torch.equal(outs[i], r[0]) and torch.equal(low[i:i + 1], r[1]) and torch.equal(trace[i:i + 1], r[3])
  assert calls == []


def test_curves_has_no_effect_without_a_generic_filter_and_bad_values_raise():
  cfg = make_cfg()
  torch.manual_seed(4)
  ag = xagent.Agent(cfg)
  imgs = images(SIZES, 7)
  z, masks = inputs(cfg, 3, 8)
  del calls[:]
  with fake_curves():
    a = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full', curves='fused')
    b = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full')
    c = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], curves='fused')
    d = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks])
  assert calls == [] and sorted(a[3]) == sorted(b[3]) == ['abi_filter_ids', 'params24', 'selected']
  assert all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and torch.equal(c[0], d[0])
  assert evaluate.CURVES == ('stepwise', 'fused')
  with pytest.raises(ValueError):
    evaluate.retouch(ag, imgs[0], curves='both')
  with pytest.raises(ValueError):
    evaluate.retouch_batch(ag, imgs, curves=True)


@pytest.mark.parametrize('L', [4, 16])
@pytest.mark.parametrize('kind', ['u8', 'storage'])
def test_retouch_batch_fused_curves_equal_the_stepwise_schedule(kind, L):
  cfg, ag = generic_agent(L)
  imgs = images(SIZES, 7)
  imgs[1] = imgs[1][0]
  z, masks = inputs(cfg, 3, 8)
  del calls[:]
  with fake_curves(), mock.patch.object(ag, 'forward', wraps=ag.forward) as fwd:
    outs, low, states, ops, inter, pics = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full',
                                                                 intermediates=kind, picture=True, curves='fused')
    batch_sizes = [c.args[0][0].shape[0] for c in fwd.call_args_list]
    routs, rlow, rstates, rops, rinter, rpics = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks,
                                                                      return_trace='full', intermediates=kind, picture=True)
  assert batch_sizes == [3] * cfg.test_steps  # exactly one agent pass, on the stacked proxies
  assert calls == [(3, L)]  # exactly one stand-in call: outputs, pictures and intermediates
  assert torch.equal(ops['selected'], rops['selected']) and torch.equal(ops['abi_filter_ids'], rops['abi_filter_ids'])
  assert sorted(ops) == ['abi_filter_ids', 'params24', 'params48', 'selected'] and 'params48' not in rops
  assert ops['params48'].shape == (3, cfg.test_steps, 48) and ops['params24'].shape == rops['params24'].shape
  close(low, rlow, 'low')
  assert torch.equal(states, rstates)
  for i, im in enumerate(imgs):
    close(outs[i], routs[i], 'out %d' % i)
    assert inter[i].shape == (cfg.test_steps - 1,) + tuple(im.shape[-3:])
    if kind == 'storage':
      close(inter[i], rinter[i], 'intermediates %d' % i)
    else:  # 8-bit values: the same picture up to one level where a value sits on a rounding boundary
      assert inter[i].dtype == torch.uint8 and int((inter[i].int() - rinter[i].int()).abs().max()) <= 1
    assert pics[i].shape == tuple(im.shape[-3:]) and pics[i].dtype == torch.uint8
    np.testing.assert_array_equal(pics[i].numpy(), host_u8(outs[i].reshape(im.shape[-3:]).numpy()))
    assert int((pics[i].int() - rpics[i].int()).abs().max()) <= 1


@pytest.mark.parametrize('L', [4, 16])
def test_retouch_fused_curves_dense_batch(L):
  """a dense (N, H, W, 3) tensor goes in as N views of one ragged call"""
  cfg, ag = generic_agent(L)
  hi = torch.cat(images([(24, 40)] * 2, 1))
  z, masks = inputs(cfg, 2, 2)
  del calls[:]
  with fake_curves():
    out, low, states, ops, st, pic = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace='full',
                                                      intermediates='storage', picture=True, curves='fused')
    out8, _, _, trace, u8, pic8 = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace=True,
                                                   intermediates='u8', picture=True, curves='fused')
    plain = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, curves='fused')
    ref, rlow, rstates, rops, rst, rpic = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, return_trace='full',
                                                           intermediates='storage', picture=True)
    assert calls == [(2, L)] * 3
    stepwise_wins = evaluate.retouch(ag, hi, z=z, dropout_masks=masks, fused=False, curves='fused')
    assert calls == [(2, L)] * 3
    # the trace replays to the same bits
    again, _ = evaluate.fused_curves_chain(hi, ops['abi_filter_ids'], ops['params48'], L)
  assert torch.equal(stepwise_wins[0], ref) and torch.equal(again, out)
  close(out, ref, 'out')
  close(low, rlow, 'low')
  assert torch.equal(out8, out) and torch.equal(plain[0], out) and torch.equal(trace, rops['selected'])
  assert torch.equal(ops['selected'], rops['selected']) and torch.equal(ops['abi_filter_ids'], rops['abi_filter_ids'])
  assert st.shape == (cfg.test_steps - 1, 2, 24, 40, 3) and st.dtype == hi.dtype
  close(st, rst, 'intermediates')
  np.testing.assert_array_equal(u8.numpy(), host_u8(st.numpy()))
  np.testing.assert_array_equal(pic.numpy(), host_u8(out.numpy()))
  assert torch.equal(pic8, pic) and int((pic.int() - rpic.int()).abs().max()) <= 1
  assert sorted(ops) == ['abi_filter_ids', 'params24', 'params48', 'selected']


def test_masking_with_generic_curves_keeps_the_stepwise_schedule():
  cfg, ag = generic_agent(4, masking=True)
  imgs = images(SIZES[:2], 7)
  z, masks = inputs(cfg, 2, 8)
  del calls[:]
  with fake_curves():
    a = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], curves='fused',
                         masks='fused')
    b = evaluate.retouch(ag, imgs[0], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], fused=False)
    c = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, curves='fused')
  assert calls == [] and torch.equal(a[0], b[0]) and torch.equal(c[0][0], a[0])


@pytest.mark.parametrize('L', [4, 16])
def test_debug_info_params48_is_the_selected_filters_packed_row(L):
  cfg, ag = generic_agent(L)
  n = 6
  low = torch.cat(images([(64, 64)] * n, 3))
  z, masks = inputs(cfg, n, 5)
  states = torch.zeros((n, cfg.num_state_dim))
  seen = set()
  with fake_curves(), torch.no_grad():
    for step in range(3):
      (low, states, _s, _p), dbg, _ = ag((low, z, states), is_train=0, progress=0.0, dropout_masks=masks[step])
      p48 = dbg['params48']
      assert p48.shape == (n, 48) and p48.dtype == torch.float32
      assert torch.equal(dbg['abi_filter_ids'], ag.abi_filter_ids[dbg['selected_filter_ids'].long()])
      for i, j in enumerate(dbg['selected_filter_ids'].tolist()):
        row = dbg['packed_params'][j][i].float()
        assert row.numel() == row_len(int(ag.abi_filter_ids[j]), L)
        assert torch.equal(p48[i, :row.numel()], row) and not p48[i, row.numel():].any()
        seen.add(j)
  assert len(seen) >= 2
  cfg8 = make_cfg()
  torch.manual_seed(4)
  with fake_curves(), torch.no_grad():
    _, dbg8, _ = xagent.Agent(cfg8)((low, z, states), is_train=0, progress=0.0, dropout_masks=masks[0])
  assert 'params48' not in dbg8 and 'params24' in dbg8


def test_retouch_batch_raw_keeps_refusing_generic_curves():
  cfg, ag = generic_agent(4)
  with pytest.raises(ValueError, match='curve_steps'):
    evaluate.retouch_batch_raw(ag, [(np.zeros((8, 8, 3), np.uint8), 'srgb8')], torch.float32, 'cpu')


def test_cli_fused_curves_writes_the_stepwise_clis_files(tmp_path):
  paths = _write_inputs(tmp_path, [(20, 30), (17, 9), (32, 32)])
  common = ['--seed', '3', '--dtype', 'f32', '--batch', '3', '--step-by-step', '--device-png', '--curve-steps', '4']
  del calls[:]
  with fake_curves(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    plain = evaluate.main(common + ['--out', str(tmp_path / 'plain') + os.sep] + paths)
    assert calls == []
    recs = evaluate.main(common + ['--fused-curves', '--out', str(tmp_path / 'fused') + os.sep] + paths)
    assert calls == [(3, 4)]
    eight = evaluate.main(common[:-2] + ['--fused-curves', '--out', str(tmp_path / 'eight') + os.sep] + paths)
    assert calls == [(3, 4)]  # 8-step curves: no effect
  assert sorted(os.listdir(tmp_path / 'fused')) == sorted(os.listdir(tmp_path / 'plain')) == \
      sorted(os.listdir(tmp_path / 'eight'))
  assert len(os.listdir(tmp_path / 'fused')) == 3 * (1 + 1 + 4)  # .npy, .png, four intermediates
  for rec, ref in zip(recs, plain):
    assert sorted(rec['png']) == sorted(ref['png']) and all(os.path.exists(f) for f in rec['png'].values())


@pytest.mark.parametrize('argv', [
    ['--fused-curves', '--stepwise', 'a.png'],
    ['--curve-steps', '0', 'a.png'],
    ['--curve-steps', '17', 'a.png'],
    ['--curve-steps', '4', '--fused-decode', 'a.png'],
    ['--curve-steps', '4', '--fused-curves', '--fused-decode', 'a.png'],
])
def test_cli_argument_errors(argv, capsys):
  with mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'), pytest.raises(SystemExit) as e:
    evaluate.main(argv)
  assert e.value.code == 2
  err = capsys.readouterr().err
  assert ('--fused-curves' in err or '--curve-steps' in err), err


def test_cli_weights_of_another_curve_steps_fail_with_the_shape_message(tmp_path):
  cfg, ag = generic_agent(4)
  w = str(tmp_path / 'm.pt')
  torch.save(ag.state_dict(), w)
  paths = _write_inputs(tmp_path, [(12, 12)])
  with fake_curves(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    evaluate.main(['--weights', w, '--curve-steps', '4', '--out', str(tmp_path / 'o.npy')] + paths)
    with pytest.raises(RuntimeError, match='size mismatch'):
      evaluate.main(['--weights', w, '--curve-steps', '8', '--out', str(tmp_path / 'p.npy')] + paths)
  assert not os.path.exists(tmp_path / 'p.npy')


def test_train_cli_takes_curve_steps():
  assert train.parse_args(['--curve-steps', '4']).curve_steps == 4
  assert train.parse_args([]).curve_steps is None
  for bad in ('0', '17'):
    with pytest.raises(SystemExit):
      train.parse_args(['--curve-steps', bad])
