"""CPU: the host half of retouching straight from integer codes for any cfg.curve_steps --
evaluate.retouch_batch_raw(curves='fused') with a generic agent and the CLI's --fused-decode-curves -- against a CPU
stand-in of the new binding defined here by what include/exposure_hip.h promises: a pixel enters as float(table[code])
(the gather of tests/test_fused_decode_host.py), then the pass from tensors (the stand-in of
tests/test_curves_chain_host.py).  Everything else runs on the stand-ins of tests/test_fused_decode_host.py.  The GPU
counterpart is tests/test_hip_curves_codes.py."""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import evaluate
from exposure_amd.config import make_cfg
from tests import test_curves_chain_host as cch
from tests import test_fused_decode_host as fdh
from tests import test_taps16_host as t16
from tests.test_taps_host import agent, inputs

new_calls = []  # (number of images, L, code dtype, channels) of every call of the new binding's stand-in


def curves_ragged(ids, params48, curve_steps, xs, ys, tap_mask=0, taps=None):
  """tests/test_curves_chain_host.py's stand-in, with uint16 taps encoded by EXPO_TAP_U16's definition"""
  if taps is None or taps[0].dtype != torch.uint16:
    return cch._curves_ragged(ids, params48, curve_steps, xs, ys, tap_mask, taps)
  storage = [torch.empty(t.shape, dtype=xs[0].dtype) for t in taps]
  cch._curves_ragged(ids, params48, curve_steps, xs, ys, tap_mask, storage)
  for t, s in zip(taps, storage):
    for j in range(t.shape[0]):
      t16._put(t[j], s[j])


def fake_curves_codes(ids, params48, curve_steps, codes, tables, stride, ys, tap_mask=0, taps=None):
  new_calls.append((len(codes), curve_steps, codes[0].dtype, codes[0].shape[2]))
  fdh.calls.append(('pass', len(codes), codes[0].dtype, codes[0].shape[2]))
  assert ids.shape[0] == params48.shape[0] == len(codes) and ids.is_contiguous() and params48.is_contiguous()
  curves_ragged(ids, params48, curve_steps, fdh._gather(codes, tables, stride), ys, tap_mask, taps)


@contextlib.contextmanager
def stand_ins():
  with fdh.stand_ins(), mock.patch.multiple('exposure_amd._cabi', chain_fused_curves_fwd_ragged=curves_ragged,
                                            chain_fused_curves_fwd_ragged_codes=fake_curves_codes):
    yield


GROUPS = [(2, torch.uint8, 3), (2, torch.uint16, 3), (1, torch.uint8, 4), (1, torch.uint16, 1)]  # of fdh.mixed_raws


@pytest.mark.parametrize('L', [4, 16])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('code', ['u8', 'u16'])
def test_retouch_batch_raw_fused_curves_groups_order_and_results(code, dtype, L):
  cfg, ag = cch.generic_agent(L)
  raws = fdh.mixed_raws(5)
  n = len(raws)
  z, masks = inputs(cfg, n, 6)
  kw = dict(z=z, dropout_masks=masks, return_trace='full', intermediates=code, picture=code)
  with stand_ins():
    want = evaluate.retouch_batch(ag, evaluate.decode_images(raws, dtype, 'cpu'), proxy='device', curves='fused', **kw)
    del fdh.calls[:], new_calls[:], cch.calls[:]
    got = evaluate.retouch_batch_raw(ag, raws, dtype, 'cpu', curves='fused', **kw)
    made, new = list(fdh.calls), list(new_calls)
    bare = evaluate.retouch_batch_raw(ag, raws, dtype, 'cpu', outputs=False, curves='fused', **kw)
    plain = evaluate.retouch_batch_raw(ag, raws, dtype, 'cpu', z=z, dropout_masks=masks, curves='fused')
  # per (kind, channels) group, in order of first appearance: tables then proxy; after the one agent run, one pass each
  assert made == [(name,) + g for g in GROUPS for name in ('tables', 'proxy')] + [('pass',) + g for g in GROUPS]
  assert new == [(g[0], L) + g[1:] for g in GROUPS]
  assert len(got) == len(want) == 6
  for name, g, w in zip(('outputs', 'low', 'states', 'ops', 'intermediates', 'pictures'), got, want):
    fdh.same(g, w, name)
  assert sorted(got[3]) == ['abi_filter_ids', 'params24', 'params48', 'selected'] and got[3]['params48'].shape[2] == 48
  for (codes, _kind), o in zip(raws, got[0]):  # argument order, whatever the grouping
    assert tuple(o.shape) == (1, codes.shape[0], codes.shape[1], 3) and o.dtype == dtype
  assert bare[0] == [None] * n
  fdh.same(bare[1:], want[1:], 'outputs=False')
  assert len(plain) == 3
  fdh.same(plain[0], want[0], 'no taps')


def test_storage_intermediates_next_to_a_picture():
  cfg, ag = cch.generic_agent(4)
  raws = fdh.mixed_raws(9)[:3]
  z, masks = inputs(cfg, 3, 2)
  kw = dict(z=z, dropout_masks=masks, return_trace=True, intermediates='storage', picture='u8')
  with stand_ins():
    want = evaluate.retouch_batch(ag, evaluate.decode_images(raws, torch.float32, 'cpu'), proxy='device', curves='fused', **kw)
    got = evaluate.retouch_batch_raw(ag, raws, torch.float32, 'cpu', curves='fused', **kw)
  fdh.same(got, want, 'storage intermediates')


def test_default_curves_still_raises_before_any_binding_and_bad_values_raise():
  cfg, ag = cch.generic_agent(6)
  raws = fdh.mixed_raws(7)[:2]
  boom = mock.Mock(side_effect=AssertionError('called'))
  with stand_ins(), mock.patch.multiple('exposure_amd._cabi', decode_tables=boom, bilinear_resize_ragged_codes=boom,
                                        chain_fused_curves_fwd_ragged_codes=boom, chain_fused_fwd_ragged_codes=boom):
    with pytest.raises(ValueError, match='curve_steps'):
      evaluate.retouch_batch_raw(ag, raws, torch.float32, 'cpu')
    with pytest.raises(ValueError, match='curve_steps'):
      evaluate.retouch_batch_raw(ag, raws, torch.float32, 'cpu', curves='stepwise')
    for bad in ('both', True, None):
      with pytest.raises(ValueError, match='curves'):
        evaluate.retouch_batch_raw(ag, raws, torch.float32, 'cpu', curves=bad)
    masked = make_cfg()
    masked.masking = True
    masked.curve_steps = 6
    with pytest.raises(ValueError, match='masking'):
      evaluate.retouch_batch_raw(agent(masked), raws, torch.float32, 'cpu', curves='fused')
  assert not boom.called


def test_curves_has_no_effect_on_an_8_step_agent():
  cfg = make_cfg()
  ag = agent(cfg)
  raws = fdh.mixed_raws(5)
  z, masks = inputs(cfg, len(raws), 6)
  kw = dict(z=z, dropout_masks=masks, return_trace='full', intermediates='u8', picture='u8')
  with stand_ins():
    want = evaluate.retouch_batch_raw(ag, raws, torch.float32, 'cpu', **kw)
    del fdh.calls[:], new_calls[:]
    got = evaluate.retouch_batch_raw(ag, raws, torch.float32, 'cpu', curves='fused', **kw)
  assert new_calls == [] and [c for c in fdh.calls if c[0] == 'pass'] == [('pass',) + g for g in GROUPS]
  fdh.same(got, want, '8-step agent')
  assert sorted(got[3]) == ['abi_filter_ids', 'params24', 'selected']


def _run(argv):
  with stand_ins(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    return evaluate.main(argv)


@pytest.mark.parametrize('mode', [['--device-png', '--step-by-step', '--batch', '4'], ['--tiff16', '--step-by-step', '--batch', '3'],
                                  ['--device-png', '--batch', '1'], ['--batch', '4']])
def test_cli_fused_decode_curves_writes_the_same_files(tmp_path, mode):
  paths = fdh._write_files(tmp_path)
  runs = {}
  for name, extra in (('parent', ['--device-decode', '--device-proxy', '--fused-curves']), ('fused', ['--fused-decode-curves'])):
    out = str(tmp_path / name) + os.sep
    del new_calls[:]
    runs[name] = _run(['--seed', '3', '--dtype', 'f32', '--curve-steps', '4', '--out', out, *mode, *extra, *paths])
    assert bool(new_calls) == (name == 'fused') and all(c[1] == 4 for c in new_calls)
  assert len(runs['parent']) == len(runs['fused']) == len(paths)
  for a, b in zip(runs['parent'], runs['fused']):
    assert a['filters'] == b['filters'] and a['states'] == b['states'] and a['abi_filter_ids'] == b['abi_filter_ids']
    assert open(a['output'], 'rb').read() == open(b['output'], 'rb').read()
    assert sorted(a['png']) == sorted(b['png']) and sorted(a['tiff']) == sorted(b['tiff'])
    for kind in ('png', 'tiff'):
      for k in a[kind]:
        assert open(a[kind][k], 'rb').read() == open(b[kind][k], 'rb').read(), k
  assert sorted(os.listdir(str(tmp_path / 'parent'))) == sorted(os.listdir(str(tmp_path / 'fused')))


def test_cli_flag_composes_as_fused_decode_does(tmp_path):
  """--pictures-only passes outputs=False, and with 8-step curves the flag is --fused-decode"""
  paths = fdh._write_files(tmp_path)[:2]
  seen = []
  real = evaluate.retouch_batch_raw

  def spy(*a, **kw):
    seen.append((kw.get('outputs'), kw.get('curves')))
    return real(*a, **kw)

  with mock.patch.object(evaluate, 'retouch_batch_raw', spy):
    del new_calls[:]
    only = _run(['--fused-decode-curves', '--curve-steps', '16', '--tiff16', '--pictures-only', '--batch', '2', '--out',
                 str(tmp_path / 'o') + os.sep] + paths)
    assert [c[:2] for c in new_calls] == [(2, 16)]
    del new_calls[:]
    _run(['--fused-decode-curves', '--device-png', '--batch', '2', '--out', str(tmp_path / 'p') + os.sep] + paths)
    assert new_calls == []
  assert seen == [(False, 'fused'), (True, 'fused')]
  assert all(r['output'] is None and sorted(r['tiff']) == ['retouched'] for r in only)
  assert not [f for f in os.listdir(str(tmp_path / 'o')) if f.endswith('.npy')]


@pytest.mark.parametrize('flags', [['--stepwise'], ['--masking'], ['--show-input'], ['--curve-steps', '4', '--stepwise'],
                                   ['--curve-steps', '4', '--masking'], ['--curve-steps', '4', '--show-linear']])
def test_cli_refusals(tmp_path, flags, capsys):
  paths = fdh._write_files(tmp_path)[:1]
  with pytest.raises(SystemExit) as e:
    _run(['--fused-decode-curves'] + flags + paths)
  assert e.value.code == 2 and '--fused-decode-curves' in capsys.readouterr().err
