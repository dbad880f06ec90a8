"""CPU-only: the exports of the per-image dispatch for any cfg.curve_steps are in the header, the binding and the built
library, and validate their arguments before anything is enqueued (every call here is rejected or is the empty no-op, so
the fake device addresses are never touched); and, with the bindings mocked by the oracle (tests/_curve_dispatch_ref.py),
``Agent.curve_dispatch`` changes the launches the op-by-op step makes, not what it computes.  The GPU counterparts are
tests/test_hip_curve_dispatch.py and tests/test_hip_curve_dispatch_agent.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from exposure_amd.config import make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # a device address that is never dereferenced
NAMES = ('expo_filter_dispatch_curves_workspace_bytes', 'expo_filter_dispatch_curves_fwd', 'expo_filter_dispatch_curves_bwd',
         'expo_heads_regress_curves_fwd', 'expo_heads_regress_curves_bwd')


@pytest.fixture(scope='module')
def lib():
  return _cabi.load()


def test_exported_bound_and_version_stays_9(lib):
  assert lib.expo_version() == 9 == _cabi.EXPO_ABI_VERSION
  with open(os.path.join(ROOT, 'include', 'exposure_hip.h')) as f:
    header = f.read()
  for name in NAMES:
    assert name in _cabi.SIGNATURES and hasattr(lib, name), name
    assert '%s(' % name in header, name
  for fn in ('dispatch_curves_fwd', 'dispatch_curves_bwd', 'heads_regress_curves_fwd', 'heads_regress_curves_bwd'):
    assert callable(getattr(_cabi, fn))


def test_workspace_is_zero_for_bad_arguments_and_grows_with_the_step_count(lib):
  ws = lib.expo_filter_dispatch_curves_workspace_bytes
  f16, f32 = _cabi.EXPO_F16, _cabi.EXPO_F32
  for bad in ((0, 64, 64, f16, 8), (-1, 64, 64, f16, 8), (4, 0, 64, f16, 8), (4, 64, 0, f16, 8), (4, 64, 64, 7, 8),
              (4, 64, 64, f16, 0), (4, 64, 64, f16, 17), (4, 64, 64, f16, -3), (70000, 64, 64, f16, 8)):
    assert ws(*bad) == 0, bad
  sizes = [ws(64, 64, 64, f16, L) for L in range(1, 17)]
  assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
  # two curve blocks per 64x64 image, 3 (2 L + 1) record floats each, beside the light launches' 32-float records
  assert sizes[15] - sizes[0] == 64 * 2 * 3 * 2 * 15 * 4
  assert sizes[0] >= 64 * (32 + 2 * 9) * 4
  assert ws(64, 64, 64, f32, 16) >= sizes[15] and ws(64, 512, 512, f16, 16) > sizes[15]
  assert ws(64, 64, 64, f16, 16) >= lib.expo_workspace_bytes(64, 64, 64, f16)


def test_dispatch_argument_checks(lib):
  big = 1 << 24

  def fwd(steps=12, n=2, h=4, w=4, dtype=0, ws=FAKE, wsb=big, pen=FAKE, ids=FAKE):
    return lib.expo_filter_dispatch_curves_fwd(ids, FAKE, FAKE, FAKE, steps, pen, n, h, w, dtype, ws, wsb, None)

  def bwd(steps=12, n=2, h=4, w=4, dtype=0, ws=FAKE, wsb=big, mode=0, dparams=FAKE):
    return lib.expo_filter_dispatch_curves_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, dparams, FAKE, steps, n, h, w, dtype, mode, ws, wsb,
                                               None)

  for call in (fwd, bwd):
    for steps in (0, -1, 17, 1 << 20):
      assert call(steps=steps) == -1 and b'curve_steps' in lib.expo_last_error()
      assert call(steps=steps, n=0) == -1  # checked before the n == 0 early return
    assert call(ws=None, wsb=0) == -1 and b'workspace' in lib.expo_last_error()
    assert call(wsb=lib.expo_filter_dispatch_curves_workspace_bytes(2, 4, 4, 0, 12) - 1) == -1
    assert b'workspace' in lib.expo_last_error()
    assert call(ws=FAKE + 2) == -1 and b'aligned' in lib.expo_last_error()
    assert call(dtype=5) == -2 and call(n=-1) == -1 and call(h=0) == -1
    assert call(h=1 << 15, w=1 << 15, dtype=1) == -1 and b'2 GiB' in lib.expo_last_error()
    assert call(n=0) == 0 and call(n=0, ws=None, wsb=0) == 0
  assert fwd(ids=None) == -1 and b'null' in lib.expo_last_error()
  assert bwd(dparams=None) == -1 and b'null' in lib.expo_last_error()
  assert bwd(mode=2) == -1 and b'hsv_grad_mode' in lib.expo_last_error()


def test_heads_argument_checks(lib):
  rng = (ctypes.c_float * 9)(3.5, 1.1, 0.5, 2.0, 0.0, 0.9, 1.1, 0.0, 0.0)

  def heads(count, abi=None, widths=None, n=4, back=False, steps=16, sel=FAKE):
    m = max(count, 1)
    abi = abi or [0] * m
    widths = widths or [64] * m
    r = (ctypes.c_void_p * m)(*[FAKE + 0x1000 * i for i in range(m)])
    d = (ctypes.c_void_p * m)(*[FAKE + 0x100000 + 0x1000 * i for i in range(m)])
    wd, a = (ctypes.c_int * m)(*widths), (ctypes.c_int * m)(*abi)
    if back:
      return lib.expo_heads_regress_curves_bwd(r, d, wd, a, count, rng, sel, FAKE, steps, n, None)
    return lib.expo_heads_regress_curves_fwd(r, wd, a, count, rng, sel, FAKE, steps, n, None)

  for back in (False, True):
    assert heads(0, back=back) == -1 and heads(17, back=back) == -1
    for abi in ([0, 9], [-1, 0], [-2, 0]):
      assert heads(2, abi=abi, back=back) == -1 and b'filter_id' in lib.expo_last_error()
    for steps in (0, 17, -1):
      assert heads(2, steps=steps, back=back) == -1 and b'curve_steps' in lib.expo_last_error()
    assert heads(2, abi=[0, 7], widths=[1, 47], back=back) == -1  # a colour head has 48 parameters at 16 steps
    assert heads(2, abi=[4, 2], widths=[15, 3], back=back) == -1 and b'narrower' in lib.expo_last_error()
    assert heads(2, abi=[4, 7], widths=[5, 15], steps=5, sel=None, back=back) == -1 and b'null' in lib.expo_last_error()
    assert heads(2, n=-1, back=back) == -1
    assert heads(2, abi=[4, 7], widths=[5, 15], steps=5, n=0, back=back) == 0


def test_bindings_reject_before_the_library_is_asked():
  x = torch.zeros((2, 4, 4, 3))
  with pytest.raises(_cabi.ExposureHipError, match='no CPU fallback'):
    _cabi.dispatch_curves_fwd(torch.zeros(2, dtype=torch.int32), x, x.clone(), torch.zeros((2, 48)), 4)
  with pytest.raises(_cabi.ExposureHipError, match='no CPU fallback'):
    _cabi.dispatch_curves_bwd(torch.zeros(2, dtype=torch.int32), x, x, None, torch.zeros((2, 48)), torch.zeros((2, 48)), 4)
  with pytest.raises(_cabi.ExposureHipError):
    _cabi.heads_regress_curves_fwd([torch.zeros((2, 10))], (4,), (0,) * 9, torch.zeros(2, dtype=torch.int32),
                                   torch.zeros((2, 48)), 4)


# ---- the agent's op-by-op step under mocks ------------------------------------------------------------------------------
def agent_step(steps, switch, masking=False, high_res=True):
  from exposure_amd.agent import Agent
  from tests._curve_dispatch_ref import fake_hip_curves
  from tests.test_oracle_nets import make_batch
  torch.manual_seed(3)
  cfg = make_cfg()
  cfg.curve_steps = steps
  cfg.masking = masking
  agent = Agent(cfg)
  agent.curve_dispatch = switch
  n = 8
  fake_input, _real, states, z, masks, _alpha = make_batch(n, 3)
  # noise spread over (0, 1) so that the batch selects many different filters, the curve filters among them
  z = z.copy()
  z[:, 0] = (np.arange(n) + 0.5) / n
  t = torch.from_numpy
  hi = torch.rand((n, 12, 10, 3), generator=torch.Generator().manual_seed(5)) * 1.4 if high_res else None
  with fake_hip_curves() as calls:
    inp = (t(fake_input).clone().requires_grad_(True), t(z), t(states))
    outs, dbg, _ = agent(inp, 1, 0.3, high_res=hi, dropout_masks=[t(m) for m in masks])
    res = dict(out=outs[0], ids=dbg['selected_filter_ids'], dbg=dbg)
    if high_res:
      res['high'] = outs[2]
      loss = (outs[0] * 0.7).sum() + (outs[2] * 0.3).sum()
    else:
      res['penalty'] = outs[3]
      loss = (outs[0] * 0.7).sum() + outs[3].sum() * 5.0 + outs[2].sum()
    loss.backward()
  res['grads'] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in agent.named_parameters()}
  res['calls'] = dict(calls)
  return res


@pytest.mark.parametrize('steps', [4, 16])
@pytest.mark.parametrize('high_res', [False, True], ids=['train', 'high_res'])
def test_switch_changes_the_launches_not_the_values(steps, high_res):
  off = agent_step(steps, False, high_res=high_res)
  on = agent_step(steps, True, high_res=high_res)
  assert off['calls'] == dict(dispatch_fwd=0, dispatch_bwd=0, heads_fwd=0, heads_bwd=0)
  assert on['calls']['dispatch_fwd'] == (2 if high_res else 1) and on['calls']['dispatch_bwd'] >= 1
  assert torch.equal(on['ids'], off['ids'])
  assert {4, 7} <= set(on['dbg']['abi_filter_ids'].tolist()), 'the batch must select both curve filters'
  close = lambda a, b: float((a.detach().double() - b.detach().double()).abs().max()) <= 1e-6
  assert close(on['out'], off['out'])
  for key in ('high', 'penalty'):
    if key in on:
      assert close(on[key], off[key]), key
  assert close(on['dbg']['params48'], off['dbg']['params48'])
  assert torch.equal(on['dbg']['abi_filter_ids'], off['dbg']['abi_filter_ids'])
  assert torch.equal(on['dbg']['pdf_batch'], off['dbg']['pdf_batch'])
  live = 0
  for name, g in off['grads'].items():
    h = on['grads'][name]
    assert (g is None) == (h is None) or (g is None and float(h.abs().max()) == 0) or (h is None and float(g.abs().max()) == 0), name
    if g is not None and h is not None:
      assert close(h, g), name
      live += int(float(g.abs().max()) > 0)
  assert live >= 10


def test_masking_keeps_the_stack_path():
  res = agent_step(4, True, masking=True, high_res=False)
  assert res['calls'] == dict(dispatch_fwd=0, dispatch_bwd=0, heads_fwd=0, heads_bwd=0)
  assert 'params48' in res['dbg'] and 'packed_params' in res['dbg']


def test_switch_is_off_by_default_and_reaches_the_agent_through_gan():
  from exposure_amd.agent import Agent
  from exposure_amd.gan import GAN
  cfg = make_cfg()
  cfg.curve_steps = 4
  assert Agent(cfg).curve_dispatch is False
  assert GAN(cfg).generator.curve_dispatch is False
  assert GAN(cfg, curve_dispatch=True).generator.curve_dispatch is True
