"""A run of expo_chain_bwd recomputes its interior activations (csrc/chain_steps_bwd_rc.hip): the run kernel loads the
head's dy and the x of the run's LOWEST step only, rebuilds the x of the steps above it with the forward bodies of
csrc/chain_steps.hip and runs the backward steps from those registers.  Nothing the entry point returns may change by a
bit, and tests/test_hip_chain_bwd_runs.py already holds the default path to the per-step kernels.  Here:

* the recomputation really runs (launch counts cannot show it): with every interior activation of every run replaced by
  a NaN-filled tensor, every grads[i] and dparams[i] is torch.equal to the clean call's -- and with
  EXPO_CHAIN_BWD_RECOMPUTE=0 in a child process the same call yields NaN, so this test can fail;
* EXPO_CHAIN_BWD_RECOMPUTE=0 against the default, byte for byte, on two lanes and on tiles;
* what is no run keeps its kernels: a single step between two curves, Tone / Color, a shape off the vector path.

The poisoned positions follow the recomputable table restated in tests/_chain_bwd_recompute_child.py: the output of a
filter outside it is still loaded and stays clean."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import _chain_bwd_recompute_child as rcc
from tests import _chain_plan_child as cp
from tests import test_hip_chain_bwd_runs as runs  # its child helpers, plan cases and per-step comparison

pytestmark = pytest.mark.gpu

SEQUENCES = {
    'metric': tuple(range(8)),           # [C] [BW] [Ct] [T] [S+, W, G, E]: the forwards of E, G, W are recomputed
    'run8': (0, 1, 2, 3, 8, 1, 0, 3),    # one run of 8: every filter of the table recomputed at least once, repeats
    's-plus-inside': (3, 3, 0),          # the forward of S+ inside a run, twice
    'acc-limit': (2, 2, 2, 2, 2),        # the LDS bound cuts the run after four steps
}
SHAPES = {
    'full': (3, 64, 64),
    'partial': (2, 50, 36),    # a partial last chunk, idle waves
    # 6.3 M values: a forward that rounded once where the per-step kernel rounds twice differs in one value of 2^14
    'large': (8, 512, 512),
}


def test_the_restated_run_collection():
  """(No GPU work: the positions the poisoning relies on.)"""
  assert rcc.runs_of(SEQUENCES['metric'], 'f16', 0) == [(0, 3)]
  assert rcc.runs_of(SEQUENCES['run8'], 'f16', 1) == [(0, 7)]
  assert rcc.runs_of(SEQUENCES['run8'], 'f32', 1) == [(4, 6), (0, 2)]  # S+ with mode 1 in fp32 is no step of a run
  assert rcc.runs_of(SEQUENCES['acc-limit'], 'f32', 0) == [(1, 4)]
  assert rcc.runs_of((4, 0, 4), 'f16', 0) == []
  assert rcc.poisoned_positions(SEQUENCES['metric'], 'f16', 0) == [1, 2, 3]
  assert rcc.poisoned_positions(SEQUENCES['s-plus-inside'], 'f32', 0) == [1, 2]


@functools.lru_cache(maxsize=1)  # (the two hsv_grad_mode cases of one (sequence, shape, type) follow each other)
def inputs(seq, shape, dt):
  ids = SEQUENCES[seq]
  n, h, w = SHAPES[shape]
  return cp.make_inputs(6100 + 7 * len(ids) + n, (n, h, w, 3), cp.NP_DT[dt], ids)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('dt', ['f16', 'f32'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('seq', sorted(SEQUENCES))
def test_poisoned_interior_activations_change_nothing(seq, shape, dt, mode, gpu_device):
  ids = SEQUENCES[seq]
  x, dy, params = inputs(seq, shape, dt)
  grads, dps, p_grads, p_dps, where = rcc.poisoned_call(ids, mode, x, dy, params, dt, gpu_device)
  # (S+ with hsv_grad_mode 1 in fp32 is no step of a run: (3, 3, 0) then has none, and nothing is poisoned)
  assert bool(where) == (not (seq == 's-plus-inside' and dt == 'f32' and mode == 1)), (seq, dt, mode, where)
  for i in range(len(ids)):
    assert torch.equal(p_grads[i].view(torch.uint8), grads[i].view(torch.uint8)), \
        'grads[%d] read a poisoned activation (acts %s)' % (i, where)
    assert torch.equal(p_dps[i].view(torch.int32), dps[i].view(torch.int32)), \
        'dparams[%d] read a poisoned activation (acts %s)' % (i, where)
    assert not bool(torch.isnan(grads[i]).any()) and not bool(torch.isnan(dps[i]).any()), 'the clean call, step %d' % i


def test_without_recomputation_the_poison_shows(gpu_device):
  """EXPO_CHAIN_BWD_RECOMPUTE=0 loads every activation, so the comparison above fails there: in every run a tensor
  differs from the clean call's.  The NaN itself survives only where the filter lets it (csrc/filter_math.h): the
  parameter gradients of Exposure and White balance are sums of dy * x; Gamma, S+ and Level pass x through fmaxf / fminf
  / a comparison first, which swallow a NaN, and no dx of the run table is a NaN for a NaN x (Exposure's and White
  balance's do not depend on x).  So: NaN dparams at every poisoned Exposure / White-balance step, a difference in
  every run."""
  cases = [[list(SEQUENCES[seq]), mode, 3, 64, 64, dt, 6200] for seq in sorted(SEQUENCES)
           for dt, mode in (('f16', 1), ('f32', 0))]
  out = runs.run_child('_chain_bwd_recompute_child.py', [json.dumps(cases)], {'EXPO_CHAIN_BWD_RECOMPUTE': '0'})
  got = json.loads(out.strip().splitlines()[-1])
  assert len(got) == len(cases)
  for (ids, mode, _, _, _, dt, _), (nan_grads, nan_dps, diff_grads, diff_dps) in zip(cases, got):
    where = rcc.poisoned_positions(ids, dt, mode)
    assert where and {i for i in where if ids[i] in (0, 2)} <= set(nan_dps), (ids, dt, mode, where, nan_dps)
    for lo, hi in rcc.runs_of(ids, dt, mode):
      assert set(range(lo, hi + 1)) & (set(diff_grads) | set(diff_dps)), (ids, dt, mode, (lo, hi), diff_grads, diff_dps)


@pytest.mark.parametrize('plan', sorted(runs.PLANS))
def test_knob_zero_reproduces_the_default_bytes(plan, gpu_device, tmp_path):
  outs = []
  for knob in (None, '0'):
    knobs = dict(runs.PLANS[plan])
    if knob:
      knobs['EXPO_CHAIN_BWD_RECOMPUTE'] = knob
    path = str(tmp_path / ('plan_%s.npz' % knob))
    runs.run_child('_chain_plan_child.py', [json.dumps(runs.PLAN_CASES), path], knobs)
    outs.append(np.load(path))
    assert json.loads(str(outs[-1]['env'])) == knobs
  recomputed, loaded = outs
  assert int(recomputed['c0_lanes']) == (2 if plan == 'two-lanes' else 1)
  assert len(recomputed['c2_chunks']) == (3 if plan == 'tiles' else 2), recomputed['c2_chunks']
  keys = sorted(k for k in recomputed.files if k != 'env')
  assert keys == sorted(k for k in loaded.files if k != 'env')
  assert any(k.endswith('grad_digest') for k in keys) and any('_dp' in k for k in keys)
  for k in keys:
    a, b = recomputed[k], loaded[k]
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), '%s: %s' % (plan, k)


OFF_RUN = [
    ((4, 0, 7, 3, 4), (3, 64, 64), 'f16'),           # single steps between curves, Tone and Color
    ((4, 0, 7, 3, 4), (2, 50, 36), 'f32'),
    (tuple(range(8)), (2, 33, 31), 'f16'),           # an odd fp16 pixel count: off the vector path, per-step launches
]


@pytest.mark.parametrize('ids,shape,dt', OFF_RUN)
def test_what_is_no_run_equals_the_per_step_calls(ids, shape, dt, gpu_device):
  x, dy, params = cp.make_inputs(6300, shape + (3,), cp.NP_DT[dt], ids)
  acts, grads, prm, dps = runs.run_chain(ids, 1, x, dy, params, gpu_device)
  runs.assert_equals_per_step_calls(ids, 1, acts, grads, prm, dps, '%s %s %s' % (ids, shape, dt))
