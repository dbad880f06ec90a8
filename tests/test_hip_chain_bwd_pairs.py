"""The run kernels of expo_chain_bwd at every filter pair, every run length and the filters' clamp edges.

A run of element-wise backward steps is one launch of chain_steps_bwd_rc_kernel<T, MODE, IO, NS> (the default: it
recomputes the run's interior activations) or of chain_steps_bwd_kernel<T, MODE, IO, NS> (EXPO_CHAIN_BWD_RECOMPUTE=0):
56 instantiations each, and in fp32 -- where pack / unpack are bit casts -- the bodies of neighbouring steps meet in one
function, so whether the per-step kernels' bits hold depends on which filter follows which, at which run length.
tests/test_hip_chain_bwd_runs.py and tests/test_hip_chain_bwd_recompute.py reach 13 of the 25 ordered pairs of the run
table and the run lengths 2, 3, 4 and 8, on synthetic images only.  Here:

* a covering set of sequences (tests/_chain_bwd_pairs_child.py::COVERING) that puts all 25 pairs (16 in fp32 with
  hsv_grad_mode 1, where S+ is no step of a run) and every run length 2..8 inside runs, in each (storage type, mode):
  test_the_sequences_cover proves that from the restated run collection, without a GPU;
* on 2 x 256 x 256 (the vector path in both types; 393 216 values per tensor, so a rounding mixture that moves one
  value in 2^14 -- csrc/chain_steps.hip -- moves about 24; 3 x 64 x 64 would show about 2), with an edge block in
  image 0 (the filters' thresholds, their neighbours in the storage type, values beyond both ends, black / white /
  negative / grey / tied pixels, a Level step whose `lower` occurs in the image): every grads[i] and dparams[i] of
  expo_chain_bwd bit-equal to expo_filter_bwd step by step, and every activation of expo_chain_fwd bit-equal to
  expo_filter_fwd step by step -- in process (recompute, cached policy), and in one child process each with
  EXPO_CHAIN_BWD_RECOMPUTE=0, with EXPO_STREAM_MIN_BYTES=1 (the IoStream instantiations) and with both.  Nothing a
  caller can observe tells which cache policy ran: the knob's effect is host_common.h's `g.stream` and is taken on
  trust here, as in test_hip_filters.py::test_streaming_policy_equals_cached_policy;
* every covering sequence is really one launch (kernel nodes of a captured call) and really recomputes (poisoned
  interior activations change nothing);
* the float64 oracle on the same inputs, step by step on the GPU's own acts[i] and grads[i + 1] -- bit-equality to the
  per-step kernels proves nothing where both are wrong -- with fixed parameters under which no step's gradient dies;
* fp16 saturation through the recompute path: interior activations at +-65504, against the loading kernels and the
  per-step calls.  (Inf and NaN inputs are out of scope: the project defines no result for them.)"""
import functools
import json
import tempfile

import numpy as np
import pytest
import torch

from tests import _chain_bwd_pairs_child as pc
from tests import _chain_bwd_recompute_child as rcc
from tests import _chain_plan_child as cp
from tests import test_hip_chain_bwd_runs as runs  # run_chain, assert_equals_per_step_calls, run_child
from tests._tol import assert_image_close, assert_param_grad_close

gpu = pytest.mark.gpu

SEQS = sorted(pc.COVERING)
CELL_IDS = ['%s-mode%d' % c for c in pc.CELLS]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the covering set covers (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def full_coverage(dt, mode):
  ids = pc.fusable_ids(dt, mode)
  return {(a, b) for a in ids for b in ids}, set(range(2, 9))


@pytest.mark.parametrize('dt,mode', pc.CELLS, ids=CELL_IDS)
def test_the_sequences_cover(dt, mode):
  """Per (storage type, mode): the adjacent pairs inside runs are the full product of the ids fusable there, and the run
  lengths are 2..8."""
  assert len(full_coverage(dt, mode)[0]) == (16 if (dt, mode) == ('f32', 1) else 25)
  assert pc.coverage(pc.COVERING.values(), dt, mode) == full_coverage(dt, mode)


@pytest.mark.parametrize('seq', SEQS)
def test_no_sequence_is_redundant(seq):
  """Without any one of the sequences some cell loses a pair or a run length."""
  rest = [v for k, v in pc.COVERING.items() if k != seq]
  assert any(pc.coverage(rest, dt, mode) != full_coverage(dt, mode) for dt, mode in pc.CELLS)


def test_each_sequence_is_one_run_where_the_issue_says_so():
  """(No GPU.)  Whole sequences as one run: all of them in fp16 and in fp32 mode 0, the S+-free ones in fp32 mode 1; the
  accumulator floats stay within the 48 a run may hold."""
  for seq, ids in pc.COVERING.items():
    assert sum(rcc.RUN_ACC_FLOATS[f] for f in ids) <= 48, seq
    for dt, mode in pc.CELLS:
      whole = rcc.runs_of(ids, dt, mode) == [(0, len(ids) - 1)]
      assert whole == (3 not in ids or (dt, mode) != ('f32', 1)), (seq, dt, mode)


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit-equality with the per-step kernels, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)  # (the cases of one (sequence, type, parameters) follow each other)
def equal_inputs(seq, dt, prm):
  return pc.equal_inputs(seq, dt, prm)


@gpu
@pytest.mark.parametrize('prm', ['fixed', 'drawn'])
@pytest.mark.parametrize('dt,mode', pc.CELLS, ids=CELL_IDS)
@pytest.mark.parametrize('seq', SEQS)
def test_chain_equals_per_step_calls(seq, dt, mode, prm, gpu_device):
  """In process: the default configuration (recompute, cached policy at this size)."""
  ids = pc.COVERING[seq]
  x, dy, params = equal_inputs(seq, dt, prm)
  acts, grads, tp, dps = runs.run_chain(ids, mode, x, dy, params, gpu_device)
  what = '%s %s mode %d %s' % (seq, dt, mode, prm)
  runs.assert_equals_per_step_calls(ids, mode, acts, grads, tp, dps, what)
  assert pc.differing_activations(ids, acts, tp) == [], what + ': expo_chain_fwd differs from expo_filter_fwd'


CONFIGS = {
    'load': {'EXPO_CHAIN_BWD_RECOMPUTE': '0'},                                 # chain_steps_bwd_kernel, lengths 5..7 too
    'stream': {'EXPO_STREAM_MIN_BYTES': '1'},                                  # the IoStream instantiations
    'load-stream': {'EXPO_CHAIN_BWD_RECOMPUTE': '0', 'EXPO_STREAM_MIN_BYTES': '1'},
}


@functools.lru_cache(maxsize=None)
def child_results(config):
  """One child process per configuration runs every case (tests/_chain_bwd_pairs_child.py) and is shared by the tests
  that read its results."""
  with tempfile.TemporaryDirectory() as tmp:
    path = '%s/%s.npz' % (tmp, config)
    runs.run_child('_chain_bwd_pairs_child.py', [path], CONFIGS[config])
    with np.load(path) as f:
      return {k: f[k] for k in f.files}


@gpu
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_chain_equals_per_step_calls_under_the_knobs(config, gpu_device):
  got = child_results(config)
  env = json.loads(str(got['env']))
  assert {k: env.get(k) for k in CONFIGS[config]} == CONFIGS[config], env
  equal = json.loads(str(got['equal']))
  assert len(equal) == len(pc.EQUAL_CASES) == 11 * 4 * 2
  differing = {'%s %s mode %d %s' % case: bad for case, bad in zip(pc.EQUAL_CASES, equal) if bad}
  assert not differing, differing
  for k in range(len(pc.SATURATION_CASES)):
    assert json.loads(str(got['s%d_bad' % k])) == [], pc.SATURATION_CASES[k]


@gpu
def test_every_covering_sequence_is_one_launch(gpu_device):
  """3 x 64 x 64, both storage types (mode 0): the run and the finish.  A silent fall-back to per-step launches would
  pass every comparison above."""
  from tests import _chain_bwd_runs_child as rc
  got = [rc.backward_kernel_nodes(*case) for case in pc.NODE_CASES]
  assert got == [1 + 1] * len(pc.NODE_CASES), list(zip(pc.NODE_CASES, got))


@gpu
@pytest.mark.parametrize('dt,mode', pc.CELLS, ids=CELL_IDS)
@pytest.mark.parametrize('seq', SEQS)
def test_poisoned_interior_activations_change_nothing(seq, dt, mode, gpu_device):
  """The recomputation really runs on these sequences: with every interior activation of every run a NaN-filled tensor
  nothing the call returns changes by a bit (rcc.poisoned_call; with EXPO_CHAIN_BWD_RECOMPUTE=0 this fails)."""
  ids = pc.COVERING[seq]
  x, dy, params = pc.make_inputs(7400, (3, 64, 64, 3), dt, ids)
  grads, dps, p_grads, p_dps, where = rcc.poisoned_call(ids, mode, x, dy, params, dt, gpu_device)
  # (S+ with hsv_grad_mode 1 in fp32 is no step of a run: (1, 3) then has none, and nothing is poisoned)
  assert bool(where) == ((seq, dt, mode) != ('len2', 'f32', 1)), (seq, dt, mode, where)
  if 3 not in ids or (dt, mode) != ('f32', 1):
    assert where == list(range(1, len(ids)))
  for i in range(len(ids)):
    assert torch.equal(p_grads[i].view(torch.uint8), grads[i].view(torch.uint8)), \
        'grads[%d] read a poisoned activation (acts %s)' % (i, where)
    assert torch.equal(p_dps[i].view(torch.int32), dps[i].view(torch.int32)), \
        'dparams[%d] read a poisoned activation (acts %s)' % (i, where)
    assert not bool(torch.isnan(grads[i]).any()) and not bool(torch.isnan(dps[i]).any()), 'the clean call, step %d' % i


# ---------------------------------------------------------------------------------------------------------------------
# 3. the float64 oracle on the same inputs
# ---------------------------------------------------------------------------------------------------------------------
ORACLE_SHAPE = (2, 48, 64, 3)


@gpu
@pytest.mark.parametrize('dt,mode', pc.CELLS, ids=CELL_IDS)
@pytest.mark.parametrize('seq', SEQS)
def test_every_step_matches_the_float64_oracle(seq, dt, mode, gpu_device):
  """Each step's oracle input is the GPU's own acts[i] and grads[i + 1] (test_hip_filters.py::
  test_chain_matches_stepwise_oracle), so the bounds stay per step: assert_image_close on y and dx, assert_param_grad_close
  on dparams -- the project's bounds unchanged; no gradient of the edge block needs the relative form of
  test_out_of_range_inputs (S+ with hsv_grad_mode 1 in fp32, with its 1 / rng and 1 / v factors, included).

  Liveness, asserted on the ORACLE's outputs: in every step at least a quarter of dx is non-zero and no parameter
  gradient is zero -- the parameters are fixed (pc.FIXED) so that no step clips the gradient away."""
  from oracle import filters_np as fnp
  from tests.test_hip_filters import grad_abs
  ids = pc.COVERING[seq]
  np_dt = cp.NP_DT[dt]
  x, dy, params = pc.make_inputs(7200, ORACLE_SHAPE, dt, ids)
  acts, grads, _, dps = runs.run_chain(ids, mode, x, dy, params, gpu_device)
  for i, fid in enumerate(ids):
    what = '%s %s mode %d step %d (filter %d)' % (seq, dt, mode, i, fid)
    xin, gin = acts[i].cpu().numpy(), grads[i + 1].cpu().numpy()
    x64, g64, p64 = xin.astype(np.float64), gin.astype(np.float64), params[i].astype(np.float64)
    ry = fnp.process_packed(fid, x64, p64)
    rdx, rdp = fnp.backward_packed(fid, x64, p64, g64, hsv_grad_mode=mode)
    assert np.isfinite(ry).all() and np.isfinite(rdx).all() and np.isfinite(rdp).all(), what
    assert np.count_nonzero(rdx) >= rdx.size / 4, '%s: the reference dx is dead' % what
    assert (rdp != 0).all(), '%s: a reference parameter gradient is zero' % what
    y, dx, dp = acts[i + 1].float().cpu().numpy(), grads[i].float().cpu().numpy(), dps[i].cpu().numpy()
    assert np.isfinite(y).all() and np.isfinite(dx).all() and np.isfinite(dp).all(), what
    assert_image_close(y, ry, np_dt, 'y ' + what)
    assert_image_close(dx, rdx, np_dt, 'dx ' + what)
    assert_param_grad_close(dp, rdp, grad_abs(fid, xin, gin, params[i]), 'dparams ' + what)


# ---------------------------------------------------------------------------------------------------------------------
# 4. fp16 saturation through the recompute path
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('seq,mode', pc.SATURATION_CASES)
def test_saturating_activations_through_the_recompute_path(seq, mode, gpu_device):
  """EV = +3.5 on an image that holds +-60000, 65504 and 3000: the interior activations of the run saturate, and the
  recompute kernel must reproduce the forward's MODE.FP16_OVFL store bit for bit.  The default call against the per-step
  calls and against the EXPO_CHAIN_BWD_RECOMPUTE=0 child's call (which itself equals its per-step calls:
  test_chain_equals_per_step_calls_under_the_knobs); everything finite, the saturated values exactly +-65504.  Inf and
  NaN inputs are out of scope."""
  ids = pc.SATURATION[seq]
  assert rcc.runs_of(ids, 'f16', mode) == [(0, len(ids) - 1)]
  mine, bad = pc.saturation_tensors(seq, mode, gpu_device)
  assert bad == [], bad
  theirs = child_results('load')
  k = pc.SATURATION_CASES.index((seq, mode))
  for name, a in mine.items():
    b = theirs['s%d_%s' % (k, name)]
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), \
        '%s differs from the EXPO_CHAIN_BWD_RECOMPUTE=0 call' % name
    assert np.isfinite(a.astype(np.float64)).all(), name
  # the first Exposure step: whatever 2^3.5 x carries beyond fp16's range is +-65504 -- and the run's interior holds it
  x, _, _ = pc.saturation_inputs(seq)
  over = np.abs(x.astype(np.float64)) * 2.0**3.5 >= 65536.0
  assert over.sum() >= 1000
  y = mine['act1'].astype(np.float64)
  assert (y[over] == np.sign(x.astype(np.float64)[over]) * 65504.0).all()
  for i in range(1, len(ids)):  # an interior activation of the run (the output of step i - 1, i - 1 below the head)
    assert (np.abs(mine['act%d' % i].astype(np.float64)) == 65504.0).any(), 'acts[%d] holds no saturated value' % i
