"""The runs of expo_chain_bwd whose filter sequence csrc/chain_steps_bwd_seq.hip was compiled for.

The reference ships one filter order, so the run a chain call of its configuration collects is [S+, W, G, E] from the
head down.  For the (sequence, storage type, hsv_grad_mode) entries of that unit's table EXPO_RUN_SEQUENCES -- restated
in tests/_chain_bwd_seq_child.py::TABLE -- such a run is one launch of chain_steps_bwd_seq_kernel<T, MODE, IO, 3, 2, 1, 0>
instead of chain_steps_bwd_rc_kernel<T, MODE, IO, 4>: straight-line code, accumulators in registers.  Nothing the entry
point returns may change by a bit, and the launch counts stay; only expo_chain_bwd_seq_launches() tells which ran.

For every entry of the table, in both cache policies (EXPO_STREAM_MIN_BYTES=1 in a child selects the IoStream kernels):

* expo_chain_bwd against expo_filter_bwd step by step on the chain's own inputs, torch.equal on the bytes of every
  grads[i] and dparams[i]: 3 x 64 x 64 (whole wave chunks), 2 x 50 x 36 (a partial last chunk, idle waves at the
  barriers), 2 x 256 x 256 with the edge block of tests/test_hip_chain_bwd_pairs.py (thresholds, -0, subnormals, values
  beyond both ends); the fp16 saturation image of that test (EV +3.5 on +-60000, 65504, 3000);
* the same calls with EXPO_CHAIN_BWD_SEQ=0 (today's kernels) and with EXPO_CHAIN_BWD_RECOMPUTE=0 (the loading kernels)
  in children, digest for digest, on one lane and on two (27 x 512 x 512, the metric order);
* ping-pong gradient buffers against distinct ones;
* a thread that walks two groups with the prefetch live (EXPO_BWD_GROUPS_PER_THREAD=4 at 16 x 512 x 512);
* poisoned interior activations change nothing;
* the counter rises by one per lane for a run of the table and stays put for a run outside it, with
  EXPO_CHAIN_BWD_SEQ=0 and with EXPO_CHAIN_BWD_RECOMPUTE=0;
* the kernel nodes of a captured expo_chain_bwd are today's.

(The 'large' and 'tall' cases of tests/test_hip_chain_bwd_runs.py run the metric order through the default path: they
cover 8 x 512 x 512 and 1 x 1536 x 1536 with this kernel without new code.)"""
import functools
import json
import tempfile

import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from tests import _chain_bwd_recompute_child as rcc
from tests import _chain_bwd_runs_child as rc
from tests import _chain_bwd_seq_child as sc
from tests import _chain_plan_child as cp
from tests import test_hip_chain_bwd_runs as runs  # run_child

pytestmark = pytest.mark.gpu

CELL_IDS = ['%s-mode%d' % c for c in sc.CELLS]
ALL = sorted(sc.CASES['all'])
IN_TABLE = [name for name in ALL if not name.startswith('outside')]

CONFIGS = {
    'stream': ('all', {'EXPO_STREAM_MIN_BYTES': '1'}),                               # the IoStream instantiations
    'off': ('all', {'EXPO_CHAIN_BWD_SEQ': '0'}),                                     # today's kernels
    'off-stream': ('all', {'EXPO_CHAIN_BWD_SEQ': '0', 'EXPO_STREAM_MIN_BYTES': '1'}),
    'load': ('all', {'EXPO_CHAIN_BWD_RECOMPUTE': '0'}),                              # the loading kernels
    'groups': ('groups', {'EXPO_BWD_GROUPS_PER_THREAD': '4'}),
    'groups-off': ('groups', {'EXPO_BWD_GROUPS_PER_THREAD': '4', 'EXPO_CHAIN_BWD_SEQ': '0'}),
}


def lanes_of(case):
  _, _, shape, dt, _, _ = case
  return _cabi.chain_plan(*shape, _cabi.EXPO_F16 if dt == 'f16' else _cabi.EXPO_F32)[1]


@functools.lru_cache(maxsize=None)
def here(name):
  """One case in this process: the default configuration (the compiled sequence, the cached policy at these sizes)."""
  return sc.run_case(sc.CASES['all'][name], torch.device('cuda:0'))


@functools.lru_cache(maxsize=None)
def child(config):
  """One child process per configuration runs every case and is shared by the tests that read its results."""
  which, knobs = CONFIGS[config]
  with tempfile.TemporaryDirectory() as tmp:
    path = '%s/%s.npz' % (tmp, config)
    runs.run_child('_chain_bwd_seq_child.py', [path, which], knobs)
    with np.load(path) as f:
      got = {k: f[k] for k in f.files}
  env = json.loads(str(got['env']))
  assert {k: env.get(k) for k in knobs} == knobs, env
  return got


def test_the_table_is_the_metric_orders_run():
  """(No GPU work.)  Every entry is the run the metric order's backward ends in, in a cell where S+ is a step of runs."""
  for (dt, mode), seqs in sc.TABLE.items():
    for seq in seqs:
      assert tuple(reversed(seq)) == sc.RUN == sc.METRIC[:4]
      assert rcc.runs_of(sc.RUN, dt, mode) == [(0, 3)] and rcc.runs_of(sc.METRIC, dt, mode) == [(0, 3)]
  assert rcc.runs_of(sc.RUN8, 'f16', 0) == [(0, 7)]
  assert _cabi.chain_plan(*sc.TWO_LANES, _cabi.EXPO_F16)[1] == 2


@pytest.mark.parametrize('name', ALL)
def test_chain_equals_per_step_calls(name, gpu_device):
  """In process.  The counter: one launch per lane for a run of the table, none for the run of eight."""
  bad, rose, _ = here(name)
  assert bad == [], (name, bad)
  assert rose == (lanes_of(sc.CASES['all'][name]) if name in IN_TABLE else 0), (name, rose)


@pytest.mark.parametrize('config', ['stream', 'off', 'off-stream', 'load'])
def test_chain_equals_per_step_calls_under_the_knobs(config, gpu_device):
  """Each child against the per-step calls made in it, and its counter: the streaming policy runs the compiled
  sequences, EXPO_CHAIN_BWD_SEQ=0 and EXPO_CHAIN_BWD_RECOMPUTE=0 run none."""
  got = child(config)
  for name in ALL:
    assert json.loads(str(got[name + '_bad'])) == [], (config, name)
    want = lanes_of(sc.CASES['all'][name]) if config == 'stream' and name in IN_TABLE else 0
    assert int(got[name + '_seq']) == want, (config, name, int(got[name + '_seq']))


@pytest.mark.parametrize('config', ['off', 'load'])
@pytest.mark.parametrize('name', ALL)
def test_the_bytes_are_todays(name, config, gpu_device):
  """Digest for digest against the same call through chain_steps_bwd_rc_kernel ('off') and through
  chain_steps_bwd_kernel ('load'): one lane, two lanes, the edge block, the saturating image."""
  mine, theirs = here(name)[2], child(config)[name + '_digest']
  assert mine.shape == theirs.shape and mine.tobytes() == theirs.tobytes(), (name, config)


@pytest.mark.parametrize('name', ALL)
def test_the_streaming_bytes_are_todays(name, gpu_device):
  mine, theirs = child('stream')[name + '_digest'], child('off-stream')[name + '_digest']
  assert mine.shape == theirs.shape and mine.tobytes() == theirs.tobytes(), name
  assert mine.tobytes() == here(name)[2].tobytes(), name  # (and the cached policy's)


def test_two_groups_per_thread_with_the_prefetch_live(gpu_device):
  """16 x 512 x 512 fp16 at four groups per thread: 64 blocks per image, every thread walks two groups, so the next
  group's pair is loaded while the current group's steps run and the accumulators live across both."""
  got, off = child('groups'), child('groups-off')
  for name in sorted(sc.CASES['groups']):
    assert json.loads(str(got[name + '_bad'])) == [], name
    assert int(got[name + '_seq']) == lanes_of(sc.CASES['groups'][name]) and int(off[name + '_seq']) == 0, name
    assert got[name + '_digest'].tobytes() == off[name + '_digest'].tobytes(), name


@pytest.mark.parametrize('dt,mode', sc.CELLS, ids=CELL_IDS)
def test_poisoned_interior_activations_change_nothing(dt, mode, gpu_device):
  """The kernel reads the run's lowest activation only: with acts[1..3] NaN-filled tensors nothing changes by a bit."""
  x, dy, params = cp.make_inputs(9400, (3, 64, 64, 3), cp.NP_DT[dt], sc.RUN)
  before = _cabi.chain_bwd_seq_launches()
  grads, dps, p_grads, p_dps, where = rcc.poisoned_call(sc.RUN, mode, x, dy, params, dt, gpu_device)
  assert _cabi.chain_bwd_seq_launches() - before == 2 and where == [1, 2, 3]
  for i in range(len(sc.RUN)):
    assert torch.equal(p_grads[i].view(torch.uint8), grads[i].view(torch.uint8)), 'grads[%d]' % i
    assert torch.equal(p_dps[i].view(torch.int32), dps[i].view(torch.int32)), 'dparams[%d]' % i
    assert not bool(torch.isnan(grads[i]).any()) and not bool(torch.isnan(dps[i]).any()), 'the clean call, step %d' % i


def test_the_kernel_nodes_are_todays(gpu_device):
  """A captured expo_chain_bwd: one launch per run either way."""
  got = [rc.backward_kernel_nodes(*case) for case in sc.NODE_CASES]
  assert got == sc.NODES_TODAY, got
  assert list(child('off')['nodes']) == sc.NODES_TODAY
