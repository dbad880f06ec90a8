"""expo_chain_bwd runs consecutive element-wise steps of a chunk in ONE launch (csrc/chain_steps_bwd.hip): a group of
the run head's dy is loaded once, every step's dx is rounded to the storage type, stored to its grads[i] and carried on
in registers.  Tone / Color, a step without a dx and a shape off the vector path keep their per-step kernels -- and so
do Contrast (5) and WNB (6), and S+ with hsv_grad_mode 1 in fp32: their fused bodies did not give the per-step kernels'
bits in the comparisons below, so the library's static run table holds ids 0, 1, 2, 3, 8 only.  The
metric order's backward is therefore [C] [BW] [Ct] [T] [S+, W, G, E]: 5 launches and the finish, where all seven
element-wise ids in one table would give [C] [BW, Ct] [T] [S+, W, G, E], 4 and the finish.  Nothing the entry point
returns may change by a bit:

* expo_chain_bwd against expo_filter_bwd step by step, each step fed the chain's own inputs: torch.equal on every
  grads[i] (distinct buffers) and every dparams[i] -- both storage types, both values of hsv_grad_mode, sequences and
  shapes listed below;
* a thread that walks two groups with the prefetch live (EXPO_BWD_GROUPS_PER_THREAD=4 in a child process);
* ping-pong gradient buffers (two buffers, as bench.py builds them) against distinct ones;
* grads[0] = NULL: all dparams equal the full call's;
* EXPO_CHAIN_FUSE_BWD_STEPS=1 (one kernel per step) against the default, byte for byte, on two lanes and on tiles.

That the fused kernel really ran (the per-step launches are bit-identical by contract and would pass all of the above) is
pinned by the number of kernel nodes of a captured expo_chain_bwd (tests/_chain_bwd_runs_child.py)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from tests import _chain_bwd_runs_child as rc
from tests import _chain_plan_child as cp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_DT_OF = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32}

METRIC = tuple(range(8))  # backward: [C] [BW] [Ct] [T] [S+, W, G, E]
SEQUENCES = {
    'metric': METRIC,
    'all-seven': (0, 1, 2, 3, 5, 6, 8, 0),      # every element-wise id, a repeat: [E, L] [BW] [Ct] [S+, W, G, E]
    'run8': (0, 1, 2, 3, 8, 1, 0, 3),           # one run of 8 with repeats and Level (44 accumulator floats of 48)
    'nine': (2, 0, 3, 8, 1, 1, 0, 3, 0),        # nine steps of the run table: a run of 8 plus a single (step 0)
    'cut': (4, 3, 7, 5, 6, 4),                  # runs cut by curve steps, an S+ alone between two curves
    'acc-limit': (2, 2, 2, 2, 2),               # 5 x 12 accumulator floats: the LDS bound cuts the run after four
}
SHAPES = {
    'full': (3, 64, 64),       # whole 3 KiB wave chunks in both storage types
    'partial': (2, 50, 36),    # a partial last chunk, idle waves at the reductions' barriers
    'odd': (2, 33, 31),        # fp16: off the vector path, per-step launches
    # 6.3 M values: a step whose conversion to fp16 rounded once where the per-step kernel rounds twice differs in one
    # value of 2^14 (csrc/chain_steps.hip) -- none at all in a small image
    'large': (8, 512, 512),
    # 294 912 groups in fp16 and 589 824 in fp32, above the 262 144 that 1024 blocks cover: threads walk 2 or 3 groups
    'tall': (1, 1536, 1536),
}


@functools.lru_cache(maxsize=1)  # (the two hsv_grad_mode cases of one (sequence, shape, type) follow each other)
def inputs(seq, shape, dt):
  ids = SEQUENCES[seq]
  n, h, w = SHAPES[shape]
  return cp.make_inputs(5100 + 7 * len(ids) + n, (n, h, w, 3), cp.NP_DT[dt], ids)


def run_chain(ids, mode, x, dy, params, dev, pingpong=False, null_dx=False):
  acts = [torch.from_numpy(x).to(dev)] + [torch.empty(x.shape, dtype=TORCH_DT_OF[x.dtype], device=dev) for _ in ids]
  prm = [torch.from_numpy(p).to(dev) for p in params]
  dps = [torch.full_like(p, float('nan')) for p in prm]
  gy = torch.from_numpy(dy).to(dev)
  if pingpong:
    # bench.py: two buffers; grads[steps] = dy, grads[i] alternate so that step i never writes what it reads
    buf = [torch.full_like(gy, float('nan')), torch.full_like(gy, float('nan'))]
    grads = [buf[i & 1] for i in range(len(ids))] + [gy]
  else:
    grads = [torch.full_like(gy, float('nan')) for _ in ids] + [gy]
  _cabi.chain_fwd(list(ids), acts, prm)
  if null_dx:
    cp.chain_bwd_without_dx(list(ids), acts, grads, prm, dps, mode)
  else:
    _cabi.chain_bwd(list(ids), acts, grads, prm, dps, hsv_grad_mode=mode)
  torch.cuda.synchronize()
  return acts, grads, prm, dps


def assert_equals_per_step_calls(ids, mode, acts, grads, prm, dps, what):
  """Every backward step of the chain against expo_filter_bwd fed the chain's own inputs of that step."""
  ref = torch.empty_like(acts[0])
  for i in reversed(range(len(ids))):
    fid = ids[i]
    dp = torch.full_like(prm[i], float('nan'))
    ref.fill_(float('nan'))
    _cabi.filter_bwd(fid, acts[i], grads[i + 1], ref, prm[i], dp, mode)
    assert torch.equal(ref.view(torch.uint8), grads[i].view(torch.uint8)), \
        '%s: grads[%d] (filter %d) differs from expo_filter_bwd' % (what, i, fid)
    assert torch.equal(dp.view(torch.int32), dps[i].view(torch.int32)), \
        '%s: dparams[%d] (filter %d) differ from expo_filter_bwd' % (what, i, fid)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('dt', ['f16', 'f32'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('seq', sorted(SEQUENCES))
def test_chain_bwd_equals_per_step_calls(seq, shape, dt, mode, gpu_device):
  ids = SEQUENCES[seq]
  x, dy, params = inputs(seq, shape, dt)
  acts, grads, prm, dps = run_chain(ids, mode, x, dy, params, gpu_device)
  assert_equals_per_step_calls(ids, mode, acts, grads, prm, dps, '%s %s %s mode %d' % (seq, shape, dt, mode))


@pytest.mark.parametrize('dt', ['f16', 'f32'])
@pytest.mark.parametrize('seq', ['metric', 'run8', 'nine'])
def test_pingpong_grads_equal_distinct_buffers(seq, dt, gpu_device):
  """The run's input grads[head + 1] is also the buffer of grads[head - 1]."""
  ids = SEQUENCES[seq]
  x, dy, params = cp.make_inputs(5300, (5, 64, 96, 3), cp.NP_DT[dt], ids)
  _, grads, _, dps = run_chain(ids, 0, x, dy, params, gpu_device)
  _, pp, _, pp_dps = run_chain(ids, 0, x, dy, params, gpu_device, pingpong=True)
  assert pp[0] is not pp[1] and pp[0] is pp[2]
  assert torch.equal(pp[0].view(torch.uint8), grads[0].view(torch.uint8)), 'grads[0]'
  assert torch.equal(pp[1].view(torch.uint8), grads[1].view(torch.uint8)), 'grads[1]'
  for i in range(len(ids)):
    assert torch.equal(pp_dps[i].view(torch.int32), dps[i].view(torch.int32)), 'dparams[%d]' % i


@pytest.mark.parametrize('dt', ['f16', 'f32'])
@pytest.mark.parametrize('seq', ['metric', 'run8', 'all-seven'])
def test_without_dx_all_dparams_equal_the_full_calls(seq, dt, gpu_device):
  """grads[0] = NULL: step 0 leaves its run and keeps its HAS_DX = false kernel (the node count below shows the launch)."""
  ids = SEQUENCES[seq]
  x, dy, params = cp.make_inputs(5400, (3, 64, 64, 3), cp.NP_DT[dt], ids)
  _, grads, _, dps = run_chain(ids, 1, x, dy, params, gpu_device)
  _, g2, _, dps2 = run_chain(ids, 1, x, dy, params, gpu_device, null_dx=True)
  for i in range(len(ids)):
    assert torch.equal(dps2[i].view(torch.int32), dps[i].view(torch.int32)), 'dparams[%d]' % i
  for i in range(1, len(ids)):
    assert torch.equal(g2[i].view(torch.uint8), grads[i].view(torch.uint8)), 'grads[%d]' % i
  assert bool(torch.isnan(g2[0]).all()), 'grads[0] was written'


# ---------------------------------------------------------------------------------------------------------------------
# knobs that are read once per process: child processes
# ---------------------------------------------------------------------------------------------------------------------
def child_env(knobs):
  env = {k: v for k, v in os.environ.items() if not k.startswith('EXPO_CHAIN_') and k != 'EXPO_BWD_GROUPS_PER_THREAD'}
  env.update(knobs)
  return env


def run_child(script, args, knobs):
  flags = ['-s'] if sys.flags.no_user_site else []
  proc = subprocess.run([sys.executable] + flags + [os.path.join(ROOT, 'tests', script)] + args, env=child_env(knobs),
                        cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert proc.returncode == 0, 'child (%s) exited with %d:\n%s' % (knobs, proc.returncode, proc.stderr[-4000:])
  return proc.stdout


def test_two_groups_per_thread_with_the_prefetch_live(gpu_device):
  """16 x 512 x 512 fp16 at four groups per thread: 64 blocks per image, every thread walks two groups, so the next
  group's dy and x are loaded while the current group's steps run.  Against per-step calls made in the same child."""
  cases = [[list(METRIC), 0, 16, 512, 512, 'f16', 5500], [list(SEQUENCES['run8']), 1, 16, 512, 512, 'f16', 5501]]
  out = run_child('_chain_bwd_runs_child.py', ['equal', json.dumps(cases)], {'EXPO_BWD_GROUPS_PER_THREAD': '4'})
  assert json.loads(out.strip().splitlines()[-1]) == [[], []]


PLAN_CASES = [[6, 64, 64, 'f16', 5600], [5, 50, 36, 'f32', 5601], [100, 64, 64, 'f16', 5602]]
PLANS = {
    'two-lanes': {'EXPO_CHAIN_STREAMS': '2'},
    # 1 MiB tiles: 100 x 64 x 64 fp16 runs as three tiles of 34 / 33 / 33 images, every tile through all its steps
    'tiles': {'EXPO_CHAIN_TILE_MIN_MIB': '0', 'EXPO_CHAIN_TILE_MIB': '1'},
}


@pytest.mark.parametrize('plan', sorted(PLANS))
def test_knob_one_reproduces_the_default_bytes(plan, gpu_device, tmp_path):
  outs = []
  for knob in (None, '1'):
    knobs = dict(PLANS[plan])
    if knob:
      knobs['EXPO_CHAIN_FUSE_BWD_STEPS'] = knob
    path = str(tmp_path / ('plan_%s.npz' % knob))
    run_child('_chain_plan_child.py', [json.dumps(PLAN_CASES), path], knobs)
    outs.append(np.load(path))
    assert json.loads(str(outs[-1]['env'])) == knobs
  fused, per_step = outs
  assert int(fused['c0_lanes']) == (2 if plan == 'two-lanes' else 1)
  assert len(fused['c2_chunks']) == (3 if plan == 'tiles' else 2), fused['c2_chunks']
  keys = sorted(k for k in fused.files if k != 'env')
  assert keys == sorted(k for k in per_step.files if k != 'env')
  assert any(k.endswith('grad_digest') for k in keys) and any('_dp' in k for k in keys)
  for k in keys:
    a, b = fused[k], per_step[k]
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), '%s: %s' % (plan, k)


# ---------------------------------------------------------------------------------------------------------------------
# the launches themselves: kernel nodes of a captured expo_chain_bwd (the steps' kernels plus one finish launch)
# ---------------------------------------------------------------------------------------------------------------------
# (filter ids, n, h, w, dtype, grads[0] = NULL)
ONE_LANE = [list(METRIC), 3, 64, 64, 'f16', False]
LAUNCH_CASES = [
    ONE_LANE,                                    # [C] [BW] [Ct] [T] [S+, W, G, E]
    [list(METRIC), 27, 512, 512, 'f16', False],  # two lanes: every lane launches its own runs
    [list(METRIC), 2, 33, 31, 'f16', False],     # odd fp16 pixel count: per-step launches
    [list(METRIC), 3, 64, 64, 'f16', True],      # step 0 (E) leaves the run: [S+, W, G] and a launch of its own
    [list(SEQUENCES['run8']), 3, 64, 64, 'f16', False],       # one run of 8
    [list(SEQUENCES['nine']), 3, 64, 64, 'f32', False],       # a run of 8, a single
    [list(SEQUENCES['acc-limit']), 3, 64, 64, 'f32', False],  # a run of 4 (48 accumulator floats), a single
    [list(SEQUENCES['all-seven']), 3, 64, 64, 'f16', False],  # [E, L] [BW] [Ct] [S+, W, G, E]
]


def test_default_runs_one_launch_per_run(gpu_device):
  """(With Contrast and WNB in the run table the metric order's counts would be 4 + 1, 2 * 4 + 1 and, without dx, 5 + 1.)"""
  assert _cabi.chain_plan(27, 512, 512, _cabi.EXPO_F16)[1] == 2
  got = [rc.backward_kernel_nodes(*case) for case in LAUNCH_CASES]
  assert got == [5 + 1, 2 * 5 + 1, 8 + 1, 6 + 1, 1 + 1, 2 + 1, 2 + 1, 4 + 1], got


@pytest.mark.parametrize('k,nodes', [(1, 8 + 1), (2, 6 + 1)])
def test_knob_sets_the_launch_count(k, nodes, gpu_device):
  """Metric order, one lane.  2: [C] [BW] [Ct] [T] [S+, W] [G, E] (5 + 1 with Contrast and WNB in the run table)."""
  out = run_child('_chain_bwd_runs_child.py', ['nodes', json.dumps([ONE_LANE])], {'EXPO_CHAIN_FUSE_BWD_STEPS': str(k)})
  assert json.loads(out.strip().splitlines()[-1]) == [nodes]
