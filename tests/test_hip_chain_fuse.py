"""expo_chain_fwd runs up to eight consecutive steps of a chunk in ONE launch (csrc/chain_steps.hip): a pixel group is
loaded once, every step's result is rounded to the storage type, stored to its activation and carried on in registers.
Nothing the entry points return may change by a bit:

* expo_chain_fwd against a sequence of expo_filter_fwd, expo_chain_bwd against expo_filter_bwd step by step, each fed
  the chain's own inputs of that step: torch.equal on every activation, every data gradient (distinct buffers) and
  every parameter gradient -- both storage types, both values of hsv_grad_mode, the metric order, a shuffled order, an
  order with repeated filters and adjacent curve steps, 1 / 3 / 8 / 9 steps (9 = one above the launch's maximum), a
  shape with a partial last chunk, one off the vector path (per-step launches), a batch on two lanes and a tiled one;
* ping-pong gradient buffers (two buffers, as bench.py builds them) against distinct ones;
* EXPO_CHAIN_FUSE_STEPS=1 (one kernel per step, the path before the fused kernel) against the default, byte for byte.

That the fused kernel really ran (the per-step fallback is bit-identical by contract and would pass all of the above) is
pinned by the number of kernel nodes of a captured expo_chain_fwd (tests/_chain_fuse_child.py), for the default and
for EXPO_CHAIN_FUSE_STEPS = 1 / 3.

The knobs are read once per process, so the forced configurations run in children (tests/_chain_plan_child.py, which
writes a digest of every image of every tensor)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from tests import _chain_fuse_child as fc
from tests import _chain_plan_child as cp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_DT_OF = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32}
CODE = {'f16': _cabi.EXPO_F16, 'f32': _cabi.EXPO_F32}
FUSE_MAX = 8  # kChainFuseMax (csrc/host_common.h)

# (filter ids, hsv_grad_mode)
SEQUENCES = {
    'metric': (tuple(range(8)), 0),
    'metric-hsv1': (tuple(range(8)), 1),
    'shuffled': ((5, 2, 7, 0, 3, 6, 1, 4), 0),
    # 9 steps (one above FUSE_MAX: a launch of 8 and a per-step one), repeats, adjacent curve steps, Level
    'repeats': ((4, 4, 7, 7, 3, 3, 8, 0, 4), 1),
    'one': ((3,), 0),
    'three': ((7, 4, 1), 1),
}
SHAPES = {
    'full': (3, 64, 64),      # whole 3 KiB wave chunks in both storage types
    'partial': (2, 50, 36),   # 1800 pixels: the last chunk of an image is partial, the last block has idle waves
    'odd': (2, 33, 31),       # fp16: an odd pixel count is off the dwordx3 path
    # 6.3 M values: a step whose conversion to fp16 rounded once where the per-step kernel rounds twice (or the other
    # way round: v_fma_mixlo_f16 against v_fma_f32 + v_cvt, csrc/chain_steps.hip) differs in one value of 2^14 -- about
    # 16 values for each of the 24 elements of a pixel group here, none at all in a small image
    'large': (8, 512, 512),
}


def run_chain(ids, mode, x, dy, params, dev, pingpong=False):
  acts = [torch.from_numpy(x).to(dev)] + [torch.full(x.shape, float('nan'), dtype=TORCH_DT_OF[x.dtype], device=dev)
                                          for _ in ids]
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
  _cabi.chain_bwd(list(ids), acts, grads, prm, dps, hsv_grad_mode=mode)
  torch.cuda.synchronize()
  return acts, grads, prm, dps


def assert_equals_per_step_calls(ids, mode, acts, grads, prm, dps, what):
  """Every step of the chain against expo_filter_fwd / expo_filter_bwd fed the chain's own inputs of that step."""
  ref = torch.empty_like(acts[0])
  for i, fid in enumerate(ids):
    ref.fill_(float('nan'))
    _cabi.filter_fwd(fid, acts[i], ref, prm[i])
    assert torch.equal(ref.view(torch.uint8), acts[i + 1].view(torch.uint8)), \
        '%s: acts[%d] (filter %d) differs from expo_filter_fwd' % (what, i + 1, fid)
  for i in reversed(range(len(ids))):
    fid = ids[i]
    dp = torch.full_like(prm[i], float('nan'))
    ref.fill_(float('nan'))
    _cabi.filter_bwd(fid, acts[i], grads[i + 1], ref, prm[i], dp, mode)
    assert torch.equal(ref.view(torch.uint8), grads[i].view(torch.uint8)), \
        '%s: grads[%d] (filter %d) differs from expo_filter_bwd' % (what, i, fid)
    assert torch.equal(dp.view(torch.int32), dps[i].view(torch.int32)), \
        '%s: dparams[%d] (filter %d) differ from expo_filter_bwd' % (what, i, fid)


@pytest.mark.parametrize('dt', ['f16', 'f32'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('seq', sorted(SEQUENCES))
def test_chain_equals_per_step_calls(seq, shape, dt, gpu_device):
  ids, mode = SEQUENCES[seq]
  n, h, w = SHAPES[shape]
  x, dy, params = cp.make_inputs(4100 + 7 * len(ids) + n, (n, h, w, 3), cp.NP_DT[dt], ids)
  acts, grads, prm, dps = run_chain(ids, mode, x, dy, params, gpu_device)
  assert_equals_per_step_calls(ids, mode, acts, grads, prm, dps, '%s %s %s' % (seq, shape, dt))


@pytest.mark.parametrize('dt', ['f16', 'f32'])
def test_two_lane_chain_equals_per_step_calls(dt, gpu_device):
  """40.5 / 42 MiB per tensor: two half-batches (13 / 14 or 7 / 7 images) on the caller's stream and the helper."""
  n = 27 if dt == 'f16' else 14
  chunks, lanes, snake = _cabi.chain_plan(n, 512, 512, CODE[dt])
  assert (chunks, lanes, snake) == ([(0, n // 2, 0), (n // 2, n - n // 2, 1)], 2, False)
  ids, mode = SEQUENCES['repeats']
  x, dy, params = cp.make_inputs(4200, (n, 512, 512, 3), cp.NP_DT[dt], ids)
  acts, grads, prm, dps = run_chain(ids, mode, x, dy, params, gpu_device)
  del x, dy
  assert_equals_per_step_calls(ids, mode, acts, grads, prm, dps, 'two lanes %s' % dt)


@pytest.mark.parametrize('dt', ['f16', 'f32'])
@pytest.mark.parametrize('seq', ['metric', 'repeats', 'three'])
def test_pingpong_grads_equal_distinct_buffers(seq, dt, gpu_device):
  ids, mode = SEQUENCES[seq]
  x, dy, params = cp.make_inputs(4300, (5, 64, 96, 3), cp.NP_DT[dt], ids)
  _, grads, _, dps = run_chain(ids, mode, x, dy, params, gpu_device)
  _, pp, _, pp_dps = run_chain(ids, mode, x, dy, params, gpu_device, pingpong=True)
  assert pp[0] is not pp[1] and (len(ids) < 3 or pp[0] is pp[2])
  assert torch.equal(pp[0].view(torch.uint8), grads[0].view(torch.uint8)), 'grads[0]'
  # the second buffer ends with the last gradient written to it: grads[1] (the odd steps write it, step 1 last)
  if len(ids) > 1:
    assert torch.equal(pp[1].view(torch.uint8), grads[1].view(torch.uint8)), 'second buffer'
  for i in range(len(ids)):
    assert torch.equal(pp_dps[i].view(torch.int32), dps[i].view(torch.int32)), 'dparams[%d]' % i


# ---------------------------------------------------------------------------------------------------------------------
# knobs that are read once per process: child processes
# ---------------------------------------------------------------------------------------------------------------------
CHILD_CASES = [[3, 64, 64, 'f16', 4400], [2, 50, 36, 'f32', 4401], [2, 33, 31, 'f16', 4402], [100, 64, 64, 'f16', 4403]]
CHILDREN = {
    # one kernel per step: the path before the fused kernel existed
    'fuse1': {'EXPO_CHAIN_FUSE_STEPS': '1'},
    'fuse3': {'EXPO_CHAIN_FUSE_STEPS': '3'},
    # 1 MiB tiles: 100 x 64 x 64 fp16 runs as three tiles of 34 / 33 / 33 images, every tile through all its steps
    'tiles': {'EXPO_CHAIN_TILE_MIN_MIB': '0', 'EXPO_CHAIN_TILE_MIB': '1'},
    'tiles-two-lanes': {'EXPO_CHAIN_TILE_MIN_MIB': '0', 'EXPO_CHAIN_TILE_MIB': '1', 'EXPO_CHAIN_STREAMS': '2'},
}


@pytest.mark.parametrize('config', sorted(CHILDREN))
def test_knobs_reproduce_the_same_bytes(config, gpu_device, tmp_path):
  """The child's chain (forced knobs) against THIS process's chain (default knobs) and against per-step calls."""
  knobs = CHILDREN[config]
  env = {k: v for k, v in os.environ.items() if not k.startswith('EXPO_CHAIN_')}
  env.update(knobs)
  out_path = str(tmp_path / 'chain_fuse.npz')
  flags = ['-s'] if sys.flags.no_user_site else []
  proc = subprocess.run([sys.executable] + flags + [os.path.join(ROOT, 'tests', '_chain_plan_child.py'),
                                                    json.dumps(CHILD_CASES), out_path],
                        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert proc.returncode == 0, 'child (%s) exited with %d:\n%s' % (config, proc.returncode, proc.stderr[-4000:])
  out = np.load(out_path)
  assert json.loads(str(out['env'])) == knobs
  if config.startswith('tiles'):
    assert len(out['c3_chunks']) == (6 if 'lanes' in config else 3), out['c3_chunks']
  for k, (n, h, w, dt, seed) in enumerate(CHILD_CASES):
    for name, ids, mode in cp.SEQUENCES:
      x, dy, params = cp.make_inputs(seed, (n, h, w, 3), cp.NP_DT[dt], ids)
      acts, grads, prm, dps = run_chain(ids, mode, x, dy, params, gpu_device)
      what = '%s %dx%dx%d %s %s' % (config, n, h, w, dt, name)
      assert_equals_per_step_calls(ids, mode, acts, grads, prm, dps, what)
      key = 'c%d_%s_' % (k, name)
      for i in range(len(ids) + 1):
        assert (out[key + 'act_digest'][i] == cp.image_digests(acts[i])).all(), '%s: acts[%d]' % (what, i)
        assert (out[key + 'grad_digest'][i] == cp.image_digests(grads[i])).all(), '%s: grads[%d]' % (what, i)
      for i in range(len(ids)):
        assert (out[key + 'dp%d' % i].view(np.uint32) == dps[i].cpu().numpy().view(np.uint32)).all(), \
            '%s: dparams[%d]' % (what, i)


# ---------------------------------------------------------------------------------------------------------------------
# the launches themselves: kernel nodes of a captured expo_chain_fwd
# ---------------------------------------------------------------------------------------------------------------------
# (filter ids, n, h, w, dtype) and the kernel nodes expected with at most k steps per launch: per chunk of the plan
# ceil-wise runs of k steps, every run one launch (a run of one step is a per-step launch: still one); off the vector
# path one launch per step whatever k
LAUNCH_CASES = [
    (list(range(8)), 3, 64, 64, 'f16', True, 1),
    (list(range(8)), 3, 64, 64, 'f32', True, 1),
    ([4, 4, 7, 7, 3, 3, 8, 0, 4], 2, 50, 36, 'f16', True, 1),   # 9 steps
    (list(range(8)), 2, 33, 31, 'f16', False, 1),                # odd fp16 pixel count: per-step launches
    (list(range(8)), 27, 512, 512, 'f16', True, 2),              # two lanes: every lane launches its own runs
]


def expected_nodes(k):
  return [chunks * (-(-len(ids) // k) if vec else len(ids)) for ids, _, _, _, _, vec, chunks in LAUNCH_CASES]


def test_default_runs_eight_steps_per_launch(gpu_device):
  got = [fc.forward_kernel_nodes(*case[:5]) for case in LAUNCH_CASES]
  assert got == expected_nodes(FUSE_MAX) == [1, 1, 2, 8, 2], got


@pytest.mark.parametrize('k', [1, 3])
def test_fuse_steps_knob_sets_the_launch_count(k, gpu_device):
  env = {key: v for key, v in os.environ.items() if not key.startswith('EXPO_CHAIN_')}
  env['EXPO_CHAIN_FUSE_STEPS'] = str(k)
  flags = ['-s'] if sys.flags.no_user_site else []
  proc = subprocess.run([sys.executable] + flags + [os.path.join(ROOT, 'tests', '_chain_fuse_child.py'),
                                                    json.dumps([case[:5] for case in LAUNCH_CASES])],
                        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert proc.returncode == 0, 'child exited with %d:\n%s' % (proc.returncode, proc.stderr[-4000:])
  got = json.loads(proc.stdout.strip().splitlines()[-1])
  assert got == expected_nodes(k), (k, got)
  assert got == ([8, 8, 9, 8, 16] if k == 1 else [3, 3, 3, 8, 6])
