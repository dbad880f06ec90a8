"""Helper of tests/test_hip_chain_bwd_seq.py (not a test module), modelled on tests/_chain_bwd_pairs_child.py.

EXPO_CHAIN_BWD_SEQ, EXPO_CHAIN_BWD_RECOMPUTE, EXPO_STREAM_MIN_BYTES and EXPO_BWD_GROUPS_PER_THREAD are read once per
process, so the test runs every forced configuration in ONE child process of its own:

    python tests/_chain_bwd_seq_child.py OUT.npz all | groups

runs every case of CASES['all'] (or 'groups') and writes to OUT.npz, per case `name`: `name_bad`, a JSON list of the
tensors of expo_chain_bwd that differ from expo_filter_bwd step by step in this process ([] = every grads[i] and
dparams[i] is bit-equal); `name_seq`, by how much expo_chain_bwd_seq_launches() rose over the call; `name_digest`, one
128-bit digest per grads[i] and dparams[i]; and, once, `nodes`: the kernel nodes of a captured expo_chain_bwd for
NODE_CASES.

The module also holds what the parent and the children must agree on: the table of compiled sequences, the cases and
their inputs."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import _chain_bwd_pairs_child as pc  # noqa: E402
from tests import _chain_plan_child as cp  # noqa: E402

# EXPO_RUN_SEQUENCES of csrc/chain_steps_bwd_seq.hip: (storage type, hsv_grad_mode) -> the runs compiled, ids from the
# run's head down to its lowest step
TABLE = {('f16', 0): [(3, 2, 1, 0)], ('f16', 1): [(3, 2, 1, 0)], ('f32', 0): [(3, 2, 1, 0)]}
CELLS = tuple(sorted(TABLE))
RUN = (0, 1, 2, 3)          # the chain whose backward is the run (3, 2, 1, 0): the first four steps of the metric order
METRIC = tuple(range(8))    # backward: [C] [BW] [Ct] [T] [S+, W, G, E]
RUN8 = (0, 1, 2, 3, 8, 1, 0, 3)  # one run of 8: no sequence of the table

SHAPES = {
    'full': (3, 64, 64),       # whole 3 KiB wave chunks
    'partial': (2, 50, 36),    # a partial last chunk, idle waves at the reductions' barriers
    's256': (2, 256, 256),     # 393 216 values per tensor, the edge block of tests/_chain_bwd_pairs_child.py in image 0
}
TWO_LANES = (27, 512, 512)   # the smallest shape of tests/test_hip_chain_bwd_runs.py that expo_chain_plan gives two lanes
GROUPS = (16, 512, 512)      # at EXPO_BWD_GROUPS_PER_THREAD=4 every thread walks two groups (the same test)


def case_name(kind, shape, dt, mode):
  return '%s_%s_%s_m%d' % (kind, shape, dt, mode)


def build_cases():
  """name -> (kind, ids, shape, storage type, mode, seed)."""
  cases = {'all': {}, 'groups': {}}
  seed = 9100
  for dt, mode in CELLS:
    for shape in sorted(SHAPES):
      seed += 1
      cases['all'][case_name('equal', shape, dt, mode)] = ('edge' if shape == 's256' else 'plain', RUN, SHAPES[shape], dt,
                                                           mode, seed)
    seed += 1
    cases['all'][case_name('pingpong', 'full', dt, mode)] = ('pingpong', RUN, (5, 64, 96), dt, mode, seed)
    if dt == 'f16':
      seed += 1
      cases['all'][case_name('saturation', 'full', dt, mode)] = ('saturation', RUN, (2, 64, 64), dt, mode, seed)
  cases['all'][case_name('lanes', 'metric', 'f16', 0)] = ('plain', METRIC, TWO_LANES, 'f16', 0, 9200)
  cases['all'][case_name('outside', 'run8', 'f16', 0)] = ('plain', RUN8, SHAPES['full'], 'f16', 0, 9201)
  for dt, mode in CELLS:
    if dt == 'f16':
      cases['groups'][case_name('groups', 'run', dt, mode)] = ('plain', RUN, GROUPS, dt, mode, 9300 + mode)
  return cases


CASES = build_cases()
# (filter ids, n, h, w, storage type, grads[0] = NULL): the run and the finish; the metric order on one and two lanes
NODE_CASES = [[list(RUN), 3, 64, 64, 'f16', False], [list(RUN), 3, 64, 64, 'f32', False],
              [list(METRIC), 3, 64, 64, 'f16', False], [list(METRIC)] + list(TWO_LANES) + ['f16', False],
              [list(METRIC), 3, 64, 64, 'f16', True]]
NODES_TODAY = [1 + 1, 1 + 1, 5 + 1, 2 * 5 + 1, 6 + 1]


def inputs(kind, ids, shape, dt, seed):
  full = tuple(shape) + (3,)
  if kind == 'edge':
    return pc.make_inputs(seed, full, dt, ids, 'drawn')
  x, dy, params = cp.make_inputs(seed, full, cp.NP_DT[dt], ids)
  if kind == 'saturation':
    # pc.saturation_inputs on this sequence: EV = +3.5, an image that holds +-60000, 65504 and 3000
    big = np.array([60000.0, -60000.0, 65504.0, 3000.0, -3000.0, 6000.0], dtype=np.float16)
    flat = x.reshape(-1)
    flat[::7] = big[np.arange(flat[::7].size) % big.size]
    params = pc.fixed_params(ids, shape[0])
    for i, fid in enumerate(ids):
      if fid == 0:
        params[i][:] = 3.5
  return x, dy, params


def digest(t):
  a = np.ascontiguousarray(t.detach().cpu().numpy())
  return np.frombuffer(hashlib.blake2b(a.view(np.uint8).tobytes(), digest_size=16).digest(), np.uint8)


def run_case(case, dev):
  """(tensors that differ from the per-step calls, the counter's rise, digests of every grads[i] and dparams[i])."""
  import torch
  from exposure_amd import _cabi
  from tests import test_hip_chain_bwd_runs as runs
  kind, ids, shape, dt, mode, seed = case
  x, dy, params = inputs(kind, ids, shape, dt, seed)
  before = _cabi.chain_bwd_seq_launches()
  acts, grads, prm, dps = runs.run_chain(ids, mode, x, dy, params, dev)
  rose = _cabi.chain_bwd_seq_launches() - before
  bad = pc.differing_gradients(ids, mode, acts, grads, prm, dps)
  if kind == 'saturation':
    bad += pc.differing_activations(ids, acts, prm)
    if not bool((acts[1].abs() == 65504).any()):  # (S+ clamps to 1: the run's upper activations need hold none)
      bad.append('acts[1] holds no saturated value')
    if not all(bool(torch.isfinite(t.float()).all()) for t in grads[:-1] + dps):
      bad.append('a result that is not finite')
  if kind == 'pingpong':
    # two buffers, as bench.py builds them: the run's input grads[head + 1] is also the buffer of grads[head - 1]
    _, pp, _, pp_dps = runs.run_chain(ids, mode, x, dy, params, dev, pingpong=True)
    assert pp[0] is not pp[1] and pp[0] is pp[2]
    bad += ['pingpong grads[%d]' % i for i in (0, 1) if not torch.equal(pp[i].view(torch.uint8), grads[i].view(torch.uint8))]
    bad += ['pingpong dparams[%d]' % i for i in range(len(ids))
            if not torch.equal(pp_dps[i].view(torch.int32), dps[i].view(torch.int32))]
  return bad, rose, np.stack([digest(t) for t in grads[:-1] + dps])


def main(argv):
  import torch
  from tests import _chain_bwd_runs_child as rc
  dev = torch.device('cuda:0')
  out = {'env': np.array(json.dumps({k: v for k, v in os.environ.items() if k.startswith('EXPO_')}))}
  for name, case in CASES[argv[2]].items():
    bad, rose, digests = run_case(case, dev)
    out[name + '_bad'] = np.array(json.dumps(bad))
    out[name + '_seq'] = np.array(rose)
    out[name + '_digest'] = digests
  if argv[2] == 'all':
    out['nodes'] = np.array([rc.backward_kernel_nodes(*case) for case in NODE_CASES])
  np.savez(argv[1], **out)
  return 0


if __name__ == '__main__':
  sys.exit(main(sys.argv))
