"""Helper of tests/test_hip_chain_bwd_pairs.py (not a test module), modelled on tests/_chain_bwd_runs_child.py.

EXPO_CHAIN_BWD_RECOMPUTE, EXPO_STREAM_MIN_BYTES and EXPO_CHAIN_FUSE_BWD_STEPS are read once per process, so the test
runs every forced configuration in ONE child process of its own:

    python tests/_chain_bwd_pairs_child.py OUT.npz

runs every case of EQUAL_CASES (expo_chain_fwd / _bwd against expo_filter_fwd / _bwd step by step, in this process and
so under the same knobs) and every case of SATURATION_CASES, and writes to OUT.npz: 'equal', a JSON list with, per case,
the names of the tensors that differ ([] = every acts[i], grads[i] and dparams[i] is bit-equal), and the activations,
data gradients and parameter gradients of the saturation cases in full (the parent compares them with its own call's).

    python tests/_chain_bwd_pairs_child.py nodes

prints one JSON list: the kernel nodes of a captured expo_chain_bwd for every case of NODE_CASES.

The module also holds what the parent and the children must agree on: the covering set of step sequences, the edge
block written into image 0, and the fixed per-step parameters."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import _chain_bwd_recompute_child as rcc  # noqa: E402
from tests import _chain_plan_child as cp  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# the covering set: every ordered (producer -> consumer) pair of the run table and every run length 2..8, in every
# (storage type, hsv_grad_mode) -- tests/test_hip_chain_bwd_pairs.py::test_the_sequences_cover proves it from runs_of
# ---------------------------------------------------------------------------------------------------------------------
COVERING = {
    # each is ONE run in fp16 (both modes) and in fp32 mode 0; accumulator floats 40, 44, 36, 48, 28, 16, 8 (of 48)
    'len8': (0, 0, 1, 1, 3, 3, 8, 8),
    'len7': (8, 0, 2, 1, 0, 8, 3),
    'len6': (3, 1, 8, 2, 0, 3),
    'len5': (2, 2, 3, 2, 8),
    'len4': (8, 1, 2, 0),
    'len3': (3, 0, 8),
    'len2': (1, 3),
    # without S+: fp32 with hsv_grad_mode 1 cuts the sequences above at S+ (lengths 2, 4, 6 remain); these are one run
    # there as well
    'len3-no-s': (1, 0, 8),
    'len5-no-s': (0, 2, 8, 1, 0),
    'len7-no-s': (8, 0, 2, 1, 0, 8, 1),
    'len8-no-s': (0, 8, 1, 0, 0, 1, 8, 1),
}
RUN_IDS = (0, 1, 2, 3, 8)
CELLS = (('f16', 0), ('f16', 1), ('f32', 0), ('f32', 1))  # (storage type, hsv_grad_mode)


def fusable_ids(dt, mode):
  return tuple(f for f in RUN_IDS if not (f == 3 and dt == 'f32' and mode == 1))


def coverage(sequences, dt, mode):
  """(adjacent (producer, consumer) pairs inside runs, run lengths) of these sequences in one cell, from runs_of."""
  pairs, lengths = set(), set()
  for ids in sequences:
    for lo, hi in rcc.runs_of(ids, dt, mode):
      lengths.add(hi - lo + 1)
      pairs |= {(ids[i], ids[i + 1]) for i in range(lo, hi)}
  return pairs, lengths


# ---------------------------------------------------------------------------------------------------------------------
# inputs: cp.make_inputs, an edge block over the first rows of image 0, parameters drawn or fixed
# ---------------------------------------------------------------------------------------------------------------------
EDGE_ROWS = 16
# whole pixels, eight of each at the start of rows 0..7 of the block: black (lum 0), white (rng 0 at v = 1), negative
# (S+: v <= 0), greys (S+: rng 0; 1.5 is clamped), two channels tied at the minimum / at the maximum, and a pixel whose
# clamp to 1 makes the tie
PIXELS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-0.25, -0.25, -0.25), (0.5, 0.5, 0.5), (1.5, 1.5, 1.5),
          (0.25, 0.25, 0.75), (0.75, 0.25, 0.25), (1.0, 0.5, 2.0))
LEVEL_EXACT = (0.125, 0.6)  # lower = 0.125 is one of the specials: t == 0 exactly


def specials(np_dt):
  """The thresholds of the run table's filters, as float32 values that the storage type holds exactly (0.001 itself is
  rounded by it): Gamma's 0.001 and the two fp16 values around it, S+'s 1 and its two neighbours in the storage type,
  0 and -0, S+'s v = 0.5, the smallest fp16 normal and subnormal, values beyond both ends."""
  below = np.float16(0.001)
  below = below if float(below) < 0.001 else np.nextafter(below, np.float16(0))
  one = np_dt(1)
  return np.array([0.0, -0.0, 1.0, 0.001, float(below), float(np.nextafter(below, np.float16(1))), 0.125, 0.25, 0.5,
                   0.75, 0.875, 2.0, -1.0, 2.0**-14, 2.0**-24, float(np.nextafter(one, np_dt(0))),
                   float(np.nextafter(one, np_dt(2)))], dtype=np.float32)


def put_edge_block(x, seed):
  """Overwrites rows [0, EDGE_ROWS) of image 0: U(-0.5, 2) as tests/test_hip_filters.py::test_out_of_range_inputs draws
  it, every eleventh value one of specials(), then the rows of whole PIXELS."""
  rng = np.random.default_rng(seed)
  blk = rng.uniform(-0.5, 2.0, (EDGE_ROWS,) + x.shape[2:]).astype(np.float32)
  flat = blk.reshape(-1)
  sp = specials(x.dtype.type)
  flat[::11] = sp[np.arange(flat[::11].size) % sp.size]
  for r, pix in enumerate(PIXELS):
    blk[r, :8] = pix
  x[0, :EDGE_ROWS] = blk.astype(x.dtype)
  return x


# moderate parameters under which no step clips its gradient away (the liveness condition of the oracle test); the k-th
# occurrence of a filter in a sequence takes entry (k + image) modulo the list, so images and repeats differ
FIXED = {
    0: ((0.5,), (-0.75,), (0.25,), (-0.5,)),                         # EV
    1: ((0.6,), (1.7,)),                                             # gamma
    2: ((1.1, 0.9, 1.05), (0.85, 1.0, 1.2)),                         # white balance scales
    3: ((0.3,), (0.8,)),                                             # S+
    8: ((0.1, 0.6), (0.05, 0.7)),                                    # Level (lower, upper - 1)
}


def fixed_params(ids, n):
  seen, out = {}, []
  for i, fid in enumerate(ids):
    k = seen.get(fid, 0)
    seen[fid] = k + 1
    rows = [FIXED[fid][(k + img) % len(FIXED[fid])] for img in range(n)]
    if fid == 8 and i == 0:
      rows[0] = LEVEL_EXACT  # step 0 reads the edge block itself
    out.append(np.array(rows, dtype=np.float32))
  return out


def make_inputs(seed, shape, dt, ids, params='fixed'):
  """(x, dy, [params of each step]): cp.make_inputs with the edge block in image 0; `params` 'drawn' keeps the
  regressors' draws, 'fixed' takes fixed_params."""
  x, dy, drawn = cp.make_inputs(seed, shape, cp.NP_DT[dt], ids)
  put_edge_block(x, seed + 1)
  return x, dy, (drawn if params == 'drawn' else fixed_params(ids, shape[0]))


# ---------------------------------------------------------------------------------------------------------------------
# the cases every configuration runs
# ---------------------------------------------------------------------------------------------------------------------
EQUAL_SHAPE = (2, 256, 256)
# (sequence, storage type, hsv_grad_mode, parameters)
EQUAL_CASES = [(seq, dt, mode, prm) for seq in COVERING for dt, mode in CELLS for prm in ('fixed', 'drawn')]
NODE_CASES = [[list(COVERING[seq]), 3, 64, 64, dt, False] for seq in COVERING for dt in ('f16', 'f32')]

SATURATION = {'e-e-g': (0, 0, 1), 'e-w-e-s': (0, 2, 0, 3)}
SATURATION_SHAPE = (2, 64, 64)
SATURATION_CASES = [(seq, mode) for seq in SATURATION for mode in (0, 1)]


def equal_inputs(seq, dt, prm):
  ids = COVERING[seq]
  return make_inputs(7100 + 13 * sorted(COVERING).index(seq), EQUAL_SHAPE + (3,), dt, ids, prm)


def saturation_inputs(seq):
  """fp16: EV = +3.5 in every Exposure step (2^3.5 = 11.3), and an image that holds +-60000, 65504 and 3000 among
  ordinary values: the interior activations of the run saturate at +-65504 (the forward's MODE.FP16_OVFL store)."""
  ids = SATURATION[seq]
  shape = SATURATION_SHAPE + (3,)
  x, dy, _ = cp.make_inputs(7300 + len(ids), shape, np.float16, ids)
  big = np.array([60000.0, -60000.0, 65504.0, 3000.0, -3000.0, 6000.0], dtype=np.float16)
  flat = x.reshape(-1)
  flat[::7] = big[np.arange(flat[::7].size) % big.size]
  params = fixed_params(ids, shape[0])
  for i, fid in enumerate(ids):
    if fid == 0:
      params[i][:] = 3.5
  return x, dy, params


def run_chain(ids, mode, x, dy, params, dev):
  """expo_chain_fwd and expo_chain_bwd with distinct NaN-filled gradient buffers: (acts, grads, params, dparams)."""
  import torch
  from exposure_amd import _cabi
  acts = [torch.from_numpy(x).to(dev)]
  acts += [torch.full_like(acts[0], float('nan')) for _ in ids]
  prm = [torch.from_numpy(p).to(dev) for p in params]
  dps = [torch.full_like(p, float('nan')) for p in prm]
  gy = torch.from_numpy(dy).to(dev)
  grads = [torch.full_like(gy, float('nan')) for _ in ids] + [gy]
  _cabi.chain_fwd(list(ids), acts, prm)
  _cabi.chain_bwd(list(ids), acts, grads, prm, dps, hsv_grad_mode=mode)
  torch.cuda.synchronize()
  return acts, grads, prm, dps


def differing_activations(ids, acts, prm):
  """Names of the acts[i + 1] of expo_chain_fwd that differ from expo_filter_fwd applied to acts[i]."""
  import torch
  from exposure_amd import _cabi
  bad = []
  y = torch.empty_like(acts[0])
  for i, fid in enumerate(ids):
    y.fill_(float('nan'))
    _cabi.filter_fwd(fid, acts[i], y, prm[i])
    if not torch.equal(y.view(torch.uint8), acts[i + 1].view(torch.uint8)):
      bad.append('acts[%d]' % (i + 1))
  return bad


def differing_gradients(ids, mode, acts, grads, prm, dps):
  """Names of the grads[i] / dparams[i] of expo_chain_bwd that differ from expo_filter_bwd on the chain's own inputs."""
  import torch
  from exposure_amd import _cabi
  bad = []
  ref = torch.empty_like(acts[0])
  for i in reversed(range(len(ids))):
    dp = torch.full_like(prm[i], float('nan'))
    ref.fill_(float('nan'))
    _cabi.filter_bwd(ids[i], acts[i], grads[i + 1], ref, prm[i], dp, mode)
    if not torch.equal(ref.view(torch.uint8), grads[i].view(torch.uint8)):
      bad.append('grads[%d]' % i)
    if not torch.equal(dp.view(torch.int32), dps[i].view(torch.int32)):
      bad.append('dparams[%d]' % i)
  return bad


def saturation_tensors(seq, mode, dev):
  """({name: host array} of one saturation case, the names of the tensors that differ from the per-step calls)."""
  ids = SATURATION[seq]
  x, dy, params = saturation_inputs(seq)
  acts, grads, prm, dps = run_chain(ids, mode, x, dy, params, dev)
  bad = differing_activations(ids, acts, prm) + differing_gradients(ids, mode, acts, grads, prm, dps)
  out = {}
  for i in range(len(ids)):
    out['act%d' % (i + 1)] = acts[i + 1].cpu().numpy()
    out['grad%d' % i] = grads[i].cpu().numpy()
    out['dp%d' % i] = dps[i].cpu().numpy()
  return out, bad


def main(argv):
  if argv[1] == 'nodes':
    from tests import _chain_bwd_runs_child as rc
    print(json.dumps([rc.backward_kernel_nodes(*case) for case in NODE_CASES]))
    return 0
  import torch
  dev = torch.device('cuda:0')
  out = {'env': np.array(json.dumps({k: v for k, v in os.environ.items() if k.startswith('EXPO_')}))}
  equal = []
  for seq, dt, mode, prm_kind in EQUAL_CASES:
    ids = COVERING[seq]
    x, dy, params = equal_inputs(seq, dt, prm_kind)
    acts, grads, prm, dps = run_chain(ids, mode, x, dy, params, dev)
    equal.append(differing_activations(ids, acts, prm) + differing_gradients(ids, mode, acts, grads, prm, dps))
  out['equal'] = np.array(json.dumps(equal))
  for k, (seq, mode) in enumerate(SATURATION_CASES):
    tensors, bad = saturation_tensors(seq, mode, dev)
    out['s%d_bad' % k] = np.array(json.dumps(bad))
    for name, a in tensors.items():
      out['s%d_%s' % (k, name)] = a
  np.savez(argv[1], **out)
  return 0


if __name__ == '__main__':
  sys.exit(main(sys.argv))
