"""Helper of tests/test_hip_chain_bwd_recompute.py (not a test module), modelled on tests/_chain_bwd_runs_child.py.

EXPO_CHAIN_BWD_RECOMPUTE is read once per process, so the test runs the forced setting in a child process:

    python tests/_chain_bwd_recompute_child.py '<json list of [filter ids, hsv_grad_mode, n, h, w, "f16" | "f32", seed]>'

runs expo_chain_fwd and then expo_chain_bwd with every interior activation of every run replaced by a NaN-filled tensor
(poisoned_call below, which the test itself uses in its own process), and prints one JSON list with, per case,
[[i for which grads[i] holds a NaN], [i for which dparams[i] holds a NaN], [i for which grads[i] differs from the clean
call's], [i for which dparams[i] differs from the clean call's]].  (A NaN input need not give a NaN output: a step's dx
may not depend on its x at all -- Exposure, White balance -- and a clamp swallows a NaN.)

The module also restates, from DESIGN.md 3.28 / 3.30, how expo_chain_bwd collects its runs and which forwards the run
kernel recomputes: the library exports neither."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import _chain_plan_child as cp  # noqa: E402

# the run table: id -> accumulator floats per thread (kAccParts * NACC); a run holds at most 48 and at most 8 steps
RUN_ACC_FLOATS = {0: 4, 1: 4, 2: 12, 3: 4, 8: 8}
# the recomputable table of csrc/chain_steps_bwd_rc.hip (EXPO_RC_FILTERS): the filters whose forward the run kernel
# recomputes, per storage type
RECOMPUTED = {'f16': {0, 1, 2, 3, 8}, 'f32': {0, 1, 2, 3, 8}}


def runs_of(ids, dt, mode):
  """[(lowest step, head step)] of the runs of two or more steps, on the vector path with every grads[i] given."""
  out = []
  i = len(ids) - 1
  while i >= 0:
    cnt = acc = 0
    while cnt < 8 and i - cnt >= 0:
      fid = ids[i - cnt]
      if fid not in RUN_ACC_FLOATS or (fid == 3 and dt == 'f32' and mode == 1):
        break
      acc += RUN_ACC_FLOATS[fid]
      if acc > 48:
        break
      cnt += 1
    cnt = max(cnt, 1)
    if cnt > 1:
      out.append((i - cnt + 1, i))
    i -= cnt
  return out


def poisoned_positions(ids, dt, mode):
  """The acts[i] a recomputing expo_chain_bwd does not read: the output of a recomputed forward inside a run."""
  return sorted(i for lo, hi in runs_of(ids, dt, mode) for i in range(lo + 1, hi + 1) if ids[i - 1] in RECOMPUTED[dt])


def poisoned_call(ids, mode, x, dy, params, dt, dev):
  """(clean grads, clean dparams, poisoned grads, poisoned dparams, positions): one forward, two backwards."""
  import torch
  from exposure_amd import _cabi
  t_dt = torch.float16 if dt == 'f16' else torch.float32
  acts = [torch.from_numpy(x).to(dev)] + [torch.empty(x.shape, dtype=t_dt, device=dev) for _ in ids]
  prm = [torch.from_numpy(p).to(dev) for p in params]
  gy = torch.from_numpy(dy).to(dev)
  _cabi.chain_fwd(list(ids), acts, prm)
  where = poisoned_positions(ids, dt, mode)
  nan = torch.full_like(acts[0], float('nan'))
  bad_acts = [nan if i in where else a for i, a in enumerate(acts)]
  results = []
  for some_acts in (acts, bad_acts):
    grads = [torch.full_like(gy, float('nan')) for _ in ids] + [gy]
    dps = [torch.full_like(p, float('nan')) for p in prm]
    _cabi.chain_bwd(list(ids), some_acts, grads, prm, dps, hsv_grad_mode=mode)
    torch.cuda.synchronize()
    results += [grads, dps]
  return results + [where]


def nan_tensors(ids, mode, n, h, w, dt, seed):
  import torch
  x, dy, params = cp.make_inputs(seed, (n, h, w, 3), cp.NP_DT[dt], ids)
  clean, clean_dps, grads, dps, _ = poisoned_call(ids, mode, x, dy, params, dt, torch.device('cuda:0'))
  return [[i for i, g in enumerate(grads) if bool(torch.isnan(g).any())],
          [i for i, d in enumerate(dps) if bool(torch.isnan(d).any())],
          [i for i, g in enumerate(grads) if not torch.equal(g.view(torch.uint8), clean[i].view(torch.uint8))],
          [i for i, d in enumerate(dps) if not torch.equal(d.view(torch.int32), clean_dps[i].view(torch.int32))]]


if __name__ == '__main__':
  print(json.dumps([nan_tensors(*case) for case in json.loads(sys.argv[1])]))
