"""Helper of tests/test_hip_chain_plans.py (not a test module): the chain entry points under one forced plan.

The chain's plan knobs (EXPO_CHAIN_STREAMS / _SNAKE / _TILE_MIB / _TILE_MIN_MIB) are read once per process, so the
test runs every forced configuration in a child process of its own:

    python tests/_chain_plan_child.py '<json list of [n, h, w, "f16" | "f32", seed]>' OUT.npz

For every case the child builds the inputs from the seed (make_inputs, which the parent calls too), runs every step
sequence of SEQUENCES through expo_chain_fwd / _bwd, one more expo_chain_bwd of the first sequence with grads[0] = NULL,
and writes to OUT.npz: its expo_chain_plan result, the parameter gradients, a digest of every image of every activation
and data gradient (bit-equality with the parent's per-step calls without shipping GiBs), and the activations and data
gradients of the images at the chunk boundaries in full (the parent's float64 oracle check)."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from exposure_amd import synthetic  # noqa: E402

# (name, filter ids, hsv_grad_mode).  's5' has an odd number of steps: the reversed walk's direction parity of the
# backward differs from 's8'.  's14' repeats filters, includes Level (id 8) and exceeds kMaxFinishSteps (12): the
# backward needs two finish launches.
SEQUENCES = (
    ('s8', tuple(range(8)), 0),
    ('s5', (4, 0, 7, 3, 5), 0),
    ('s14', (0, 3, 8, 4, 1, 7, 2, 8, 5, 6, 3, 0, 4, 7), 1),
)
NULL_DX_SEQUENCE = 's8'  # the one rerun with grads[0] = NULL
NP_DT = {'f16': np.float16, 'f32': np.float32}


def make_inputs(seed, shape, np_dt, ids):
  """(x, dy, [params of each step]) -- one draw per step, so a repeated filter gets parameters of its own."""
  rng = np.random.default_rng(seed)
  x = synthetic.make_images(rng, shape, np_dt)
  dy = synthetic.make_grad(rng, shape, np_dt)
  return x, dy, [synthetic.make_params(rng, fid, shape[0]) for fid in ids]


def image_digests(t):
  """(n, 16) uint8: a 128-bit BLAKE2 digest of the bytes of every image of an image tensor (device or host)."""
  a = t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)
  raw = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
  return np.stack([np.frombuffer(hashlib.blake2b(r.tobytes(), digest_size=16).digest(), np.uint8) for r in raw])


def boundary_images(chunks):
  """The first and the last image of every chunk, sorted."""
  return sorted({nb for nb, _, _ in chunks} | {nb + cnt - 1 for nb, cnt, _ in chunks})


def chain_bwd_without_dx(ids, acts, grads, params, dparams, hsv_grad_mode):
  """expo_chain_bwd with grads[0] = NULL (the gradient w.r.t. the chain's input is not wanted); grads[0] is ignored."""
  from exposure_amd import _cabi
  lib = _cabi.load()
  n, h, w, _ = acts[0].shape
  steps = len(ids)
  gp = _cabi._ptr_array(grads)
  gp[0] = None
  wsp, wsb = _cabi._ws(acts[0], None, steps)
  _cabi._check(lib.expo_chain_bwd((ctypes.c_int * steps)(*ids), steps, _cabi._ptr_array(acts), gp,
                                  _cabi._ptr_array(params), _cabi._ptr_array(dparams), n, h, w,
                                  _cabi._dtype_code(acts[0]), hsv_grad_mode, wsp, wsb, _cabi._stream()),
               'expo_chain_bwd (grads[0] = NULL)')


def run_case(k, case, out):
  import torch
  from exposure_amd import _cabi
  n, h, w, dt, seed = case
  np_dt = NP_DT[dt]
  t_dt = torch.float16 if dt == 'f16' else torch.float32
  dev = torch.device('cuda:0')
  shape = (n, h, w, 3)
  chunks, lanes, snake = _cabi.chain_plan(n, h, w, _cabi.EXPO_F16 if dt == 'f16' else _cabi.EXPO_F32)
  out['c%d_chunks' % k] = np.array(chunks, dtype=np.int64).reshape(-1, 3)
  out['c%d_lanes' % k] = np.int64(lanes)
  out['c%d_snake' % k] = np.int64(snake)
  edge = boundary_images(chunks)
  for name, ids, mode in SEQUENCES:
    x, dy, params = make_inputs(seed, shape, np_dt, ids)
    acts = [torch.from_numpy(x).to(dev)] + [torch.empty(shape, dtype=t_dt, device=dev) for _ in ids]
    grads = [torch.empty(shape, dtype=t_dt, device=dev) for _ in ids] + [torch.from_numpy(dy).to(dev)]
    prm = [torch.from_numpy(p).to(dev) for p in params]
    dps = [torch.full_like(p, float('nan')) for p in prm]
    _cabi.chain_fwd(list(ids), acts, prm)
    _cabi.chain_bwd(list(ids), acts, grads, prm, dps, hsv_grad_mode=mode)
    torch.cuda.synchronize()
    key = 'c%d_%s_' % (k, name)
    out[key + 'act_digest'] = np.stack([image_digests(a) for a in acts])
    out[key + 'grad_digest'] = np.stack([image_digests(g) for g in grads])
    out[key + 'act_edge'] = np.stack([a[edge].cpu().numpy() for a in acts])
    out[key + 'grad_edge'] = np.stack([g[edge].cpu().numpy() for g in grads])
    for i, dp in enumerate(dps):
      out[key + 'dp%d' % i] = dp.cpu().numpy()
    if name == NULL_DX_SEQUENCE:
      grads2 = [torch.full_like(acts[0], float('nan')) for _ in ids] + [grads[-1]]
      dps2 = [torch.full_like(p, float('nan')) for p in prm]
      chain_bwd_without_dx(list(ids), acts, grads2, prm, dps2, mode)
      torch.cuda.synchronize()
      key = 'c%d_null_' % k
      out[key + 'grad_digest'] = np.stack([image_digests(g) for g in grads2[1:]])
      for i, dp in enumerate(dps2):
        out[key + 'dp%d' % i] = dp.cpu().numpy()
    del acts, grads, prm, dps


def main(argv):
  cases = json.loads(argv[1])
  out = {'env': np.array(json.dumps({k: v for k, v in os.environ.items() if k.startswith('EXPO_CHAIN_')}))}
  for k, case in enumerate(cases):
    run_case(k, case, out)
  np.savez(argv[2], **out)
  return 0


if __name__ == '__main__':
  sys.exit(main(sys.argv))
