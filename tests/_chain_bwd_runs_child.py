"""Helper of tests/test_hip_chain_bwd_runs.py (not a test module), modelled on tests/_chain_fuse_child.py.

EXPO_CHAIN_FUSE_BWD_STEPS and EXPO_BWD_GROUPS_PER_THREAD are read once per process, so the test runs the forced
settings in child processes:

    python tests/_chain_bwd_runs_child.py nodes '<json list of [filter ids, n, h, w, "f16" | "f32", null_dx]>'

prints one JSON list: how many kernels one expo_chain_bwd call enqueues for each case.  The call is captured into a
hipGraph and the graph's kernel nodes are counted, so the number is what the runtime was handed, not what the library
says about itself.  null_dx: the call passes grads[0] = NULL.

    python tests/_chain_bwd_runs_child.py equal '<json list of [filter ids, hsv_grad_mode, n, h, w, "f16" | "f32", seed]>'

runs expo_chain_fwd / _bwd and, in the same process (the same knobs), expo_filter_bwd step by step on the chain's own
inputs, and prints one JSON list with, per case, the list of tensors that differ ([] = every grads[i] and dparams[i] is
bit-equal)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import _chain_fuse_child as fc  # noqa: E402
from tests import _chain_plan_child as cp  # noqa: E402


def count_kernel_nodes(graph):
  hip = fc._runtime()
  raw = ctypes.c_void_p(graph.raw_cuda_graph())
  count = ctypes.c_size_t(0)
  assert hip.hipGraphGetNodes(raw, None, ctypes.byref(count)) == 0
  nodes = (ctypes.c_void_p * max(count.value, 1))()
  assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(count)) == 0
  kernels = 0
  for k in range(count.value):
    kind = ctypes.c_int(-1)
    assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[k]), ctypes.byref(kind)) == 0
    kernels += kind.value == fc.HIP_GRAPH_NODE_TYPE_KERNEL
  return kernels


def backward_kernel_nodes(ids, n, h, w, dt, null_dx=False):
  """Kernel nodes of one captured expo_chain_bwd (the steps' kernels and the finish launch)."""
  import numpy as np
  import torch
  from exposure_amd import _cabi, synthetic
  dev = torch.device('cuda:0')
  t_dt = torch.float16 if dt == 'f16' else torch.float32
  rng = np.random.default_rng(5)
  acts = [torch.rand((n, h, w, 3), device=dev).to(t_dt)] + [torch.empty((n, h, w, 3), dtype=t_dt, device=dev) for _ in ids]
  grads = [torch.empty((n, h, w, 3), dtype=t_dt, device=dev) for _ in ids] + [torch.rand((n, h, w, 3), device=dev).to(t_dt)]
  prm = [torch.from_numpy(synthetic.make_params(rng, fid, n)).to(dev) for fid in ids]
  dps = [torch.empty_like(p) for p in prm]
  _cabi.chain_fwd(list(ids), acts, prm)

  def call():
    if null_dx:
      cp.chain_bwd_without_dx(list(ids), acts, grads, prm, dps, 0)
    else:
      _cabi.chain_bwd(list(ids), acts, grads, prm, dps)

  call()  # (eager first: the workspace and the helper-stream probe of a two-lane plan must exist before a capture)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph(keep_graph=True)
  with torch.cuda.graph(graph):
    call()
  return count_kernel_nodes(graph)


def differing_tensors(ids, mode, n, h, w, dt, seed):
  """Names of the grads[i] / dparams[i] of expo_chain_bwd that differ from expo_filter_bwd on the chain's own inputs."""
  import torch
  from exposure_amd import _cabi
  dev = torch.device('cuda:0')
  t_dt = torch.float16 if dt == 'f16' else torch.float32
  shape = (n, h, w, 3)
  x, dy, params = cp.make_inputs(seed, shape, cp.NP_DT[dt], ids)
  acts = [torch.from_numpy(x).to(dev)] + [torch.empty(shape, dtype=t_dt, device=dev) for _ in ids]
  grads = [torch.full(shape, float('nan'), dtype=t_dt, device=dev) for _ in ids] + [torch.from_numpy(dy).to(dev)]
  prm = [torch.from_numpy(p).to(dev) for p in params]
  dps = [torch.full_like(p, float('nan')) for p in prm]
  _cabi.chain_fwd(list(ids), acts, prm)
  _cabi.chain_bwd(list(ids), acts, grads, prm, dps, hsv_grad_mode=mode)
  torch.cuda.synchronize()
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


if __name__ == '__main__':
  fn = {'nodes': backward_kernel_nodes, 'equal': differing_tensors}[sys.argv[1]]
  print(json.dumps([fn(*case) for case in json.loads(sys.argv[2])]))
