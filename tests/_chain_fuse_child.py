"""Helper of tests/test_hip_chain_fuse.py (not a test module): how many kernels does one expo_chain_fwd call enqueue?

The call is captured into a hipGraph and the graph's kernel nodes are counted, so the number is what the runtime was
handed, not what the library says about itself.  EXPO_CHAIN_FUSE_STEPS is read once per process, so the test runs the
forced settings in child processes:

    python tests/_chain_fuse_child.py '<json list of [filter ids, n, h, w, "f16" | "f32"]>'

prints one JSON list of kernel-node counts."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

HIP_GRAPH_NODE_TYPE_KERNEL = 0


def _runtime():
  """The HIP runtime this process already uses (torch's own copy where it ships one)."""
  import torch
  own = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
  return ctypes.CDLL(own if os.path.exists(own) else 'libamdhip64.so')


def forward_kernel_nodes(ids, n, h, w, dt):
  import numpy as np
  import torch
  from exposure_amd import _cabi, synthetic
  dev = torch.device('cuda:0')
  t_dt = torch.float16 if dt == 'f16' else torch.float32
  rng = np.random.default_rng(5)
  acts = [torch.rand((n, h, w, 3), device=dev).to(t_dt)] + [torch.empty((n, h, w, 3), dtype=t_dt, device=dev) for _ in ids]
  prm = [torch.from_numpy(synthetic.make_params(rng, fid, n)).to(dev) for fid in ids]
  _cabi.chain_fwd(list(ids), acts, prm)  # (eager first: the helper-stream probe of a two-lane plan cannot run in a capture)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph(keep_graph=True)
  with torch.cuda.graph(graph):
    _cabi.chain_fwd(list(ids), acts, prm)
  hip = _runtime()
  raw = ctypes.c_void_p(graph.raw_cuda_graph())
  count = ctypes.c_size_t(0)
  assert hip.hipGraphGetNodes(raw, None, ctypes.byref(count)) == 0
  nodes = (ctypes.c_void_p * max(count.value, 1))()
  assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(count)) == 0
  kernels = 0
  for k in range(count.value):
    kind = ctypes.c_int(-1)
    assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[k]), ctypes.byref(kind)) == 0
    kernels += kind.value == HIP_GRAPH_NODE_TYPE_KERNEL
  return kernels


if __name__ == '__main__':
  print(json.dumps([forward_kernel_nodes(*case) for case in json.loads(sys.argv[1])]))
