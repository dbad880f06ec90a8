"""Every plan expo_chain_fwd / _bwd cut a batch into (exposure_hip.hip::chain_plan, include/exposure_hip.h):

* two lanes: a tensor of 40-256 MiB runs as two half-batches on the caller's stream and the library's helper stream
  (EXPO_CHAIN_STREAMS=1|2 forces this off / on);
* tile-major: a tensor of 256 MiB or more (EXPO_CHAIN_TILE_MIN_MIB) runs every step on one tile of images
  (EXPO_CHAIN_TILE_MIB per tensor, balanced: sizes differ by at most one image) before the next, each tile split over
  the two lanes when a tile of the smaller size would be.  The tile branch's `tn >= 2` guard cannot be reached: two
  lanes need chain_split(base) with base >= 2, and every tile holds base or base + 1 images;
* the reversed walk: alternate launches walk the images in reverse order (EXPO_CHAIN_TILE_MIB=0 with a tensor of
  256 MiB or more, or EXPO_CHAIN_SNAKE=1; ignored when the batch is tiled).

Each chunk launches with its own image, parameter and block-record offsets but the launch geometry of the WHOLE batch,
so every plan must give BIT-identical activations, data gradients and parameter gradients to per-step expo_filter_fwd /
expo_filter_bwd calls on the whole batch.  That is checked for every step, and the images at every chunk boundary
(first and last image of each chunk) are compared with the float64 oracle.  expo_chain_plan reports the plan a shape
got: every case asserts it reached the plan it is meant for (a mistyped knob would otherwise compare the default plan
with itself).  The knobs are read once per process: the default plans run in this process at real sizes, the forced
ones in child processes (tests/_chain_plan_child.py), one per configuration."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from exposure_amd import _cabi
from oracle import filters_np as fnp
from tests import _chain_plan_child as cp
from tests._tol import assert_image_close, assert_param_grad_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_DT = {'f16': torch.float16, 'f32': torch.float32}
CODE = {'f16': _cabi.EXPO_F16, 'f32': _cabi.EXPO_F32}


def lanes_of(at, n, two):
  """The chunks of `n` images from image `at`: one on lane 0, or n // 2 on lane 0 and the rest on lane 1."""
  if not two or n < 2:
    return [(at, n, 0)]
  return [(at, n // 2, 0), (at + n // 2, n - n // 2, 1)]


def tiles_of(sizes, two):
  chunks, at = [], 0
  for tn in sizes:
    chunks += lanes_of(at, tn, two)
    at += tn
  return chunks


def oracle_step(fid, x, p, dy, mode):
  """float64 (y, dx, dparams, A) of one step on the images given (A: the sum of absolute terms of each parameter
  gradient, tests/_tol.py).  The C restatement at 512 x 512 (it has no Level and only the TF-1 HSV gradient: those
  come from filters_np), filters_np below."""
  x64, p64, dy64 = (np.asarray(a, dtype=np.float64) for a in (x, p, dy))
  if x.shape[1] * x.shape[2] >= 512 * 512 and fid < 8:
    from oracle import filters_c as fc
    y = fc.process_packed(fid, x64, p64)
    dx, dp, a = fc.backward_packed(fid, x64, p64, dy64, with_abs=True)
    if fid == 3 and mode == 1:
      dx, _ = fnp.backward_packed(fid, x64, p64, dy64, hsv_grad_mode=1)
    return y, dx, dp, a
  y = fnp.process_packed(fid, x64, p64)
  dx, dp = fnp.backward_packed(fid, x64, p64, dy64, hsv_grad_mode=mode)
  return y, dx, dp, fnp.param_grad_abs(fid, x64, p64, dy64)


def check_edges_against_oracle(ids, mode, act_edge, grad_edge, dps, params, edge, np_dt, what):
  """act_edge / grad_edge: (steps + 1, len(edge), h, w, 3) host arrays of the chain's activations / data gradients at
  the boundary images; dps: the chain's parameter gradients of the whole batch."""
  for i, fid in enumerate(ids):
    y, dx, dp, a = oracle_step(fid, act_edge[i], params[i][edge], grad_edge[i + 1], mode)
    if np_dt == np.float16:
      np.clip(y, -65504.0, 65504.0, out=y)  # fp16 stores saturate
      np.clip(dx, -65504.0, 65504.0, out=dx)
    at = '%s step %d (filter %d) images %s' % (what, i, fid, edge)
    assert_image_close(act_edge[i + 1], y, np_dt, 'forward of ' + at)
    if fid == 3 and mode == 1:
      # the analytic HSV gradient has 1/range and 1/v factors: the relative bound of
      # test_hip_filters.py::test_satplus_analytic_mode, plus half an ulp of the fp16 storage
      got = np.asarray(grad_edge[i], dtype=np.float64)
      tol = 1e-3 + 1e-3 * np.abs(dx) + (np.abs(dx) * 2.0**-11 if np_dt == np.float16 else 0.0)
      err = np.abs(got - dx)
      assert (err <= tol).all(), 'dx of %s: worst err %.3e' % (at, err.max())
    else:
      assert_image_close(grad_edge[i], dx, np_dt, 'dx of ' + at)
    if fid == 3:
      # S+'s terms are dy (full - xc) with |full - xc| <= 1.  Where the filter is the identity on every pixel of an
      # image (each pixel's v is 0 or 1: full colour == the clamped pixel, as after a strong Exposure step), the float64
      # oracle's A is its own rounding noise (~1e-17 sum |dy|) and no entry of the comparison carries the scale that
      # tests/_tol.py's floor of 1e-10 max(A) refers to: the scale of such an image is sum |dy| itself
      a = np.maximum(a, 1e-10 * np.abs(np.asarray(grad_edge[i + 1], dtype=np.float64)).sum(axis=(1, 2, 3))[:, None])
    assert_param_grad_close(np.asarray(dps[i])[edge], dp, a, 'dparams of ' + at)


def differing_images(a, b):
  """Indices of the images whose bytes differ (device tensors, or (n, 16) digests)."""
  return torch.nonzero((a != b).reshape(a.shape[0], -1).any(dim=1)).flatten().tolist() if torch.is_tensor(a) else \
      np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# default knobs, in this process, at the sizes that choose the plans
# ---------------------------------------------------------------------------------------------------------------------
IN_PROCESS = {
    # 384 MiB per tensor: 4 tiles of 64 images, each on two lanes
    '256x512x512-f16': ((256, 512, 512, 'f16'), tiles_of([64] * 4, True)),
    # 285 MiB: balanced tiles 64 / 63 / 63, lanes 32 / 32, 31 / 32, 31 / 32
    '190x512x512-f16': ((190, 512, 512, 'f16'), tiles_of([64, 63, 63], True)),
    # 384 MiB in fp32: 4 tiles of 32 images, each on two lanes
    '128x512x512-f32': ((128, 512, 512, 'f32'), tiles_of([32] * 4, True)),
    # 40.5 MiB: one tile, uneven lanes 13 / 14
    '27x512x512-f16': ((27, 512, 512, 'f16'), lanes_of(0, 27, True)),
}


@pytest.mark.parametrize('name', sorted(IN_PROCESS))
def test_default_plan_equals_per_step_calls(name, gpu_device):
  (n, h, w, dt), want = IN_PROCESS[name]
  chunks, lanes, snake = _cabi.chain_plan(n, h, w, CODE[dt])
  assert (chunks, lanes, snake) == (want, 2, False), (chunks, lanes, snake)
  dev = gpu_device
  shape = (n, h, w, 3)
  np_dt = cp.NP_DT[dt]
  ids = list(range(8))
  x, dy, params = cp.make_inputs(77 + n, shape, np_dt, ids)
  acts = [torch.from_numpy(x).to(dev)] + [torch.empty(shape, dtype=TORCH_DT[dt], device=dev) for _ in ids]
  grads = [torch.empty(shape, dtype=TORCH_DT[dt], device=dev) for _ in ids] + [torch.from_numpy(dy).to(dev)]
  del x, dy
  prm = [torch.from_numpy(p).to(dev) for p in params]
  dps = [torch.full_like(p, float('nan')) for p in prm]
  _cabi.chain_fwd(ids, acts, prm)
  _cabi.chain_bwd(ids, acts, grads, prm, dps)
  # (a) bit-identical to per-step calls on the whole batch, fed the chain's own inputs of that step
  ref = torch.empty_like(acts[0])
  for i, fid in enumerate(ids):
    _cabi.filter_fwd(fid, acts[i], ref, prm[i])
    bad = differing_images(ref, acts[i + 1])
    assert not bad, '%s: forward of step %d differs from expo_filter_fwd on images %s' % (name, i, bad)
  for i, fid in enumerate(ids):
    dp = torch.full_like(prm[i], float('nan'))
    _cabi.filter_bwd(fid, acts[i], grads[i + 1], ref, prm[i], dp)
    bad = differing_images(ref, grads[i])
    assert not bad, '%s: dx of step %d differs from expo_filter_bwd on images %s' % (name, i, bad)
    bad = differing_images(dp, dps[i])
    assert not bad, '%s: dparams of step %d differ from expo_filter_bwd on images %s' % (name, i, bad)
  # (b) the float64 oracle on the images at the chunk boundaries
  edge = cp.boundary_images(chunks)
  act_edge = np.stack([a[edge].cpu().numpy() for a in acts])
  grad_edge = np.stack([g[edge].cpu().numpy() for g in grads])
  dps_host = [d.cpu().numpy() for d in dps]
  del acts, grads, ref
  torch.cuda.empty_cache()
  check_edges_against_oracle(ids, 0, act_edge, grad_edge, dps_host, params, edge, np_dt, name)


# ---------------------------------------------------------------------------------------------------------------------
# forced plans, one child process per configuration
# ---------------------------------------------------------------------------------------------------------------------
def _small(n, h, w, dt, two=False, snake=False):
  return [n, h, w, dt], lanes_of(0, n, two), snake


CHILDREN = {
    # 42 MiB would split by default
    'streams1': ({'EXPO_CHAIN_STREAMS': '1'}, [([28, 512, 512, 'f16'], [(0, 28, 0)], False)]),
    # n = 1 stays on one lane; n = 7 splits 3 / 4; 33 x 31 fp16 has an odd pixel count (the element path)
    'streams2': ({'EXPO_CHAIN_STREAMS': '2'},
                 [_small(n, h, w, dt, True) for n in (1, 2, 7) for h, w, dt in ((64, 64, 'f16'), (64, 64, 'f32'),
                                                                                 (33, 31, 'f16'))]),
    # 1 MiB tiles: 100 x 64 x 64 fp16 -> 42 images per tile -> 3 balanced tiles 34 / 33 / 33 on one lane; a 512 x 512
    # image is larger than a tile: tiles of one image
    'tiles': ({'EXPO_CHAIN_TILE_MIN_MIB': '0', 'EXPO_CHAIN_TILE_MIB': '1'},
              [([100, 64, 64, 'f16'], tiles_of([34, 33, 33], False), False),
               ([3, 512, 512, 'f16'], tiles_of([1, 1, 1], False), False)]),
    # the same tiles, each split over two lanes: 17 / 17, 16 / 17, 16 / 17 (tiles of one image cannot split)
    'tiles-streams2': ({'EXPO_CHAIN_TILE_MIN_MIB': '0', 'EXPO_CHAIN_TILE_MIB': '1', 'EXPO_CHAIN_STREAMS': '2'},
                       [([100, 64, 64, 'f16'], tiles_of([34, 33, 33], True), False),
                        ([3, 512, 512, 'f16'], tiles_of([1, 1, 1], False), False)]),
    # the reversed walk on one lane
    'snake': ({'EXPO_CHAIN_TILE_MIB': '0', 'EXPO_CHAIN_SNAKE': '1'},
              [_small(7, 64, 64, 'f16', snake=True), _small(5, 64, 64, 'f32', snake=True),
               _small(7, 33, 31, 'f16', snake=True)]),
    # ... and on two
    'snake-streams2': ({'EXPO_CHAIN_TILE_MIB': '0', 'EXPO_CHAIN_SNAKE': '1', 'EXPO_CHAIN_STREAMS': '2'},
                       [_small(7, 64, 64, 'f16', True, True), _small(5, 64, 64, 'f32', True, True),
                        _small(7, 33, 31, 'f16', True, True), _small(1, 64, 64, 'f16', True, True)]),
}
CHILD_TIMEOUT_S = 600


def per_step_reference(ids, mode, x, dy, params, dev):
  """Activations, data gradients and parameter gradients of per-step expo_filter_fwd / _bwd calls on the whole batch."""
  acts = [torch.from_numpy(x).to(dev)]
  prm = [torch.from_numpy(p).to(dev) for p in params]
  for i, fid in enumerate(ids):
    acts.append(torch.empty_like(acts[0]))
    _cabi.filter_fwd(fid, acts[i], acts[i + 1], prm[i])
  grads = [None] * len(ids) + [torch.from_numpy(dy).to(dev)]
  dps = [None] * len(ids)
  for i in reversed(range(len(ids))):
    grads[i] = torch.empty_like(acts[0])
    dps[i] = torch.full_like(prm[i], float('nan'))
    _cabi.filter_bwd(ids[i], acts[i], grads[i + 1], grads[i], prm[i], dps[i], mode)
  return acts, grads, [d.cpu().numpy() for d in dps]


@pytest.mark.parametrize('config', list(CHILDREN))
def test_forced_plan_equals_per_step_calls(config, gpu_device, tmp_path):
  knobs, cases = CHILDREN[config]
  env = {k: v for k, v in os.environ.items() if not k.startswith('EXPO_CHAIN_')}
  env.update(knobs)
  spec = [case + [1000 + 17 * k] for k, (case, _, _) in enumerate(cases)]
  out_path = str(tmp_path / 'chain_plan.npz')
  flags = ['-s'] if sys.flags.no_user_site else []
  proc = subprocess.run([sys.executable] + flags + [os.path.join(ROOT, 'tests', '_chain_plan_child.py'),
                                                    json.dumps(spec), out_path],
                        env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
  assert proc.returncode == 0, 'child (%s) exited with %d:\n%s' % (config, proc.returncode, proc.stderr[-4000:])
  out = np.load(out_path)
  assert json.loads(str(out['env'])) == knobs
  for k, (case, want, want_snake) in enumerate(cases):
    n, h, w, dt = case
    seed = spec[k][-1]
    what = '%s %dx%dx%d %s' % (config, n, h, w, dt)
    chunks = [tuple(int(v) for v in c) for c in out['c%d_chunks' % k]]
    lanes, snake = int(out['c%d_lanes' % k]), bool(out['c%d_snake' % k])
    assert (chunks, lanes, snake) == (want, 1 + max(c[2] for c in want), want_snake), (what, chunks, lanes, snake)
    edge = cp.boundary_images(chunks)
    np_dt = cp.NP_DT[dt]
    for name, ids, mode in cp.SEQUENCES:
      x, dy, params = cp.make_inputs(seed, (n, h, w, 3), np_dt, ids)
      acts, grads, dps = per_step_reference(ids, mode, x, dy, params, gpu_device)
      key = 'c%d_%s_' % (k, name)
      # (a) bit-identical: the digests of every image of every tensor, every parameter gradient
      for i in range(len(ids)):
        bad = differing_images(out[key + 'act_digest'][i + 1], cp.image_digests(acts[i + 1]))
        assert not bad, '%s %s: forward of step %d differs from expo_filter_fwd on images %s' % (what, name, i, bad)
      for i in reversed(range(len(ids))):
        bad = differing_images(out[key + 'grad_digest'][i], cp.image_digests(grads[i]))
        assert not bad, '%s %s: dx of step %d differs from expo_filter_bwd on images %s' % (what, name, i, bad)
        bad = differing_images(out[key + 'dp%d' % i].view(np.uint32), dps[i].view(np.uint32))
        assert not bad, '%s %s: dparams of step %d differ from expo_filter_bwd on images %s' % (what, name, i, bad)
      if name == cp.NULL_DX_SEQUENCE:
        # grads[0] = NULL: dx of the chain's input not wanted; everything else as with it
        for i in range(len(ids)):
          bad = differing_images(out['c%d_null_dp%d' % (k, i)].view(np.uint32), dps[i].view(np.uint32))
          assert not bad, '%s: dparams of step %d without dx differ on images %s' % (what, i, bad)
        for i in range(1, len(ids)):
          bad = differing_images(out['c%d_null_grad_digest' % k][i - 1], cp.image_digests(grads[i]))
          assert not bad, '%s: dx of step %d (grads[0] = NULL) differs on images %s' % (what, i, bad)
      del acts, grads
      # (b) the float64 oracle on the boundary images the CHILD computed
      check_edges_against_oracle(ids, mode, out[key + 'act_edge'], out[key + 'grad_edge'],
                                 [out[key + 'dp%d' % i] for i in range(len(ids))], params, edge, np_dt,
                                 '%s %s' % (what, name))
