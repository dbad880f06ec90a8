"""Every cache-policy and path instantiation of the inference kernels.

The host side picks an inference kernel by storage type, tap format, code width, channels -- and by two choices that no
caller sees: the cache policy (IoStream from EXPO_STREAM_MIN_BYTES = 8 MiB per call, IoCached below) and the pixel path
(12-byte vectors or element-wise; ANY_SLOW per launch in the ragged passes).  Every real photo is past 8 MiB, and the
rest of the suite launches almost none of the streaming kernels.  Here:

1. the ledger (no GPU): tests/_policy_matrix_cases.py enumerates the instantiations as a literal product of the template
   parameters -- 88 + 32 + 96 + 96 in the four fused units, as tests/test_isa_*.py and DESIGN.md §3.31 count them, and
   decode.hip's and codes_lut.hip's on top --, restates the selection rule (tests/test_ragged_launch_host.py holds the
   ragged part of the restatement to the host code itself) and proves that its cases, under the default threshold and
   under EXPO_STREAM_MIN_BYTES=1 together, select every cell but a set stated as a predicate: float32 storage on the
   element-wise path of a kernel whose path depends on float32 pointers alone (28 kernels: no tensor has a float32
   base that is not 4-byte aligned).  No case is redundant;
2. on the GPU, in process (the cached policy at these sizes): every image of every case against the float64 chain
   under tests/_tol.py's bounds (u8 / u16 taps: the same bound carried through the quantiser), the decodes, tables and
   maxima bit for bit against load_image's float32 maths, the look-ups against a NumPy gather; guards intact;
3. one child process with EXPO_STREAM_MIN_BYTES=1 runs every case again: byte for byte the parent's outputs, image by
   image and tap by tap (the policies change cache bits only);
4. batch invariance: an image's bytes do not depend on whether its launch is all-vector or mixed.

The images are the smallest at which these kernels can still go wrong (a block covers 2048 pixels in fp16, 1024 in
fp32): 41x50 (two / three blocks, a partial last group), 37x53 (odd), 1x2, 4x6, 1x1, and 41x50 with one base at a time
one element into its buffer."""
import functools
import json
import os
import tempfile

import numpy as np
import pytest

from tests import _policy_matrix_cases as pm
from tests import _policy_matrix_child as pc
from tests._tol import assert_image_close, image_tol

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# 1. the ledger (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_enumeration_has_the_pinned_counts():
  e = pm.enumerate_instantiations()
  by_kernel = {}
  for inst in e['chain_fused.hip']:
    by_kernel[inst[0]] = by_kernel.get(inst[0], 0) + 1
  assert list(by_kernel.values()) == [6, 18, 8, 24, 32] and len(e['chain_fused.hip']) == 88
  assert len(e['chain_fused_curves.hip']) == 32
  assert len(e['chain_fused_codes.hip']) == len(e['chain_fused_curves_codes.hip']) == 96
  assert len(e['decode.hip']) == 48 + 12 and len(e['codes_lut.hip']) == 24 + 6
  for unit, insts in e.items():
    assert len(set(insts)) == len(insts), unit


def test_the_cases_cover_every_reachable_cell():
  """the union over the case table, under both thresholds, is the enumeration minus exactly the predicate"""
  cells = pm.all_cells()
  run = pm.cells_run()
  assert run <= cells
  not_run = cells - run
  assert not_run == {cell for cell in cells if pm.unreachable(cell)}
  assert len(not_run) == (2 + 6 + 8 + 8) + (1 + 3) == 28
  by_kernel = {}
  for cell in not_run:
    by_kernel[cell[0]] = by_kernel.get(cell[0], 0) + 1
  assert by_kernel == {'chain_fused_fwd_ragged_kernel': 2, 'chain_fused_fwd_ragged_taps_kernel': 6,
                       'chain_fused_masked_ragged_kernel': 8, 'chain_fused_curves_ragged_kernel': 8,
                       'chain_fused_fwd_kernel': 1, 'chain_fused_fwd_taps_kernel': 3}


def test_every_instantiation_but_the_28_is_launched_under_each_policy_it_has():
  """per instantiation (not per path): the parent's threshold selects the IoCached ones, the child's the IoStream
  ones"""
  insts = {inst for unit in pm.enumerate_instantiations().values() for inst in unit}

  def launched(smb):
    cells = set()
    for case in pm.CASES:
      cells |= pm.case_cells(case, smb)
    return {cell[0] if isinstance(cell[0], tuple) else cell for cell in cells}

  parent, child = launched(pm.THRESHOLDS[0]), launched(pm.THRESHOLDS[1])
  assert all('stream' not in inst for inst in parent) and parent
  dense = ('chain_fused_fwd_kernel', 'chain_fused_fwd_taps_kernel')  # (element-wise dense calls never stream)
  assert all('stream' in inst for inst in child if inst[0] not in dense)
  assert len(insts - parent - child) == 28 and all(pm.unreachable(inst) for inst in insts - parent - child)


@pytest.mark.parametrize('case_id', pm.CASE_IDS)
def test_no_case_is_redundant(case_id):
  """without any one case a cell is lost"""
  rest = [c for c in pm.CASES if c['id'] != case_id]
  assert pm.cells_run(rest) != pm.cells_run()


def test_torch_offers_no_misaligned_float32_tensor():
  """the predicate's premise: a float32 view of a byte buffer one, two or three bytes in is refused"""
  import torch
  buf = torch.zeros(64, dtype=torch.uint8)
  for off in (1, 2, 3):
    with pytest.raises(RuntimeError):
      buf[off:off + 16].view(torch.float32)
  half = torch.zeros(32, dtype=torch.float16)
  with pytest.raises(RuntimeError):
    half[1:9].view(torch.float32)


def test_both_paths_sit_in_every_mixed_call():
  """the kernels that hold both paths: every case's one call has vector and element-wise images under both thresholds"""
  for case in pm.CASES:
    if case['family'] in pm.RAGGED_KERNEL or case['family'] in ('dense', 'dense_taps'):
      continue
    for smb in pm.THRESHOLDS:
      paths = {cell[1] for cell in pm.case_cells(case, smb)}
      assert paths == set(pm.PATHS), (case['id'], smb)


def test_host_decode_is_load_images_maths():
  from exposure_amd import evaluate
  from tests.test_hip_decode import host_math
  for ct, kind in (('u8', 'srgb8'), ('u16', 'srgb16'), ('u16', 'prophoto16')):
    for c in pm.CHANNELS:
      codes = pc.code_image(ct, c, 'S')
      a, b = pc.host_decode(codes, kind, evaluate.DECODE_NORMALIZE[kind]), host_math(codes, kind)
      assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('chain', ['p24', 'masked', 'curves'])
def test_every_reference_is_alive(chain):
  """Liveness, on the reference: no image's reference output is constant, and no tap's; an image whose sequence ends
  on -1 is exactly +0 in its output and alive in the taps before."""
  used = [u for u in pc.references_used() if u[0] == chain]
  assert used
  for _, source, key in used:
    ref = pc.reference(chain, source, key)
    assert len(ref) == pm.STEPS and all(np.isfinite(r).all() for r in ref)
    assert np.abs(ref[-1]).max() < 60000.0  # (fp16 storage saturates nowhere)
    for k in pc.KEPT[:-1]:
      assert np.ptp(ref[k]) > 1e-3, (chain, source, key, k)
    if key in pm.MINUS_ONE:
      assert pm.SEQUENCES[key][-1] == -1 and not ref[-1].any() and not np.signbit(ref[-1]).any()
    else:
      assert -1 not in pm.SEQUENCES[key] and np.ptp(ref[-1]) > 1e-3, (chain, source, key)


# ---------------------------------------------------------------------------------------------------------------------
# 2. in process: against the independent references
# ---------------------------------------------------------------------------------------------------------------------
_PARENT = {}


def parent_outputs(case_id, dev):
  """the case's outputs under this process's policy (the default threshold: IoCached at these sizes), run once"""
  if case_id not in _PARENT:
    _PARENT[case_id] = pc.run_case(pm.BY_ID[case_id], dev)
  return _PARENT[case_id]


def assert_taps_close(got, refs, fmt, np_dt, what):
  """storage taps: the image bound; u8 / u16 taps: |tap - clip(q ref, 0, q)| <= 0.5 + q image_tol(ref), the same bound
  carried through the quantiser (half a code for the rounding, the image bound scaled to codes)"""
  assert got.shape[0] == len(pc.KEPT)
  for j, k in enumerate(pc.KEPT):
    ref = refs[k]
    if fmt == pm.TAP_STORAGE:
      assert_image_close(got[j].astype(np.float64), ref, np_dt, '%s storage tap of step %d' % (what, k))
    else:
      q = 255.0 if fmt == pm.TAP_U8 else 65535.0
      assert got.dtype == (np.uint8 if fmt == pm.TAP_U8 else np.uint16)
      err = np.abs(got[j].astype(np.float64) - np.clip(q * ref, 0.0, q))
      tol = 0.5 + q * image_tol(ref, np_dt)
      assert (err <= tol).all(), '%s %s tap of step %d: worst err / tol %.3f' % (what, pm.FMT_NAME[fmt], k,
                                                                                   (err / tol).max())


def check_chain_case(case, out):
  np_dt = pc.NP_T[case['dtype']]
  chain, source = pc.CHAIN_OF[case['family']], pc.source_of(case)
  names = set()
  for key in pm.case_images(case):
    what = '%s image %s' % (case['id'], key)
    ref = [r.copy() for r in pc.reference(chain, source, key)]
    if np_dt == np.float16:
      ref = [np.clip(r, -65504.0, 65504.0) for r in ref]
    y = out['%s.y' % key]
    names.add('%s.y' % key)
    assert y.dtype == np_dt and y.shape == ref[-1].shape
    assert_image_close(y.astype(np.float64), ref[-1], np_dt, what)
    if key in pm.MINUS_ONE:
      assert not y.view(np.uint8).any(), '%s: not exactly +0 after -1' % what
    if case['fmt'] != pm.TAP_NONE:
      tap = out['%s.tap' % key]
      names.add('%s.tap' % key)
      assert_taps_close(tap, ref, case['fmt'], np_dt, what)
      if pm.without_ys(case):  # ys = NULL: the same planes
        only = out['%s.tap_only' % key]
        names.add('%s.tap_only' % key)
        assert only.dtype == tap.dtype and only.tobytes() == tap.tobytes(), '%s: taps without ys differ' % what
  assert names == set(out)


def check_gather_case(case, out):
  from exposure_amd import evaluate
  f, ct, c = case['family'], case['ct'], case['c']
  keys = pm.case_images(case)
  codes = [pc.code_image(ct, c, k) for k in keys]
  if f == 'decode':
    kind = pm.DECODE_KIND[(ct, case['norm'])]
    np_dt = pc.NP_T[case['dtype']]
    want = {'%s.y' % k: pc.host_decode(cd, kind, case['norm']).astype(np_dt) for k, cd in zip(keys, codes)}
  elif f == 'decode_tables':
    table = evaluate.decode_table(pm.DECODE_KIND[(ct, True)], 'cpu').numpy()
    assert table.dtype == np.float32
    want = {'tables': np.stack([table / (2 * table[int(pc.c3(cd).max())]) for cd in codes]).astype(
        pc.NP_T[pc.TABLES_DTYPE[ct]])}
  elif f == 'codes_max':
    want = {'maxima': np.array([int(pc.c3(cd).max()) for cd in codes], dtype=np.int32)}
    assert len(set(want['maxima'].tolist())) > 1
  else:
    luts = pc.lut_tables(case)
    want = {'%s.y' % k: luts[i][pc.c3(cd).astype(np.int64)] for i, (k, cd) in enumerate(zip(keys, codes))}
  assert set(out) == set(want)
  for name, w in want.items():
    g = out[name]
    assert g.dtype == w.dtype and g.shape == w.shape, (case['id'], name)
    bad = int((g.view(np.uint8) != w.view(np.uint8)).sum()) if g.size else 0
    assert bad == 0, '%s %s: %d bytes differ from the host' % (case['id'], name, bad)
    assert np.ptp(w.astype(np.float64)) > 0 or w.size <= 3, (case['id'], name)


@gpu
@pytest.mark.parametrize('case_id', pm.CASE_IDS)
def test_matches_the_independent_reference(case_id, gpu_device):
  case = pm.BY_ID[case_id]
  out = parent_outputs(case_id, gpu_device)
  if case['family'] in pc.CHAIN_OF:
    check_chain_case(case, out)
  else:
    check_gather_case(case, out)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the streaming instantiations: one child process, byte for byte the cached ones
# ---------------------------------------------------------------------------------------------------------------------
KNOBS = {'EXPO_STREAM_MIN_BYTES': '1'}


@functools.lru_cache(maxsize=None)
def child_results():
  """One child process runs every case under EXPO_STREAM_MIN_BYTES=1 (tests/_policy_matrix_child.py) and is shared by
  the tests that read its results."""
  from tests.test_hip_chain_bwd_runs import run_child
  with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, 'stream.npz')
    run_child('_policy_matrix_child.py', [path], KNOBS)
    with np.load(path) as f:
      return {k: f[k] for k in f.files}


@gpu
def test_the_child_ran_under_the_knob(gpu_device):
  env = json.loads(str(child_results()['env']))
  assert {k: env.get(k) for k in KNOBS} == KNOBS, env
  assert 'EXPO_STREAM_MIN_BYTES' not in os.environ, 'this process must run under the default threshold'
  cases = {k.split('|')[0] for k in child_results() if k != 'env'}
  assert cases == set(pm.CASE_IDS)


@gpu
@pytest.mark.parametrize('case_id', pm.CASE_IDS)
def test_streaming_equals_cached_bit_for_bit(case_id, gpu_device):
  mine = parent_outputs(case_id, gpu_device)
  theirs = {k.split('|', 1)[1]: v for k, v in child_results().items() if k.startswith(case_id + '|')}
  assert set(theirs) == set(mine)
  differing = [name for name, a in mine.items()
               if not (a.dtype == theirs[name].dtype and a.shape == theirs[name].shape
                       and a.tobytes() == theirs[name].tobytes())]
  assert not differing, '%s: the IoStream call differs from the IoCached call in %s' % (case_id, differing)


# ---------------------------------------------------------------------------------------------------------------------
# 4. batch invariance
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('family,fmt', [(f, fmt) for f, fmts in pm.RAGGED_FORMATS.items() for fmt in fmts],
                         ids=lambda v: pm.FMT_NAME[v] if isinstance(v, int) else v)
def test_an_image_is_the_same_in_an_all_vector_and_in_a_mixed_launch(family, fmt, gpu_device):
  """V and Q sit in both fp16 launches with the same rows: ANY_SLOW = false against ANY_SLOW = true"""
  ids = ['%s-f16-%s-%s' % (family, pm.FMT_NAME[fmt], launch) for launch in ('vector', 'mixed')]
  vector, mixed = (parent_outputs(i, gpu_device) for i in ids)
  shared = sorted(set(pm.case_images(pm.BY_ID[ids[0]])) & set(pm.case_images(pm.BY_ID[ids[1]])))
  assert shared == ['Q', 'V']
  for key in shared:
    for name in ['%s.y' % key] + (['%s.tap' % key] if fmt != pm.TAP_NONE else []):
      assert vector[name].tobytes() == mixed[name].tobytes(), '%s %s' % (ids, name)
