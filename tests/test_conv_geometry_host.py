"""CPU: the geometry cases of tests/test_hip_conv_geometry.py reach what they are there for.  From the
Python restatement of csrc/conv_ops.hip's host side (tests/_conv_plan_ref.py): the table reaches every required cell, no
case is redundant, every non-square case would reject a kernel that read h as w -- through the assertion helper the GPU
test uses -- and the restated refusals are the library's own where it is built."""
import ctypes
import os

import pytest
import torch

from tests import _conv_plan_ref as R


def test_the_table_reaches_every_required_cell():
  run = R.cells_run()
  missing = [c for c in R.REQUIRED_CELLS if c not in run]
  assert not missing, missing
  assert len(set(R.REQUIRED_CELLS)) == len(R.REQUIRED_CELLS) and len(set(R.CASE_IDS)) == len(R.CASE_IDS)


def test_no_case_is_redundant():
  """dropping any one case loses a required cell"""
  required = set(R.REQUIRED_CELLS)
  for case in R.CASES:
    rest = R.cells_run([c for c in R.CASES if c is not case])
    assert (R.case_cells(case) - rest) & required, case['id']


def test_the_shift_counts_of_conv_dims():
  d = R.conv_dims(2, 16, 8, 32, 64)
  assert (d['ho'], d['wo'], d['sh_w'], d['sh_hw'], d['m']) == (8, 4, 2, 5, 64)
  d = R.conv_dims(2, 8, 16, 32, 64)
  assert (d['sh_w'], d['sh_hw']) == (3, 5)  # log2 wo != log2 ho: sh_hw - sh_w is the row count's, not the column count's
  for dims in ((3, 8, 12, 5, 7), (2, 12, 8, 5, 7), (1, 24, 12, 6, 36)):
    d = R.conv_dims(*dims)
    assert (d['sh_w'], d['sh_hw']) == (-1, -1)
  assert R.split_mode(R.conv_dims(2, 2, 6, 3, 1)) == 'div, wo not 2^k'  # one output row: ho = 1 IS a power of two


def test_the_row_staged_kernel_its_row_counts_and_near_misses():
  plans = {c['dims']: R.fwd_plan(*c['dims']) for c in R.cases_of('fwd')}
  assert {(p['kernel'], p.get('rows')) for p in plans.values()} >= {('rows', 4), ('rows', 8), ('flat', None)}
  assert plans[(2, 8, 64, 14, 32)]['rows'] == 4 and plans[(1, 24, 64, 17, 32)]['blocks_per_image'] == 3
  assert plans[(1, 16, 64, 6, 20)]['rows'] == 8
  assert plans[(1, 4, 64, 14, 32)]['kernel'] == 'flat'   # ho = 2: not a multiple of four rows
  assert plans[(1, 64, 8, 14, 32)]['kernel'] == 'flat' and R.fwd_plan(1, 8, 64, 14, 32)['kernel'] == 'rows'  # transposed
  for dims, p in plans.items():
    if p['kernel'] == 'rows':  # a forced plan keeps the kernel out, tile code 6 asks for it, a misaligned x excludes it
      assert R.fwd_plan(*dims, tuning=(5, 1, 0))['kernel'] == 'flat' and R.fwd_plan(*dims, tuning=(6, 0, 0))['kernel'] == 'rows'
      assert R.fwd_plan(*dims, x_aligned=False)['kernel'] == 'flat' and p['lds'] <= R.LDS_LIMIT
  p = R.planes_plan(*R.cases_of('planes')[0]['dims'])
  assert p['rows'] == 4 and p['blocks_per_image'] > 1
  assert R.planes_plan(*R.cases_of('pair_planes')[0]['dims'])['rows'] == 4
  assert 'refused' in R.planes_plan(1, 4, 64, 14, 32) and 'refused' in R.planes_plan(1, 64, 8, 14, 32)


def test_the_small_kernel_its_geometries_and_the_lds_limit():
  small = [c['dims'] for c in R.cases_of('bwd') if R.bwd_data_plan(*c['dims'])['kernel'] == 'small']
  geo = {(d[2] // 2, d[4]) for d in small} - {(32, 32)}
  assert len(geo) >= 2 and any(wo & (wo - 1) for wo, _ in geo) and any(co == 36 for _, co in geo), geo
  # either side of the limit at cout = 64, from the restated formula: the last width that fits, the next even one that does not
  fit, miss = R.SMALL_FIT_W, R.SMALL_MISS_W
  assert miss == fit + 2 and (1, 8, fit, 6, 64) in small
  assert R.small_lds(R.conv_dims(1, 8, fit, 6, 64)) <= R.LDS_LIMIT < R.small_lds(R.conv_dims(1, 8, miss, 6, 64))
  p = R.bwd_data_plan(1, 8, miss, 6, 64)
  assert p['kernel'] == 'flat' and p['small_lds'] > R.LDS_LIMIT
  for dims in small:  # a forced plan and a misaligned dy both take the flat kernel: the comparison the GPU test makes
    assert R.bwd_data_plan(*dims, tuning=(0, 1, 1))['kernel'] == 'flat'
    assert R.bwd_data_plan(*dims, dy_aligned=False)['kernel'] == 'flat'


def test_the_weight_gradient_with_and_without_its_reduce_launch():
  ps = {c['dims']: R.wrw_launch(*c['dims']) for c in R.cases_of('wrw')}
  assert any(p['reduce'] for p in ps.values()) and any(not p['reduce'] for p in ps.values())
  assert all(R.wrw_launch(*d, tuning=(1, 1))['p'] == 1 for d in ps) and R.wrw_launch(3, 8, 12, 5, 8, tuning=(4, 7))['p'] > 1
  assert all(d in ps for d in R.WRW_GROUP) and len({d[1:3] for d in R.WRW_GROUP}) == 3
  assert {ps[d]['reduce'] for d in R.WRW_GROUP} == {True, False}  # the grouped call defers some reduce launches, not all


NON_SQUARE = [c['id'] for c in R.CASES if R.non_square(c)]


def test_every_case_but_none_is_non_square():
  assert len(NON_SQUARE) == len(R.CASES)


@pytest.mark.parametrize('cid', NON_SQUARE)
def test_an_h_w_swap_would_be_rejected(cid):
  """liveness: the float64 reference of the case against the float64 result of the WRONG reading -- the same memory taken
  as (n, w, h, cin), the result's memory read back in the true shape.  They differ by more than 1000 x the GPU bound at most
  positions, and the GPU test's own assertion rejects the wrong reading."""
  case = R.BY_ID[cid]
  x, w, _, dy = R.case_operands(case)
  ref = dict(zip(('y', 'dx', 'dw'), R.reference(x, w, dy)))
  wrong = dict(zip(('y', 'dx', 'dw'), R.swapped_reference(x, w, dy)))
  for name, bound in R.FAMILY_OUTPUTS[case['family']]:
    scale = float(ref[name].abs().max())
    far = float(((wrong[name] - ref[name]).abs() > 1000 * bound * scale).double().mean())
    assert far > 0.5, (cid, name, far)
    with pytest.raises(AssertionError):
      R.assert_close(wrong[name], ref[name], bound, cid)
    R.assert_close(ref[name].float(), ref[name], bound, cid)  # (and passes what float32 rounding of the truth gives)


def test_the_restated_refusals():
  for entry, dims, kw in R.REFUSALS:
    assert 'refused' in R.refusal_plan(entry, dims, kw), (entry, dims, kw)
  # what is NOT refused: a misaligned x, dy (the kernel choice changes instead), an empty batch
  assert R.fwd_plan(2, 8, 12, 5, 7, x_aligned=False)['kernel'] == 'flat'
  assert R.bwd_data_plan(2, 8, 16, 6, 8, dy_aligned=False)['kernel'] == 'flat'
  assert R.fwd_plan(0, 8, 12, 5, 7)['kernel'] is None and R.bwd_data_plan(0, 8, 12, 5, 8)['kernel'] is None
  assert R.wrw_launch(0, 8, 12, 5, 8)['kernel'] == 'memset' and R.wrw_launch(0, 8, 6, 5, 8)['kernel'] == 'memset'


A, M = 0x10000, 0x10004  # made-up addresses, 16-byte aligned and one float in: a refusal returns before anything reads them


def _call(lib, entry, dims, kw):
  n, h, w, cin, cout = dims
  vp = ctypes.c_void_p
  if entry == 'fwd':
    return lib.expo_conv4x4s2_fwd(vp(A), vp(A if kw.get('w_aligned', True) else M), None, vp(A), n, h, w, cin, cout, 0, 0.2, None)
  if entry == 'fwd_pair':
    xb = A if kw.get('pair_same_alignment', True) else M
    wb = A if kw.get('pair_w_aligned', True) else M
    return lib.expo_conv4x4s2_fwd_pair(vp(A), vp(A), None, vp(A), vp(xb), vp(wb), None, vp(A), n, h, w, cin, cout, 0, 0.2, None)
  if entry == 'bwd':
    return lib.expo_conv4x4s2_bwd_data(vp(A), vp(A), vp(A), n, h, w, cin, cout, None)
  if entry == 'bwd_pair':
    return lib.expo_conv4x4s2_bwd_data_mask_pair(vp(A), vp(A), vp(A), vp(A), vp(M), vp(A), vp(A), vp(A), n, h, w, cin, cout, 0.2, None)
  if entry == 'wrw':
    return lib.expo_conv4x4s2_wrw(vp(A), vp(A), vp(A if kw.get('dw_aligned', True) else M), n, h, w, cin, cout, None, 0, None)
  assert entry == 'wrw_bias'
  return lib.expo_conv4x4s2_wrw_bias(vp(A), vp(A), vp(A), vp(A if kw.get('dbias_aligned', True) else M), n, n, h, w, cin, cout,
                                     None, 0, None)


def test_the_library_refuses_what_the_restatement_refuses():
  """the refusals return before any launch: checked against the C entry points with made-up addresses, no GPU needed"""
  from exposure_amd import _cabi
  if not os.path.exists(_cabi.LIB_PATH):
    pytest.skip('the library is not built')
  lib = _cabi.load()
  for entry, dims, kw in R.REFUSALS:
    assert _call(lib, entry, dims, kw) == -1, (entry, dims, kw)
    assert (lib.expo_last_error() or b'').decode() == R.refusal_plan(entry, dims, kw)['refused'], (entry, dims, kw)
  # an empty batch returns before the pointers are looked at (forward, data gradient: no launch, nothing written)
  assert lib.expo_conv4x4s2_fwd(None, None, None, None, 0, 8, 12, 5, 7, 0, 0.2, None) == 0
  assert lib.expo_conv4x4s2_bwd_data(None, None, None, 0, 8, 12, 5, 6, None) == 0
  assert lib.expo_conv4x4s2_wrw_workspace_bytes(0, 8, 12, 5, 8) == 0
  # the workspace the weight gradient asks for is P copies (dw + the padded bias tail) where the restatement says P > 1
  for c in R.cases_of('wrw'):
    n, h, w, cin, cout = c['dims']
    p = R.wrw_launch(*c['dims'])['p']
    want = p * (cout * 16 * cin + (cout + 3) // 4 * 4) * 4 if p > 1 else 0
    assert lib.expo_conv4x4s2_wrw_workspace_bytes(n, h, w, cin, cout) == want, c['id']
