"""GPU: the convolution kernels of csrc/conv_ops.hip on non-square, odd-row and misaligned inputs -- the
geometries the C ABI promises and the 64 x 64 training workload never takes.  The cases come from tests/_conv_plan_ref.py,
whose host test proves which kernel, row count, split_pixel path and LDS layout each of them reaches; every result is held
to float64 (F.conv2d on the CPU and its autograd) at the project's own bounds, and every output is a view into a guarded
buffer: the kernels write all of it and nothing else."""
import pytest
import torch

from exposure_amd import _cabi, nn_ops
from tests import _conv_plan_ref as R
from tests.test_hip_fused_decode import guarded, guards_intact

pytestmark = pytest.mark.gpu

F32 = torch.float32
NAN = float('nan')


def out(shape, off=0):
  """(buffer, view): an output of `shape` between guard elements, pre-filled with NaN, `off` floats into its allocation"""
  buf, t = guarded(shape, F32, off)
  t.fill_(NAN)
  return buf, t


def out_w(shape, off=0):
  """the same for a (cout, cin, 4, 4) gradient in channels_last memory order"""
  cout, cin = shape[:2]
  buf, t = out((cout, 4, 4, cin), off)
  return buf, t.permute(0, 3, 1, 2)


def intact(*pairs):
  for buf, t in pairs:
    assert guards_intact(buf, t, F32), 'a write outside the output'


def placed(t, off):
  """a contiguous copy of `t` whose base lies `off` floats into its allocation"""
  if t.dim() == 4 and not t.is_contiguous():  # a weight: channels_last memory order
    _, v = guarded(tuple(t.permute(0, 2, 3, 1).shape), F32, off)
    v = v.permute(0, 3, 1, 2)
  else:
    _, v = guarded(tuple(t.shape), F32, off)
  v.copy_(t)
  assert (v.data_ptr() % 16 != 0) == (off % 4 != 0)
  return v


def lrelu64(v, leak=0.2):
  return torch.where(v > 0, v, v * leak)


def with_zeros(shape, dev, seed, every):
  z = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
  z.view(-1)[::every] = 0.0  # exact zeros: TF's sub-gradient (1 + leak) / 2
  return z


def yshape(dims):
  n, h, w, _, cout = dims
  return (n, h // 2, w // 2, cout)


@pytest.mark.parametrize('cid', R.ids_of('fwd'))
def test_forward_matches_float64(cid, gpu_device):
  """expo_conv4x4s2_fwd plain and with bias + lrelu, expo_conv4x4s2_fwd_mask into a separate tensor and in place, under every
  decomposition of test_hip_conv_forward_matches_float64"""
  dims = R.BY_ID[cid]['dims']
  x, w, b, dy = R.case_operands(R.BY_ID[cid], gpu_device)
  ref = R.reference(x, w, dy)[0]
  scale = float(ref.abs().max())
  want_act = lrelu64(ref + b.double().cpu())
  z = with_zeros(yshape(dims), gpu_device, 7, 5)
  want_mask = ref * R.slope(z).double().cpu()
  worst = [0.0, 0.0]
  try:
    for tuning in R.FWD_VARIANTS:
      _cabi.conv_tuning(*tuning)
      for act in (0, 1):
        buf, y = out(yshape(dims))
        _cabi.conv4x4s2_fwd(x, w, b if act else None, y, act, 0.2)
        intact((buf, y))
        worst[0] = max(worst[0], R.assert_close(y, want_act if act else ref, R.BOUND_FWD, (cid, tuning, act), scale=scale))
      buf, y = out(yshape(dims))
      _cabi.conv4x4s2_fwd_mask(x, w, z, y, 0.2)
      intact((buf, y))
      worst[1] = max(worst[1], R.assert_close(y, want_mask, R.BOUND_BWD, (cid, tuning, 'mask')))
      zbuf, zz = guarded(yshape(dims), F32)
      zz.copy_(z)
      _cabi.conv4x4s2_fwd_mask(x, w, zz, zz, 0.2)
      intact((zbuf, zz))
      assert torch.equal(zz, y), (cid, tuning, 'mask in place')
  finally:
    _cabi.conv_tuning(0, 0, 0)
  print('conv geometry fwd %s (%s): worst %.2e, masked %.2e of max |y| over %d plans' %
        (cid, R.fwd_plan(*dims)['kernel'], worst[0], worst[1], len(R.FWD_VARIANTS)))


@pytest.mark.parametrize('cid', R.ids_of('bwd'))
def test_data_gradient_matches_float64(cid, gpu_device):
  """expo_conv4x4s2_bwd_data and _bwd_data_mask (z with exact zeros) under every (channel tiles, K' slices) plan; where the
  library's own choice is the vector-ALU kernel, the forced matrix-core plan must agree with it"""
  dims = R.BY_ID[cid]['dims']
  x, w, _, dy = R.case_operands(R.BY_ID[cid], gpu_device)
  ref = R.reference(x, w, dy)[1]
  scale = float(ref.abs().max())
  z = with_zeros(x.shape, gpu_device, 11, 7)
  want_mask = ref * R.slope(z).double().cpu()
  kept, worst = {}, 0.0
  try:
    for tuning in R.BWD_VARIANTS:
      _cabi.conv_tuning(*tuning)
      buf, dx = out(x.shape)
      _cabi.conv4x4s2_bwd_data(dy, w, dx)
      intact((buf, dx))
      worst = max(worst, R.assert_close(dx, ref, R.BOUND_BWD, (cid, tuning)))
      mbuf, dm = out(x.shape)
      _cabi.conv4x4s2_bwd_data_mask(dy, w, z, dm, 0.2)
      intact((mbuf, dm))
      assert torch.equal(dm, dx * R.slope(z)), (cid, tuning, 'mask')
      R.assert_close(dm, want_mask, R.BOUND_BWD, (cid, tuning, 'mask'), scale=scale)
      kept[tuning] = dx
  finally:
    _cabi.conv_tuning(0, 0, 0)
  kernel = R.bwd_data_plan(*dims)['kernel']
  if kernel == 'small':  # (0, 1, 1) is the flat kernel: the two kernels on the same problem
    assert R.bwd_data_plan(*dims, tuning=(0, 1, 1))['kernel'] == 'flat'
    assert float((kept[(0, 1, 1)] - kept[(0, 0, 0)]).abs().max()) / scale < R.BOUND_BWD, cid
  print('conv geometry bwd %s (%s): worst %.2e of max |dx| over %d plans' % (cid, kernel, worst, len(R.BWD_VARIANTS)))


@pytest.mark.parametrize('cid', R.ids_of('wrw'))
def test_weight_gradient_matches_float64(cid, gpu_device):
  """expo_conv4x4s2_wrw and _wrw_bias (the first 0, some, all images' bias gradient) under the splits of the existing test,
  each call twice: bit-reproducible"""
  dims = R.BY_ID[cid]['dims']
  n, cout = dims[0], dims[4]
  x, w, _, dy = R.case_operands(R.BY_ID[cid], gpu_device)
  ref = R.reference(x, w, dy)[2]
  worst = [0.0, 0.0]
  try:
    for split in R.WRW_SPLITS:
      _cabi.conv_wrw_tuning(*split)
      runs = []
      for _ in range(2):
        buf, dw = out_w(w.shape)
        _cabi.conv4x4s2_wrw(x, dy, dw)
        intact((buf, dw))
        worst[0] = max(worst[0], R.assert_close(dw, ref, R.BOUND_WRW, (cid, split)))
        runs.append(dw)
      assert torch.equal(runs[0], runs[1]), (cid, split)
      for k in sorted({0, (2 * n) // 3, n}):
        runs = []
        for _ in range(2):
          buf, dw = out_w(w.shape)
          bbuf, db = out((cout,))
          _cabi.conv4x4s2_wrw_bias(x, dy, dw, db, k)
          intact((buf, dw), (bbuf, db))
          R.assert_close(dw, ref, R.BOUND_WRW, (cid, split, k))
          worst[1] = max(worst[1], R.assert_bias_close(db, dy, k, (cid, split)))
          runs.append((dw, db))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (cid, split, k)
  finally:
    _cabi.conv_wrw_tuning(0, 0)
  print('conv geometry wrw %s (P %d): worst %.2e of max |dw|, bias %.2e absolute' % (cid, R.wrw_launch(*dims)['p'], worst[0], worst[1]))


def test_grouped_weight_gradients_of_three_geometries(gpu_device):
  """one expo_conv4x4s2_wrw_group call over three non-square layers of different geometry (with and without a reduce launch,
  with and without a bias gradient) == the single calls, bit for bit"""
  items, singles, bufs = [], [], []
  for i, dims in enumerate(R.WRW_GROUP):
    n = dims[0]
    x, w, _, dy = R.make_operands(dims, 40 + i, gpu_device)
    k = (None, None, (2 * n) // 3)[i]
    row = []
    for _ in range(2):
      dwb = out_w(w.shape)
      dbb = out((dims[4],)) if i != 1 else None
      row.append((dwb, dbb))
      bufs += [dwb] + ([dbb] if dbb else [])
    (ga, gb), (sa, sb) = row
    items.append((x, dy, ga[1], gb[1] if gb else None, k))
    if sb:
      _cabi.conv4x4s2_wrw_bias(x, dy, sa[1], sb[1], k)
    else:
      _cabi.conv4x4s2_wrw(x, dy, sa[1])
    singles.append((ga, gb, sa, sb, x, w, dy))
  _cabi.conv4x4s2_wrw_group(items)
  intact(*bufs)
  for ga, gb, sa, sb, x, w, dy in singles:
    assert torch.equal(ga[1], sa[1]) and (gb is None or torch.equal(gb[1], sb[1]))
    R.assert_close(ga[1], R.reference(x, w, dy)[2], R.BOUND_WRW, tuple(x.shape))


def test_pairs_equal_their_single_calls(gpu_device):
  """expo_conv4x4s2_fwd_pair, _bwd_data_mask_pair and _fwd_planes_pair on one non-square case each == the two single calls,
  bit for bit (the restated plans say that the pair's K slicing is the single call's at these sizes) and float64"""
  dev = gpu_device
  case = R.cases_of('pair_fwd')[0]
  dims = case['dims']
  assert R.fwd_plan(*dims, pair=True)['s'] == R.fwd_plan(*dims)['s']
  ops = [R.case_operands(case, dev), R.make_operands(dims, 71, dev)]
  want, got = [out(yshape(dims)) for _ in ops], [out(yshape(dims)) for _ in ops]
  for (x, w, b, _), (_, y) in zip(ops, want):
    _cabi.conv4x4s2_fwd(x, w, b, y, 1, 0.2)
  _cabi.conv4x4s2_fwd_pair(*[(x, w, b, y) for (x, w, b, _), (_, y) in zip(ops, got)], 1, 0.2)
  intact(*got)
  for (x, w, b, dy), (_, y), (_, y1) in zip(ops, got, want):
    assert torch.equal(y, y1)
    R.assert_close(y, lrelu64(R.reference(x, w, dy)[0] + b.double().cpu()), R.BOUND_FWD, case['id'])

  case = R.cases_of('pair_bwd')[0]
  dims = case['dims']
  assert R.bwd_data_plan(*dims, pair=True)['s'] == R.bwd_data_plan(*dims)['s']
  ops = [R.case_operands(case, dev), R.make_operands(dims, 72, dev)]
  zs = [with_zeros(o[0].shape, dev, 5 + i, 7) for i, o in enumerate(ops)]
  want, got = [out(o[0].shape) for o in ops], [out(o[0].shape) for o in ops]
  for (x, w, _, dy), z, (_, dx) in zip(ops, zs, want):
    _cabi.conv4x4s2_bwd_data_mask(dy, w, z, dx, 0.2)
  _cabi.conv4x4s2_bwd_data_mask_pair(*[(dy, w, z, dx) for (x, w, _, dy), z, (_, dx) in zip(ops, zs, got)], 0.2)
  intact(*got)
  for (x, w, _, dy), z, (_, dx), (_, dx1) in zip(ops, zs, got, want):
    assert torch.equal(dx, dx1)
    R.assert_close(dx, R.reference(x, w, dy)[1] * R.slope(z).double().cpu(), R.BOUND_BWD, case['id'])

  case = R.cases_of('pair_planes')[0]
  dims = case['dims']
  x, w, b, dy = R.case_operands(case, dev)
  _, w2, b2, _ = R.make_operands(dims, 73, dev)
  want, got = [out(yshape(dims)) for _ in range(2)], [out(yshape(dims)) for _ in range(2)]
  for (ww, bb), (_, y) in zip(((w, b), (w2, b2)), want):
    _cabi.conv4x4s2_fwd_planes(x, ww, bb, y, 1, 0.2)
  _cabi.conv4x4s2_fwd_planes_pair((x, w, b, got[0][1]), (x, w2, b2, got[1][1]), 1, 0.2)
  intact(*got)
  for (ww, bb), (_, y), (_, y1) in zip(((w, b), (w2, b2)), got, want):
    assert torch.equal(y, y1)
    R.assert_close(y, lrelu64(R.reference(x, ww, dy)[0] + bb.double().cpu()), R.BOUND_PLANES, case['id'])


@pytest.mark.parametrize('cid', R.ids_of('planes'))
def test_planes_kernel_with_four_rows_per_block(cid, gpu_device):
  """expo_conv4x4s2_fwd_planes where ho is no multiple of eight (rows = 4, three blocks per image): bias + lrelu, and the
  tangent pass in place, as test_first_layer_with_its_constant_planes_folded compares them"""
  case = R.BY_ID[cid]
  dims = case['dims']
  assert R.planes_plan(*dims)['rows'] == 4
  x, w, b, dy = R.case_operands(case, gpu_device)
  ref = R.reference(x, w, dy)[0]
  buf, y = out(yshape(dims))
  _cabi.conv4x4s2_fwd_planes(x, w, b, y, 1, 0.2)
  intact((buf, y))
  e1 = R.assert_close(y, lrelu64(ref + b.double().cpu()), R.BOUND_PLANES, cid)
  z = with_zeros(yshape(dims), gpu_device, 3, 9)
  tbuf, t = guarded(yshape(dims), F32)
  t.copy_(z)
  _cabi.conv4x4s2_fwd_planes(x, w, None, t, 0, 0.2, zmask=t)
  intact((tbuf, t))
  e2 = R.assert_close(t, ref * R.slope(z).double().cpu(), R.BOUND_PLANES, (cid, 'tangent'))
  print('conv geometry planes %s: %.2e, tangent %.2e of max |y|' % (cid, e1, e2))


@pytest.mark.parametrize('off', R.OFFSETS)
@pytest.mark.parametrize('cid', R.ids_of('misaligned'))
def test_operands_that_are_not_16_byte_aligned(cid, off, gpu_device):
  """x, then dy, then y / dx (and the masks with them) 1, 2, 3 floats into their allocations: the header asks alignment of
  w, dw and dbias only.  A misaligned x keeps the row-staged kernel out, a misaligned dy the vector-ALU kernel; the CIN4
  kernels issue 16-byte buffer loads from a dword-aligned base."""
  dims = R.BY_ID[cid]['dims']
  x, w, b, dy = R.case_operands(R.BY_ID[cid], gpu_device)
  y64, dx64, dw64 = R.reference(x, w, dy)
  zy, zx = with_zeros(yshape(dims), gpu_device, 7, 5), with_zeros(x.shape, gpu_device, 11, 7)
  xm, dym = placed(x, off), placed(dy, off)
  assert xm.data_ptr() % 16 and dym.data_ptr() % 16
  want_act, want_ymask, want_xmask = lrelu64(y64 + b.double().cpu()), y64 * R.slope(zy).double().cpu(), dx64 * R.slope(zx).double().cpu()
  scale = float(y64.abs().max())
  worst = 0.0
  for xx, yoff in ((xm, 0), (x, off)):  # the input misaligned, then the output (and the mask read in place)
    buf, y = out(yshape(dims), yoff)
    assert (y.data_ptr() % 16 != 0) == (yoff != 0)
    _cabi.conv4x4s2_fwd(xx, w, b, y, 1, 0.2)
    intact((buf, y))
    worst = max(worst, R.assert_close(y, want_act, R.BOUND_FWD, (cid, off, yoff), scale=scale))
    buf, y = guarded(yshape(dims), F32, yoff)
    y.copy_(zy)
    _cabi.conv4x4s2_fwd_mask(xx, w, y, y, 0.2)
    intact((buf, y))
    worst = max(worst, R.assert_close(y, want_ymask, R.BOUND_BWD, (cid, off, yoff, 'mask')))
  for gg, xoff in ((dym, 0), (dy, off)):
    buf, dx = out(x.shape, xoff)
    _cabi.conv4x4s2_bwd_data(gg, w, dx)
    intact((buf, dx))
    worst = max(worst, R.assert_close(dx, dx64, R.BOUND_BWD, (cid, off, xoff, 'dx')))
    buf, dx = out(x.shape, xoff)
    _cabi.conv4x4s2_bwd_data_mask(gg, w, placed(zx, xoff), dx, 0.2)
    intact((buf, dx))
    worst = max(worst, R.assert_close(dx, want_xmask, R.BOUND_BWD, (cid, off, xoff, 'dx mask')))
  buf, dw = out_w(w.shape)  # (the weight gradient reads x and dy through buffer loads too)
  bbuf, db = out((dims[4],))
  _cabi.conv4x4s2_wrw_bias(xm, dym, dw, db)
  intact((buf, dw), (bbuf, db))
  R.assert_close(dw, dw64, R.BOUND_WRW, (cid, off, 'dw'))
  R.assert_bias_close(db, dy, dims[0], (cid, off))
  print('conv geometry misaligned %s + %d floats: worst %.2e of the bound\'s scale' % (cid, off, worst))


def test_refusals_leave_the_outputs_untouched(gpu_device):
  """every refusal raises ExposureHipError before anything is launched: the guarded outputs keep their NaN fill"""
  dev = gpu_device
  base = (2, 8, 12, 5, 8)
  x, w, b, dy = R.make_operands(base, 5, dev)
  x2, w2, b2, dy2 = R.make_operands(base, 6, dev)
  z, z2 = with_zeros(x.shape, dev, 1, 7), with_zeros(x.shape, dev, 2, 7)

  def refused(call, *outs):
    with pytest.raises(_cabi.ExposureHipError):
      call()
    torch.cuda.synchronize()
    for buf, t in outs:
      assert bool(torch.isnan(t).all()) and guards_intact(buf, t, F32)

  y, ya = out(yshape(base)), out(yshape(base))
  refused(lambda: _cabi.conv4x4s2_fwd(x, placed(w, 1), b, y[1], 1, 0.2), y)
  refused(lambda: _cabi.conv4x4s2_fwd_pair((x, w, b, y[1]), (x2, placed(w2, 1), b2, ya[1]), 1, 0.2), y, ya)
  refused(lambda: _cabi.conv4x4s2_fwd_pair((x, w, b, y[1]), (placed(x2, 1), w2, b2, ya[1]), 1, 0.2), y, ya)
  dx, dxa = out(x.shape), out(x.shape)
  refused(lambda: _cabi.conv4x4s2_bwd_data_mask_pair((dy, w, z, dx[1]), (placed(dy2, 2), w2, z2, dxa[1]), 0.2), dx, dxa)
  dw, db = out_w(w.shape), out((base[4],))
  dw1, db1 = out_w(w.shape, 1), out((base[4],), 1)
  refused(lambda: _cabi.conv4x4s2_wrw(x, dy, dw1[1]), dw1)
  refused(lambda: _cabi.conv4x4s2_wrw_bias(x, dy, dw1[1], db[1]), dw1, db)
  refused(lambda: _cabi.conv4x4s2_wrw_bias(x, dy, dw[1], db1[1]), dw, db1)
  # cout % 4 != 0: the data gradient, the bias gradient
  odd = (2, 8, 12, 5, 6)
  xo, wo, _, dyo = R.make_operands(odd, 7, dev)
  dxo, dwo, dbo = out(xo.shape), out_w(wo.shape), out((6,))
  refused(lambda: _cabi.conv4x4s2_bwd_data(dyo, wo, dxo[1]), dxo)
  refused(lambda: _cabi.conv4x4s2_bwd_data_mask(dyo, wo, z, dxo[1], 0.2), dxo)
  refused(lambda: _cabi.conv4x4s2_wrw_bias(xo, dyo, dwo[1], dbo[1]), dwo, dbo)
  # w / 2 odd: the weight gradient consumes pixels in pairs
  xp, wp, _, dyp = R.make_operands((2, 8, 6, 5, 8), 8, dev)
  dwp = out_w(wp.shape)
  refused(lambda: _cabi.conv4x4s2_wrw(xp, dyp, dwp[1]), dwp)
  # odd h, odd w
  for n, h, wd, cin, cout in ((2, 7, 12, 5, 8), (2, 8, 11, 5, 8)):
    xq = torch.randn((n, h, wd, cin), device=dev)
    gq = torch.randn((n, h // 2, wd // 2, cout), device=dev)
    yq, dxq, dwq = out(tuple(gq.shape)), out(tuple(xq.shape)), out_w(w.shape)
    refused(lambda: _cabi.conv4x4s2_fwd(xq, w, b, yq[1], 1, 0.2), yq)
    refused(lambda: _cabi.conv4x4s2_bwd_data(gq, w, dxq[1]), dxq)
    refused(lambda: _cabi.conv4x4s2_wrw(xq, gq, dwq[1]), dwq)


def test_empty_batches(gpu_device):
  """n = 0: the forward and the data gradient return without a launch (nothing around the empty output is written); the
  weight gradient leaves dw and dbias exactly zero"""
  dev = gpu_device
  _, w, b, _ = R.make_operands((1, 8, 12, 5, 8), 9, dev)
  x, dy = torch.empty((0, 8, 12, 5), device=dev), torch.empty((0, 4, 6, 8), device=dev)
  # (an empty view has no address of its own: the whole buffer around it must keep its fill)
  y, dx = guarded((0, 4, 6, 8), F32), guarded((0, 8, 12, 5), F32)
  before = [t[0].clone() for t in (y, dx)]
  _cabi.conv4x4s2_fwd(x, w, b, y[1], 1, 0.2)
  _cabi.conv4x4s2_bwd_data(dy, w, dx[1])
  assert torch.equal(y[0], before[0]) and torch.equal(dx[0], before[1])
  dw, db, dw2 = out_w(w.shape), out((8,)), out_w(w.shape)
  _cabi.conv4x4s2_wrw_bias(x, dy, dw[1], db[1])
  _cabi.conv4x4s2_wrw(x, dy, dw2[1])
  intact(dw, db, dw2)
  for _, t in (dw, db, dw2):
    assert bool((t == 0).all())


def test_fused_conv_layer_autograd_on_a_non_square_input(gpu_device):
  """nn_ops.conv_bias_lrelu at (3, 8, 24, 14, 32): value, gx, gw, gb and the gradient penalty's double backward against the
  same layer in float64 on the CPU, at the bound of test_fused_conv_layer_autograd_matches_the_library_pair"""
  case = R.cases_of('layer')[0]
  x0, w0, b0, c = R.case_operands(case, gpu_device)
  res = []
  for hip in (True, False):
    cast = (lambda t: t.clone()) if hip else (lambda t: t.double().cpu())
    x, w, b = [cast(t).requires_grad_(True) for t in (x0, w0, b0)]
    if hip:
      z = nn_ops.conv_bias_lrelu(x, w, b)
    else:
      y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, None, 2, 1).permute(0, 2, 3, 1) + b
      z = 0.6 * y + 0.4 * y.abs()  # util.py:225-229
    gx, gw, gb = torch.autograd.grad((z * cast(c)).sum(), [x, w, b], create_graph=True)
    ggw, = torch.autograd.grad((gx**2).sum(), [w])
    res.append([t.detach() for t in (z, gx, gw, gb, ggw)])
  errs = [R.assert_close(a, r, R.BOUND_LAYER, name, atol=1e-7) for name, a, r in zip(('z', 'gx', 'gw', 'gb', 'ggw'), *res)]
  print('conv geometry layer %s: z %.1e gx %.1e gw %.1e gb %.1e ggw %.1e of each maximum' % ((case['id'],) + tuple(errs)))
