"""The host side of csrc/conv_ops.hip restated in Python: which kernel conv_fwd_impl,
conv_fwd_planes_impl, conv_bwd_data_impl and conv_wrw_impl launch for a geometry, an operand alignment, a pair call and a
forced plan -- conv_dims with its shift counts, flat_plan / bwd_plan / wrw_plan, both LDS formulas, the refusals -- and the
table of geometry cases that tests/test_hip_conv_geometry.py runs.  Pure functions: tests/test_conv_geometry_host.py proves
on a machine without a GPU that the table reaches every cell of REQUIRED_CELLS, that no case is redundant and that every
non-square case would reject a kernel that read h as w.  The comparison helpers the GPU tests assert with live here too, so
that the liveness test runs through the very same assertions."""
import torch
import torch.nn.functional as F

LDS_LIMIT = 160 * 1024

# the project's bounds (tests/test_nn_ops.py, tests/test_critic_direct.py): of max |reference|
BOUND_FWD = 2e-6
BOUND_BWD = 3e-6   # the data gradient and the masked forward
BOUND_WRW = 1e-5
BOUND_BIAS = 1e-5  # of the largest per-channel sum of |dy|
BOUND_PLANES = 4 * 2e-6  # expo_conv4x4s2_fwd_planes, as test_first_layer_with_its_constant_planes_folded holds it

# the plans the forward cases run under (test_hip_conv_forward_matches_float64's list) as (tile, nt, slices)
FWD_VARIANTS = ([(0, 0, 0)] + [(5, nt, sl) for nt in (1, 2) for sl in (0, 1, 2, 4, 8, 16)] +
                [(t, 0, 0) for t in (1, 2, 3, 4, 6)])
BWD_VARIANTS = [(0, nt, sl) for nt in (0, 1, 2) for sl in (0, 1, 2, 4, 8, 16)]
WRW_SPLITS = ((0, 0), (1, 1), (2, 3), (4, 0), (4, 7), (3, 2))  # (waves per block, blocks per tile) of the existing test
TILED = {1: (64, 32), 2: (64, 64), 3: (32, 64), 4: (32, 32)}   # shape -> (BM, BN)


def _cdiv(a, b):
  return (a + b - 1) // b


def _pow2(v):
  return v >= 1 and (v & (v - 1)) == 0


# ---- conv_dims ----------------------------------------------------------------------------------------------------------
def conv_dims(n, h, w, cin, cout):
  """ConvDims as a dict, or the refusal's text"""
  if n < 0 or h < 2 or w < 2 or (h & 1) or (w & 1) or cin < 1 or cout < 1:
    return 'conv4x4s2: n >= 0, even h, w >= 2, cin, cout >= 1 required'
  if n * h * w * cin * 4 > 2.0e9 or n * (h // 2) * (w // 2) * cout * 4 > 2.0e9 or cout * 16 * cin * 4 > 2.0e9:
    return 'conv4x4s2: a tensor of 2 GB or more is not supported'
  d = dict(n=n, h=h, w=w, cin=cin, cout=cout, ho=h // 2, wo=w // 2, kdim=16 * cin, sh_w=-1, sh_hw=-1)
  d['m'] = n * d['ho'] * d['wo']
  if _pow2(d['wo']) and _pow2(d['ho']):
    d['sh_w'] = d['wo'].bit_length() - 1
    d['sh_hw'] = d['sh_w'] + d['ho'].bit_length() - 1
  return d


def split_mode(d):
  """how split_pixel turns a pixel index into (n, row, column)"""
  if d['sh_w'] >= 0:
    return 'shift'
  if not _pow2(d['ho']) and not _pow2(d['wo']):
    return 'div, neither 2^k'
  return 'div, %s not 2^k' % ('ho' if not _pow2(d['ho']) else 'wo')


def orient(d):
  return 'ho<wo' if d['ho'] < d['wo'] else ('ho>wo' if d['ho'] > d['wo'] else 'ho=wo')


# ---- the K slicing of the flat kernels ---------------------------------------------------------------------------------
def flat_plan(d, ni, forced_s, m=None):
  m = d['m'] if m is None else m
  tiles_m, tiles_n = _cdiv(m, 32), _cdiv(d['cout'], 32 * ni)
  tiles, target = tiles_m * tiles_n, 4096 // ni
  s = 1
  while s < 16 and tiles * s * 2 <= target + target // 2:
    s *= 2
  rr = 4 * d['cin']
  while s > 4 and _cdiv(rr, s // 4) < 8:
    s //= 2
  if forced_s > 0:
    s = min(forced_s, 16)
  s2 = 1 if s <= 4 else s // 4
  return dict(s=s, s2=s2, rs=_cdiv(_cdiv(rr, s2), 8) * 8, tiles_m=tiles_m, tiles_n=tiles_n)


def bwd_plan(d, ni, forced_s, m=None):
  m = d['m'] if m is None else m
  tiles_m, tiles_n = _cdiv(m, 32), _cdiv(d['cin'], 32 * ni)
  tiles, target = 4 * tiles_m * tiles_n, 4096
  s = 1
  while s < 16 and tiles * s * 2 <= target + target // 2:
    s *= 2
  while s > 4 and _cdiv(d['cout'], s // 4) < 8:
    s //= 2
  if forced_s > 0:
    s = forced_s
  s = min(s, 16)
  s2 = 1 if s <= 4 else s // 4
  return dict(s=s, s2=s2, rs=_cdiv(_cdiv(d['cout'], s2), 8) * 8, tiles_m=tiles_m, tiles_n=tiles_n)


def wrw_plan(d, forced_s=0, forced_p=0):
  """only as far as P (block copies: P > 1 = workspace + reduce launch) and S are needed"""
  tiles = _cdiv(d['cout'], 32) * _cdiv(d['kdim'], 128)
  total_pairs, batch = d['m'] // 2, 4
  waves = max(1, min(_cdiv(2048, tiles), _cdiv(total_pairs, 2 * batch)))
  s = 1
  while s < 4 and s * 2 <= waves:
    s *= 2
  if forced_s > 0:
    s = min(forced_s, 4)
  pb = min(_cdiv(waves, s), 256)
  if pb * tiles > 512:
    pb = max(512 // tiles, 1)
  if forced_p > 0:
    pb = forced_p
  ppw = _cdiv(_cdiv(total_pairs, pb * s), batch) * batch
  return dict(s=s, p=max(_cdiv(total_pairs, ppw * s), 1), tiles_k=_cdiv(d['kdim'], 128), tiles_co=_cdiv(d['cout'], 32))


# ---- both LDS formulas ------------------------------------------------------------------------------------------------
def rows_lds(d, rows):
  cin = d['cin']
  lpad, rpad, rowk = _cdiv(cin, 4) * 4, _cdiv(cin + 8, 4) * 4, _cdiv(4 * cin, 8) * 8
  return ((2 * rows + 2) * (lpad + d['w'] * cin + rpad) + 32 * (4 * rowk + 4)) * 4


def small_lds(d):
  return (6 * (d['wo'] + 2) * (d['cout'] + 4) + 16 * d['cout'] * (_cdiv(d['cin'], 4) * 4)) * 4


# ---- conv_fwd_impl ------------------------------------------------------------------------------------------------------
def fwd_plan(n, h, w, cin, cout, x_aligned=True, w_aligned=True, pair=False, pair_same_alignment=True, pair_w_aligned=True,
             tuning=(0, 0, 0)):
  """{'refused': text} | {'kernel': None} (empty batch) | the launch: kernel 'rows' | 'flat' | 'tiled' and its parameters"""
  d = conv_dims(n, h, w, cin, cout)
  if isinstance(d, str):
    return dict(refused=d)
  if n == 0:
    return dict(kernel=None, d=d)
  if not w_aligned:
    return dict(refused='conv4x4s2: weight must be 16-byte aligned')
  if pair and (not pair_w_aligned or not pair_same_alignment):
    return dict(refused='conv4x4s2 pair: the second problem needs the same operands, equally aligned')
  forced, forced_nt, forced_s = tuning
  pair_mul = 2 if pair else 1
  shape = forced
  if shape == 0 and cout > 32 and forced_nt == 0 and forced_s == 0:
    b64 = _cdiv(d['m'], 64) * _cdiv(cout, 64) * pair_mul
    shape = 2 if b64 >= 512 else (3 if b64 >= 256 else 0)
  if shape in (0, 6) and forced_nt == 0 and forced_s == 0 and d['wo'] == 32 and cout <= 32 and cin <= 20 and \
      d['ho'] % 4 == 0 and x_aligned:
    rows = 8 if d['ho'] % 8 == 0 else 4
    lds = rows_lds(d, rows)
    if lds <= LDS_LIMIT:
      return dict(kernel='rows', rows=rows, lds=lds, blocks_per_image=d['ho'] // rows, d=d)
  if shape == 6:
    shape = 0
  cin4 = cin % 4 == 0
  if shape < 1 or shape > 4:
    ni = forced_nt
    if ni == 0:
      t2, t1 = pair_mul * _cdiv(d['m'], 32) * _cdiv(cout, 64), pair_mul * _cdiv(d['m'], 32) * _cdiv(cout, 32)
      ni = 2 if t2 >= 256 else 1
      if ni == 2 and t2 % 256 != 0 and t2 < 1024 and t1 % 256 == 0:
        ni = 1
    if ni not in (1, 2) or cout <= 32:
      ni = 1
    pl = flat_plan(d, ni, forced_s)
    if pair and forced_s == 0:
      p2 = flat_plan(d, ni, 0, m=2 * d['m'])
      pl.update(s=p2['s'], s2=p2['s2'], rs=p2['rs'])
    return dict(kernel='flat', ni=ni, cin4=cin4, s=pl['s'], lds=pl['s'] * ni * 4096 if pl['s'] > 1 else 0,
                blocks=pl['tiles_m'] * pl['tiles_n'], split=split_mode(d), d=d)
  bm, bn = TILED[shape]
  return dict(kernel='tiled', shape=shape, cin4=cin4, blocks=_cdiv(d['m'], bm) * _cdiv(cout, bn), d=d)


# ---- conv_fwd_planes_impl ---------------------------------------------------------------------------------------------
def planes_plan(n, h, w, cin, cout):
  d = conv_dims(n, h, w, cin, cout)
  if isinstance(d, str):
    return dict(refused=d)
  if d['wo'] != 32 or cout > 32 or cin < 4 or cin > 20 or d['ho'] % 4 != 0:
    return dict(refused='conv4x4s2_fwd_planes: 64-wide inputs of 4 .. 20 planes, at most 32 output channels')
  if n == 0:
    return dict(kernel=None, d=d)
  rows = 8 if d['ho'] % 8 == 0 else 4
  lds = ((2 * rows + 2) * (4 + 3 * w + 8) + 32 * 68 + 512 + rows * 96 + 32) * 4
  return dict(kernel='planes', rows=rows, lds=lds, blocks_per_image=d['ho'] // rows, d=d)


# ---- conv_bwd_data_impl -----------------------------------------------------------------------------------------------
def bwd_data_plan(n, h, w, cin, cout, dy_aligned=True, pair=False, pair_same_alignment=True, tuning=(0, 0, 0)):
  d = conv_dims(n, h, w, cin, cout)
  if isinstance(d, str):
    return dict(refused=d)
  if n == 0:
    return dict(kernel=None, d=d)
  if cout % 4 != 0:
    return dict(refused='conv4x4s2_bwd_data: cout must be a multiple of 4')
  if pair and not pair_same_alignment:
    return dict(refused='conv4x4s2_bwd_data pair: the second problem needs the same operands, equally aligned')
  _, ni, forced_s = tuning
  lds = small_lds(d)
  if ni == 0 and forced_s == 0 and cin == 6 and dy_aligned and d['ho'] % 4 == 0 and lds <= LDS_LIMIT:
    return dict(kernel='small', lds=lds, blocks_per_image=d['ho'] // 4, launches=2 if pair else 1, d=d)
  if ni == 0:
    ni = 2 if cin >= 64 else 1
  if ni not in (1, 2) or cin <= 32:
    ni = 1
  pl = bwd_plan(d, ni, forced_s)
  if pair and forced_s == 0:
    p2 = bwd_plan(d, ni, 0, m=2 * d['m'])
    pl.update(s=p2['s'], s2=p2['s2'], rs=p2['rs'])
  return dict(kernel='flat', ni=ni, s=pl['s'], lds=pl['s'] * ni * 4096 if pl['s'] > 1 else 0,
              blocks=4 * pl['tiles_m'] * pl['tiles_n'], split=split_mode(d), small_lds=lds, d=d)


# ---- conv_wrw_impl ------------------------------------------------------------------------------------------------------
def wrw_launch(n, h, w, cin, cout, dw_aligned=True, dbias=False, dbias_aligned=True, bias_images=0, tuning=(0, 0)):
  d = conv_dims(n, h, w, cin, cout)
  if isinstance(d, str):
    return dict(refused=d)
  if not dw_aligned:
    return dict(refused='conv4x4s2_wrw: dw must be 16-byte aligned')
  if dbias and (not dbias_aligned or cout % 4 != 0):
    return dict(refused='conv4x4s2_wrw: dbias must be 16-byte aligned and cout a multiple of 4')
  if bias_images < 0 or bias_images > n:
    return dict(refused='conv4x4s2_wrw: 0 <= bias_images <= n')
  if n == 0:
    return dict(kernel='memset', d=d)
  if d['wo'] & 1:
    return dict(refused='conv4x4s2_wrw: w / 2 must be even (pixels are consumed in pairs)')
  pl = wrw_plan(d, *tuning)
  return dict(kernel='wrw', cin4=cin % 4 == 0, p=pl['p'], s=pl['s'], reduce=pl['p'] > 1, tiles_k=pl['tiles_k'], d=d)


def small_kernel_limits(h, cout, cin=6):
  """(the widest even w whose conv_bwd_small_kernel staging still fits the LDS, the next even w): derived from small_lds"""
  w = 2
  while small_lds(conv_dims(1, h, w + 2, cin, cout)) <= LDS_LIMIT:
    w += 2
  return w, w + 2


# ---- the case table ---------------------------------------------------------------------------------------------------
SMALL_FIT_W, SMALL_MISS_W = small_kernel_limits(8, 64)


def _c(family, dims, **kw):
  return dict(id='%s-%s' % (family, 'x'.join(str(v) for v in dims)) + ''.join('-%s' % v for v in kw.values()), family=family,
              dims=tuple(dims), **kw)


def _r4(c):
  return (c + 3) // 4 * 4


FWD_TABLE = [(3, 8, 12, 5, 7), (2, 12, 8, 5, 7), (2, 2, 6, 3, 1), (2, 6, 2, 3, 1), (2, 16, 8, 32, 64), (2, 8, 16, 32, 64),
             (3, 4, 12, 64, 128),
             (2, 8, 64, 14, 32), (1, 24, 64, 17, 32), (1, 16, 64, 6, 20),  # the row-staged kernel: rows 4, 4 (three blocks), 8
             (1, 4, 64, 14, 32), (1, 64, 8, 14, 32)]                       # ... and its near misses
SMALL_TABLE = [(2, 8, 16, 6, 8), (1, 24, 12, 6, 36), (1, 8, 64, 6, 32), (1, 64, 8, 6, 32),
               (1, 8, SMALL_FIT_W, 6, 64), (1, 8, SMALL_MISS_W, 6, 64)]
# the forward table with cout rounded up to a multiple of 4 -- less the cases that reach no cell of their own in the data
# gradient (test_no_case_is_redundant): its kernels know no row-staged path, so the 64-wide cases of 14 and 17 planes and
# (1, 64, 8, 14, 32) repeat what (3, 8, 12, 5, 8) and the small table's cases under their forced flat plans reach, and
# (1, 16, 64, 6, 20) repeats the small kernel's (1, 8, 64, 6, 32)
BWD_DROPPED = [(1, 4, 64, 14, 32), (1, 24, 64, 17, 32), (1, 16, 64, 6, 20), (2, 8, 64, 14, 32), (1, 64, 8, 14, 32)]
BWD_TABLE = [(n, h, w, cin, _r4(cout)) for n, h, w, cin, cout in FWD_TABLE if (n, h, w, cin, cout) not in BWD_DROPPED] + SMALL_TABLE
WRW_TABLE = [(3, 8, 12, 5, 8), (2, 12, 8, 5, 8), (2, 2, 4, 3, 4), (2, 6, 4, 3, 4), (2, 16, 8, 32, 64), (2, 8, 16, 32, 64),
             (1, 24, 64, 17, 32)]
WRW_GROUP = [(3, 8, 12, 5, 8), (2, 16, 8, 32, 64), (1, 24, 64, 17, 32)]  # one grouped call: three geometries
MISALIGNED = [(2, 8, 12, 32, 16), (1, 8, 64, 14, 32), (2, 8, 16, 6, 8)]   # CIN4; rows kernel when aligned; small kernel when aligned
OFFSETS = (1, 2, 3)  # floats into the allocation

CASES = ([_c('fwd', t) for t in FWD_TABLE] + [_c('bwd', t) for t in BWD_TABLE] + [_c('wrw', t) for t in WRW_TABLE] +
         [_c('planes', (2, 24, 64, 14, 32)),
          _c('pair_fwd', (2, 8, 12, 5, 7)), _c('pair_bwd', (2, 12, 8, 5, 8)), _c('pair_planes', (1, 8, 64, 17, 32)),
          _c('layer', (3, 8, 24, 14, 32))] + [_c('misaligned', t) for t in MISALIGNED])
CASE_IDS = [c['id'] for c in CASES]
BY_ID = dict(zip(CASE_IDS, CASES))


def cases_of(family):
  return [c for c in CASES if c['family'] == family]


def ids_of(family):
  return [c['id'] for c in cases_of(family)]


def non_square(case):
  return case['dims'][1] != case['dims'][2]


def _wo_class(wo):
  return '32' if wo == 32 else ('>32' if wo > 32 else ('pow2' if _pow2(wo) else 'npow2'))


def _tiles(d):
  return ('one pixel tile' if d['m'] <= 32 else 'pixel tiles>1') + (', n>1' if d['n'] > 1 else ', n=1')


def _fwd_cells(dims, prefix='fwd', **kw):
  """the cells one forward launch reaches"""
  p = fwd_plan(*dims, **kw)
  d = p['d']
  cells = set()
  if p['kernel'] == 'rows':
    cells.add((prefix, 'rows', p['rows'], 'blocks/image>1' if p['blocks_per_image'] > 1 else 'blocks/image=1'))
  elif p['kernel'] == 'flat':
    cells.add((prefix, 'flat', 'split_pixel', p['split'], orient(d), 'cin4' if p['cin4'] else 'cut', _tiles(d)))
    cells.add((prefix, 'flat', 'NI=%d' % p['ni'], orient(d)))
  else:
    cells.add((prefix, 'tiled', p['shape'], orient(d)))
  return cells


def _bwd_cells(dims, prefix='bwd', **kw):
  p = bwd_data_plan(*dims, **kw)
  d = p['d']
  cells = set()
  if p['kernel'] == 'small':
    cells.add((prefix, 'small', 'wo ' + _wo_class(d['wo']), orient(d)))
    if d['cout'] == 36:
      cells.add((prefix, 'small', 'cout=36'))
    if (d['wo'], d['cout']) != (32, 32):
      cells.add((prefix, 'small', 'geometry', d['wo'], d['cout']))
    if small_lds(conv_dims(d['n'], d['h'], d['w'] + 2, d['cin'], d['cout'])) > LDS_LIMIT:
      cells.add((prefix, 'small', 'the widest w that fits the LDS'))
  else:
    cells.add((prefix, 'flat', 'split_pixel', p['split'], orient(d),
               'cin<32' if d['cin'] < 32 else ('cin=32' if d['cin'] == 32 else 'cin>32'), _tiles(d)))  # (a ragged / full / second channel tile)
    cells.add((prefix, 'flat', 'NI=%d' % p['ni'], orient(d)))
    if d['ho'] == 1 or d['wo'] == 1:
      cells.add((prefix, 'one dy ' + ('row' if d['ho'] == 1 else 'column')))
    if kw.get('tuning', (0, 0, 0)) == (0, 0, 0) and d['cin'] == 6 and kw.get('dy_aligned', True) and d['ho'] % 4 == 0:
      cells.add((prefix, 'small near miss', 'LDS'))
  return cells


def case_cells(case):
  """every cell the GPU test of this case reaches"""
  fam, dims = case['family'], case['dims']
  n, h, w, cin, cout = dims
  cells = set()
  if fam == 'fwd':
    for t in FWD_VARIANTS:
      cells |= _fwd_cells(dims, tuning=t)
    d = conv_dims(*dims)
    if d['ho'] == 1 or d['wo'] == 1:
      cells.add(('fwd', 'one output ' + ('row' if d['ho'] == 1 else 'column')))
    # near misses of the row-staged kernel: everything but ONE condition of its selection holds
    if fwd_plan(*dims)['kernel'] != 'rows' and d['wo'] == 32 and cout <= 32 and cin <= 20 and d['ho'] % 4 != 0:
      cells.add(('fwd', 'rows near miss', 'ho % 4 != 0'))
    if fwd_plan(*dims)['kernel'] != 'rows' and fwd_plan(n, w, h, cin, cout)['kernel'] == 'rows':
      cells.add(('fwd', 'rows near miss', 'transposed'))
  elif fam == 'bwd':
    for t in BWD_VARIANTS:
      cells |= _bwd_cells(dims, tuning=t)
  elif fam == 'wrw':
    p = wrw_launch(*dims)
    d = p['d']
    cells.add(('wrw', 'P>1' if p['reduce'] else 'P=1', 'cin4' if p['cin4'] else 'cut', orient(d),
               'tiles_k>1' if p['tiles_k'] > 1 else 'tiles_k=1'))
    if non_square(case):
      cells.add(('wrw', 'P>1' if p['reduce'] else 'P=1', 'non-square'))
  elif fam == 'planes':
    p = planes_plan(*dims)
    cells.add(('planes', 'rows=%d' % p['rows']))
  elif fam == 'pair_fwd':
    cells.add(('pair', 'fwd', fwd_plan(*dims, pair=True)['kernel'], orient(conv_dims(*dims))))
  elif fam == 'pair_bwd':
    cells.add(('pair', 'bwd', bwd_data_plan(*dims, pair=True)['kernel'], orient(conv_dims(*dims))))
  elif fam == 'pair_planes':
    cells.add(('pair', 'planes', 'rows=%d' % planes_plan(*dims)['rows']))
  elif fam == 'layer':
    cells.add(('layer', 'autograd', orient(conv_dims(*dims))))
  elif fam == 'misaligned':
    aligned_f, aligned_b = fwd_plan(*dims), bwd_data_plan(*dims)
    f, b = fwd_plan(*dims, x_aligned=False), bwd_data_plan(*dims, dy_aligned=False)
    cells.add(('misaligned x', f['kernel'], 'cin4' if f['cin4'] else 'cut'))
    if aligned_f['kernel'] == 'rows':
      cells.add(('misaligned x', 'excludes the rows kernel'))
    cells.add(('misaligned dy', b['kernel'], 'cin %s 32' % ('<=' if cin <= 32 else '>')))
    if aligned_b['kernel'] == 'small':
      cells.add(('misaligned dy', 'excludes the small kernel'))
  return cells


# what the table must reach; every case owns at least one of these cells
REQUIRED_CELLS = (
    # split_pixel by division and by shifts (ho != wo: log2 ho != log2 wo), rows shorter and longer than columns
    # (cut / cin4: chunks cut by the image edge or whole; cin < / = / > 32: a ragged, a full, a second channel tile)
    [('fwd', 'flat', 'split_pixel') + t for t in (
        ('div, ho not 2^k', 'ho<wo', 'cut', 'pixel tiles>1, n=1'),
        ('div, ho not 2^k', 'ho>wo', 'cut', 'one pixel tile, n>1'),
        ('div, ho not 2^k', 'ho>wo', 'cut', 'pixel tiles>1, n>1'),
        ('div, wo not 2^k', 'ho<wo', 'cin4', 'pixel tiles>1, n>1'),
        ('div, wo not 2^k', 'ho<wo', 'cut', 'one pixel tile, n>1'),
        ('div, wo not 2^k', 'ho<wo', 'cut', 'pixel tiles>1, n>1'),
        ('shift', 'ho<wo', 'cin4', 'pixel tiles>1, n>1'),
        ('shift', 'ho<wo', 'cut', 'pixel tiles>1, n=1'),
        ('shift', 'ho<wo', 'cut', 'pixel tiles>1, n>1'),
        ('shift', 'ho>wo', 'cin4', 'pixel tiles>1, n>1'),
        ('shift', 'ho>wo', 'cut', 'pixel tiles>1, n=1'))] +
    [('bwd', 'flat', 'split_pixel') + t for t in (
        ('div, ho not 2^k', 'ho>wo', 'cin<32', 'one pixel tile, n>1'),
        ('div, ho not 2^k', 'ho>wo', 'cin<32', 'pixel tiles>1, n>1'),
        ('div, neither 2^k', 'ho>wo', 'cin<32', 'pixel tiles>1, n=1'),
        ('div, wo not 2^k', 'ho<wo', 'cin<32', 'one pixel tile, n>1'),
        ('div, wo not 2^k', 'ho<wo', 'cin<32', 'pixel tiles>1, n=1'),
        ('div, wo not 2^k', 'ho<wo', 'cin<32', 'pixel tiles>1, n>1'),
        ('div, wo not 2^k', 'ho<wo', 'cin>32', 'pixel tiles>1, n>1'),
        ('shift', 'ho<wo', 'cin<32', 'pixel tiles>1, n=1'),
        ('shift', 'ho<wo', 'cin<32', 'pixel tiles>1, n>1'),
        ('shift', 'ho<wo', 'cin=32', 'pixel tiles>1, n>1'),
        ('shift', 'ho>wo', 'cin<32', 'pixel tiles>1, n=1'),
        ('shift', 'ho>wo', 'cin=32', 'pixel tiles>1, n>1'))] +
    [('bwd', 'one dy row'), ('bwd', 'one dy column'),
     ('fwd', 'one output row'), ('fwd', 'one output column'),
     ('fwd', 'rows', 4, 'blocks/image=1'), ('fwd', 'rows', 4, 'blocks/image>1'), ('fwd', 'rows', 8, 'blocks/image=1'),
     ('fwd', 'rows near miss', 'ho % 4 != 0'), ('fwd', 'rows near miss', 'transposed'),
     ('planes', 'rows=4'),
     ('bwd', 'small', 'wo pow2', 'ho<wo'), ('bwd', 'small', 'wo pow2', 'ho>wo'), ('bwd', 'small', 'wo npow2', 'ho>wo'),
     ('bwd', 'small', 'wo 32', 'ho<wo'), ('bwd', 'small', 'wo >32', 'ho<wo'), ('bwd', 'small', 'cout=36'),
     ('bwd', 'small', 'the widest w that fits the LDS'), ('bwd', 'small near miss', 'LDS'),
     ('misaligned x', 'excludes the rows kernel'), ('misaligned x', 'flat', 'cin4'), ('misaligned x', 'flat', 'cut'),
     ('misaligned dy', 'excludes the small kernel'), ('misaligned dy', 'flat', 'cin <= 32'),
     ('fwd', 'flat', 'NI=2', 'ho<wo'), ('fwd', 'flat', 'NI=2', 'ho>wo'), ('bwd', 'flat', 'NI=2', 'ho<wo')] +
    [('fwd', 'tiled', s, o) for s in (1, 2, 3, 4) for o in ('ho<wo', 'ho>wo')] +
    [('wrw', 'P=1', 'non-square'), ('wrw', 'P>1', 'non-square'),
     ('wrw', 'P>1', 'cut', 'ho<wo', 'tiles_k=1'), ('wrw', 'P>1', 'cut', 'ho>wo', 'tiles_k=1'),
     ('wrw', 'P=1', 'cut', 'ho<wo', 'tiles_k=1'), ('wrw', 'P=1', 'cut', 'ho>wo', 'tiles_k=1'),
     ('wrw', 'P=1', 'cin4', 'ho<wo', 'tiles_k>1'), ('wrw', 'P=1', 'cin4', 'ho>wo', 'tiles_k>1'),
     ('wrw', 'P>1', 'cut', 'ho<wo', 'tiles_k>1'),
     ('pair', 'fwd', 'flat', 'ho<wo'), ('pair', 'bwd', 'flat', 'ho>wo'), ('pair', 'planes', 'rows=4'),
     ('layer', 'autograd', 'ho<wo')])


def cells_run(cases=None):
  out = set()
  for c in (CASES if cases is None else cases):
    out |= case_cells(c)
  return out


# ---- the refusals the GPU test provokes (and the host test checks against the C entry points) ---------------------------
# (entry, geometry, what is wrong) -> the restated plan must refuse it
REFUSALS = [
    ('fwd', (2, 8, 12, 5, 7), dict(w_aligned=False)),
    ('fwd_pair', (2, 8, 12, 5, 7), dict(pair=True, pair_w_aligned=False)),
    ('fwd_pair', (2, 8, 12, 5, 7), dict(pair=True, pair_same_alignment=False)),
    ('bwd_pair', (2, 8, 12, 5, 8), dict(pair=True, pair_same_alignment=False)),
    ('wrw', (2, 8, 12, 5, 8), dict(dw_aligned=False)),
    ('wrw_bias', (2, 8, 12, 5, 8), dict(dbias=True, dbias_aligned=False)),
    ('wrw_bias', (2, 8, 12, 5, 6), dict(dbias=True)),   # cout % 4 != 0 for dbias
    ('bwd', (2, 8, 12, 5, 6), dict()),                   # cout % 4 != 0 for the data gradient
    ('wrw', (2, 8, 6, 5, 8), dict()),                    # w / 2 odd
    ('fwd', (2, 7, 12, 5, 8), dict()), ('fwd', (2, 8, 11, 5, 8), dict()),
    ('bwd', (2, 7, 12, 5, 8), dict()), ('bwd', (2, 8, 11, 5, 8), dict()),
    ('wrw', (2, 7, 12, 5, 8), dict()), ('wrw', (2, 8, 11, 5, 8), dict()),
]


def refusal_plan(entry, dims, kw):
  if entry in ('fwd', 'fwd_pair'):
    return fwd_plan(*dims, **kw)
  if entry in ('bwd', 'bwd_pair'):
    return bwd_data_plan(*dims, **kw)
  return wrw_launch(*dims, **kw)


# ---- float64 references and the assertions the GPU tests make ---------------------------------------------------------
def make_operands(dims, seed, device='cpu'):
  """(x, w, bias, dy) of a case: float32, NHWC, the weight in channels_last memory order"""
  n, h, w_, cin, cout = dims
  g = torch.Generator(device='cpu').manual_seed(seed)
  x = torch.randn((n, h, w_, cin), generator=g)
  w = (torch.randn((cout, cin, 4, 4), generator=g) / (16 * cin)**0.5).contiguous(memory_format=torch.channels_last)
  b = torch.randn((cout,), generator=g) * 0.1
  dy = torch.randn((n, h // 2, w_ // 2, cout), generator=g)
  return tuple(t.to(device) for t in (x, w, b, dy))


def slope(z, leak=0.2):
  return torch.where(z > 0, torch.ones_like(z), torch.where(z < 0, torch.full_like(z, leak), torch.full_like(z, 0.5 * (1 + leak))))


def reference(x, w, dy):
  """float64 on the CPU: (y, dx, dw) of conv2d(stride 2, padding 1) without bias, NHWC in and out; dw shaped like w"""
  xd = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
  wd = w.double().cpu().requires_grad_(True)
  y = F.conv2d(xd, wd, None, 2, 1)
  dx, dw = torch.autograd.grad(y, [xd, wd], dy.double().cpu().permute(0, 3, 1, 2))
  return y.detach().permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous(), dw


def swapped_reference(x, w, dy):
  """what a kernel that read h as w would compute: the SAME memory taken as (n, w, h, cin) / (n, wo, ho, cout), the
  results' memory read back in the true shapes (no operand is transposed: that would transpose the result and show nothing)"""
  n, h, w_, cin = x.shape
  y, dx, dw = reference(x.cpu().reshape(n, w_, h, cin), w, dy.cpu().reshape(n, w_ // 2, h // 2, dy.shape[-1]))
  return y.reshape(n, h // 2, w_ // 2, -1), dx.reshape(n, h, w_, cin), dw


def rel_err(got, ref):
  """max |got - ref| / max |ref|, NaN where an element was not written"""
  return float((got.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def assert_close(got, ref, bound, what, atol=0.0, scale=None):
  """the assertion of every value comparison in tests/test_hip_conv_geometry.py: max |got - ref| < bound x `scale` (default:
  max |ref|); returns the error as a fraction of the scale for the report"""
  assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
  scale = float(ref.abs().max()) if scale is None else scale
  err = float((got.detach().double().cpu() - ref).abs().max())
  assert err < bound * scale + atol, (what, err / scale, bound)  # (a NaN -- an element nobody wrote -- fails too)
  return err / scale


def assert_bias_close(got, dy, k, what):
  want = dy[:k].double().sum(dim=(0, 1, 2)).cpu()
  tol = BOUND_BIAS * float(dy[:k].double().abs().sum(dim=(0, 1, 2)).max()) + 1e-30
  err = float((got.double().cpu() - want).abs().max())
  assert err <= tol, (what, k, err, tol)
  return err


BOUND_LAYER = 2e-5  # nn_ops.conv_bias_lrelu: test_fused_conv_layer_autograd_matches_the_library_pair's (+ 1e-7 absolute)
# the outputs a family's GPU test compares with float64, each with the LOOSEST bound any of its assertions uses
FAMILY_OUTPUTS = {'fwd': (('y', BOUND_BWD),), 'bwd': (('dx', BOUND_BWD),), 'wrw': (('dw', BOUND_WRW),),
                  'planes': (('y', BOUND_PLANES),), 'pair_fwd': (('y', BOUND_FWD),), 'pair_bwd': (('dx', BOUND_BWD),),
                  'pair_planes': (('y', BOUND_PLANES),), 'layer': (('y', BOUND_LAYER), ('dx', BOUND_LAYER), ('dw', BOUND_LAYER)),
                  'misaligned': (('y', BOUND_BWD), ('dx', BOUND_BWD))}


def case_operands(case, device='cpu'):
  """(x, w, bias, dy) of a case; the planes families get an input whose channels 3 .. are per-image constants"""
  x, w, b, dy = make_operands(case['dims'], seed=100 + CASE_IDS.index(case['id']))
  if case['family'] in ('planes', 'pair_planes'):
    x[..., 3:] = x[:, :1, :1, 3:]
  return tuple(t.to(device) for t in (x, w, b, dy))
