"""Helper of tests/test_hip_policy_matrix.py (not a test module; pure Python, no torch): every kernel instantiation the
host side of the inference passes can select, the selection rule restated from its description, and the table of cases
whose launches -- under the default EXPO_STREAM_MIN_BYTES and under EXPO_STREAM_MIN_BYTES=1 together -- select every
one of them that a caller can reach.

The rule, restated (chain_fused.hip's "ragged" comment, DESIGN.md §3.15 / §3.16 / §3.31, host_common.h::make_geom,
decode.hip::decode_ragged_t / decode_tables_t / codes_max_t, codes_lut.hip::codes_lut_t):

  * ragged passes: ragged_plan below (tests/test_ragged_launch_host.py compares it with the host code itself);
  * dense kernels (make_geom): the vector path when hw is a whole number of 12-byte vectors and x, y and -- for storage
    taps and u16 taps of fp16 -- the tap buffer are 4-byte aligned; IoStream only on the vector path, when the tensor
    holds at least EXPO_STREAM_MIN_BYTES;
  * decode_ragged: IoStream when the call's code bytes plus output bytes reach the threshold; an image is on the vector
    path when its codes and its output are 4-byte aligned and hw % PPV == 0; decode_max_kernel (normalize only; also
    from decode_tables and codes_max_ragged, which count code bytes alone) when its codes are 4-byte aligned;
  * codes_lut_ragged: code bytes plus output bytes; the vector path needs aligned codes and output and hw % PPV == 0
    with PPV = 12 / (3 sizeof(OT)); 16-bit codes with uint8 entries take the LDS-staged kernel unless
    EXPO_CODES_LUT_LDS16=0 (the tables of the cases are 16-byte aligned).
"""
import itertools

TAP_STORAGE, TAP_U8, TAP_U16, TAP_NONE = 0, 1, 3, -1
FMT_NAME = {TAP_NONE: 'none', TAP_STORAGE: 'storage', TAP_U8: 'u8', TAP_U16: 'u16'}
FMT3 = (TAP_STORAGE, TAP_U8, TAP_U16)
FMT4 = (TAP_NONE,) + FMT3
DTYPES = ('f16', 'f32')
IOS = ('cached', 'stream')
CODE_TYPES = ('u8', 'u16')
CHANNELS = (1, 3, 4)
SIZEOF = {'f16': 2, 'f32': 4, 'u8': 1, 'u16': 2}
DEFAULT_STREAM_MIN_BYTES = 8 << 20
THRESHOLDS = (DEFAULT_STREAM_MIN_BYTES, 1)  # the parent process; the EXPO_STREAM_MIN_BYTES=1 child

STEPS = 5
TAP_MASK = 0b10101
CURVE_STEPS = 5
SHARP, MIN_STRENGTH = 1.0, 0.3


def tap_vector_stored(dtype, fmt):
  return fmt == TAP_STORAGE or (fmt == TAP_U16 and dtype == 'f16')


# ---------------------------------------------------------------------------------------------------------------------
# the instantiations: a literal product of the template parameters
# ---------------------------------------------------------------------------------------------------------------------
DENSE_PATHS = (('vector', 'stream'), ('vector', 'cached'), ('element', 'cached'))  # (VEC, IO) of the dense ladders


def enumerate_instantiations():
  """{unit: [instantiation, ...]}; an instantiation is (kernel, template arguments...)."""
  slow = (False, True)
  chain_fused = (
      [('chain_fused_fwd_kernel', t, vec, io) for t in DTYPES for vec, io in DENSE_PATHS] +
      [('chain_fused_fwd_taps_kernel', t, vec, io, f) for t in DTYPES for vec, io in DENSE_PATHS for f in FMT3] +
      [('chain_fused_fwd_ragged_kernel', t, io, s) for t in DTYPES for io in IOS for s in slow] +
      [('chain_fused_fwd_ragged_taps_kernel', t, io, s, f) for t in DTYPES for io in IOS for s in slow for f in FMT3] +
      [('chain_fused_masked_ragged_kernel', t, io, s, f) for t in DTYPES for io in IOS for s in slow for f in FMT4])
  curves = [('chain_fused_curves_ragged_kernel', t, io, s, f) for t in DTYPES for io in IOS for s in slow for f in FMT4]
  codes = [('chain_fused_fwd_ragged_codes_kernel', ct, c, t, io, f)
           for ct in CODE_TYPES for c in CHANNELS for t in DTYPES for io in IOS for f in FMT4]
  curves_codes = [('chain_fused_fwd_ragged_codes_kernel[curves]',) + inst[1:] for inst in codes]
  decode = (
      [('decode_kernel', ct, c, t, norm, io)
       for ct in CODE_TYPES for c in CHANNELS for t in DTYPES for norm in (False, True) for io in IOS] +
      [('decode_max_kernel', ct, c, io) for ct in CODE_TYPES for c in CHANNELS for io in IOS])
  lut = ([('codes_lut_kernel', ct, c, ot, io, False)
          for ct in CODE_TYPES for c in CHANNELS for ot in CODE_TYPES for io in IOS] +
         [('codes_lut_kernel', 'u16', c, 'u8', io, True) for c in CHANNELS for io in IOS])
  return {'chain_fused.hip': chain_fused, 'chain_fused_curves.hip': curves, 'chain_fused_codes.hip': codes,
          'chain_fused_curves_codes.hip': curves_codes, 'decode.hip': decode, 'codes_lut.hip': lut}


BOTH_PATHS = ('chain_fused_fwd_ragged_codes_kernel', 'chain_fused_fwd_ragged_codes_kernel[curves]', 'decode_kernel',
              'decode_max_kernel', 'codes_lut_kernel')  # kernels that hold the vector and the element-wise path
PATHS = ('vector', 'element')
MAX_ENTRIES = ('decode_ragged', 'decode_tables', 'codes_max_ragged')  # who launches decode_max_kernel


def cells_of_instantiation(inst):
  """The cells of one instantiation: itself; with each path for a kernel that holds both; decode_max_kernel also with
  each of its three callers."""
  if inst[0] == 'decode_max_kernel':
    return [(inst, p, e) for p in PATHS for e in MAX_ENTRIES]
  if inst[0] in BOTH_PATHS:
    return [(inst, p) for p in PATHS]
  return [inst]


def all_cells():
  insts = [inst for unit in enumerate_instantiations().values() for inst in unit]
  return {cell for inst in insts for cell in cells_of_instantiation(inst)}


FLOAT_POINTER_KERNELS = ('chain_fused_fwd_kernel', 'chain_fused_fwd_taps_kernel', 'chain_fused_fwd_ragged_kernel',
                         'chain_fused_fwd_ragged_taps_kernel', 'chain_fused_masked_ragged_kernel',
                         'chain_fused_curves_ragged_kernel')


def unreachable(cell):
  """float32 storage on the element-wise path, in a kernel whose path depends only on float32 pointers: hw is always a
  whole number of 12-byte vectors there (one pixel), so the element-wise path needs a float32 base that is not 4-byte
  aligned -- and no tensor has one (torch refuses a float32 view at a byte offset that is no multiple of 4)."""
  if cell[0] not in FLOAT_POINTER_KERNELS or cell[1] != 'f32':
    return False
  if cell[0] in ('chain_fused_fwd_kernel', 'chain_fused_fwd_taps_kernel'):
    return cell[2] == 'element'
  return cell[3] is True  # ANY_SLOW


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def ragged_plan(dtype, fmt, images, ys=True, stream_min_bytes=DEFAULT_STREAM_MIN_BYTES):
  """The launches of one ragged call.  images: (h, w, x, y, taps) with byte addresses (x: the input, or the codes of a
  codes pass).  -> [{'stream', 'any_slow', 'first', 'base', 'n', 'vec', 'slots': [(j, x, y, h, w, taps)]}]"""
  ppl, ppv, size = (8, 2, 2) if dtype == 'f16' else (4, 1, 4)
  stream = sum(h * w * 3 * size for h, w, _, _, _ in images) >= stream_min_bytes
  out = []
  for base in range(0, len(images), 64):
    part = images[base:base + 64]
    first, vec, slots = [0], 0, []
    for j, (h, w, x, y, taps) in enumerate(part):
      hw = h * w
      y = y if ys else 0
      taps = 0 if fmt == TAP_NONE else taps  # no tap kernel reads a tap pointer
      groups = -(-hw // ppl)
      first.append(first[-1] + -(-groups // 256))
      aligned = x % 4 == 0 and y % 4 == 0 and (not tap_vector_stored(dtype, fmt) or taps % 4 == 0)
      if hw % ppv == 0 and aligned:
        vec |= 1 << j
      slots.append((j, x, y, h, w, taps))
    out.append({'stream': stream, 'any_slow': vec != (1 << len(part)) - 1, 'first': first, 'base': base,
                'n': len(part), 'vec': vec, 'slots': slots})
  return out


# ---------------------------------------------------------------------------------------------------------------------
# the images (a block covers 2048 pixels in fp16 -- 256 lanes x 8 -- and 1024 in fp32)
# ---------------------------------------------------------------------------------------------------------------------
SIZE = {
    'V': (41, 50),   # 2050 pixels: even, two blocks in fp16 and three in fp32, the last group partial
    'S': (37, 53),   # 1961 pixels: odd (element-wise in fp16), a partial last group
    'P': (1, 2),     # the vector path, a single group
    'Q': (4, 6),     # the vector path, a single group; its sequence ends on -1
    'O': (1, 1),     # one pixel: element-wise in fp16
    'W': (65, 64),   # the look-up only: 4160 pixels, a multiple of its PPV = 4 (uint8 entries; V's 2050 is not), two
                     # blocks of 4096 pixels there and three of 2048 with uint16 entries
}
# an image of a launch is (size name, which base starts one element into its buffer: '' none, 'x' the input, 'y' the
# output, 't' the tap planes, 'c' the codes -- one byte for uint8 codes, one element for uint16 ones)
IMAGE_KEYS = ('V', 'S', 'P', 'Q', 'O', 'Vx', 'Vy', 'Vt', 'Vc', 'W', 'V2', 'S2')  # V2, S2: a dense case's second image
# Tone = 4 and Color = 7 in every sequence (the per-wave curve table); Q ends on -1: its output is exactly +0
SEQUENCES = {'V': (0, 4, 7, 5, 1), 'S': (1, 4, 7, 4, 5), 'P': (2, 7, 4, 3, 6), 'Q': (1, 7, 4, 0, -1),
             'O': (7, 2, 4, 6, 3), 'Vx': (5, 4, 3, 7, 0), 'Vy': (7, 2, 4, 8, 1), 'Vt': (3, 7, 6, 4, 2),
             'Vc': (5, 4, 3, 7, 0), 'W': (6, 7, 1, 4, 8), 'V2': (4, 5, 7, 2, 3), 'S2': (7, 0, 4, 6, 1)}
MINUS_ONE = ('Q',)


def size_of(key):
  return SIZE[key[0]]


def ragged_images(dtype, fmt, launch):
  """The images of a float ragged launch.  'vector': every image on the vector path; 'mixed' (fp16): V, the odd S, V
  with x / y / the tap planes (where the taps are vector-stored) one element in, one pixel, and a vector image last."""
  if launch == 'vector':
    return ['V', 'P', 'Q']
  assert dtype == 'f16'
  return ['V', 'S', 'Vx', 'Vy'] + (['Vt'] if tap_vector_stored(dtype, fmt) else []) + ['O', 'Q']


CODES_IMAGES = ['V', 'S', 'Vc', 'O', 'Q']        # fp16: V, Q vector; fp32: S and O too; Vc element-wise in both
LUT_IMAGES = ['V', 'W', 'S', 'Vc', 'O', 'Q']


def addresses(keys, elem, code_elem=None):
  """(h, w, x, y, taps) byte addresses of a launch's images in a model address space: every buffer 4-byte aligned, a
  misaligned base one element in (elem: bytes of a storage element; code_elem: of a code)"""
  out = []
  for i, key in enumerate(keys):
    h, w = size_of(key)
    base = 0x100000 * (i + 1)
    x = base + (elem if key[1:] == 'x' else code_elem if key[1:] == 'c' else 0)
    y = base + 0x40000 + (elem if key[1:] == 'y' else 0)
    taps = base + 0x80000 + (elem if key[1:] == 't' else 0)
    out.append((h, w, x, y, taps))
  return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
RAGGED_KERNEL = {'ragged': 'chain_fused_fwd_ragged_kernel', 'ragged_taps': 'chain_fused_fwd_ragged_taps_kernel',
                 'masked': 'chain_fused_masked_ragged_kernel', 'curves': 'chain_fused_curves_ragged_kernel'}
RAGGED_FORMATS = {'ragged': (TAP_NONE,), 'ragged_taps': FMT3, 'masked': FMT4, 'curves': FMT4}
CODES_KERNEL = {'codes': 'chain_fused_fwd_ragged_codes_kernel',
                'curves_codes': 'chain_fused_fwd_ragged_codes_kernel[curves]'}
DECODE_KIND = {('u8', True): 'srgb8', ('u8', False): 'srgb8', ('u16', True): 'srgb16', ('u16', False): 'prophoto16'}


def codes_kind(ct, c):
  """the decode kind behind a codes pass's tables: a normalised table per image, or (16-bit, three channels) the one
  shared ProPhoto table"""
  return 'srgb8' if ct == 'u8' else 'prophoto16' if c == 3 else 'srgb16'


def _case(**kw):
  parts = [kw['family']] + [FMT_NAME[v] if k == 'fmt' else ('%s%s' % (k, v) if isinstance(v, (bool, int)) else str(v))
                            for k, v in kw.items() if k != 'family']
  kw['id'] = '-'.join(parts)
  return kw


def make_cases():
  cases = []
  # dense: two images of one size; V on the vector path, S (fp16) element-wise
  for family, fmts in (('dense', (TAP_NONE,)), ('dense_taps', FMT3)):
    for fmt in fmts:
      for dtype, shape in (('f16', 'V'), ('f16', 'S'), ('f32', 'V')):
        cases.append(_case(family=family, dtype=dtype, fmt=fmt, shape=shape))
  # the four float ragged passes: an all-vector launch in both dtypes, a mixed one in fp16
  for family, fmts in RAGGED_FORMATS.items():
    for fmt in fmts:
      for dtype, launch in (('f16', 'vector'), ('f16', 'mixed'), ('f32', 'vector')):
        cases.append(_case(family=family, dtype=dtype, fmt=fmt, launch=launch))
  # the passes from codes: one mixed call per kernel
  for family in CODES_KERNEL:
    for ct, c, dtype, fmt in itertools.product(CODE_TYPES, CHANNELS, DTYPES, FMT4):
      cases.append(_case(family=family, ct=ct, c=c, dtype=dtype, fmt=fmt))
  for ct, c, dtype, norm in itertools.product(CODE_TYPES, CHANNELS, DTYPES, (False, True)):
    cases.append(_case(family='decode', ct=ct, c=c, dtype=dtype, norm=norm))
  for family in ('decode_tables', 'codes_max'):
    for ct, c in itertools.product(CODE_TYPES, CHANNELS):
      cases.append(_case(family=family, ct=ct, c=c))
  for ct, c, ot in itertools.product(CODE_TYPES, CHANNELS, CODE_TYPES):
    for lds16 in ((False, True) if (ct, ot) == ('u16', 'u8') else (False,)):
      cases.append(_case(family='lut', ct=ct, c=c, ot=ot, lds16=lds16))
  return cases


CASES = make_cases()
CASE_IDS = [c['id'] for c in CASES]
BY_ID = dict(zip(CASE_IDS, CASES))
assert len(BY_ID) == len(CASES)


def case_images(case):
  """the image keys of a case's call, in order"""
  f = case['family']
  if f in ('dense', 'dense_taps'):
    return [case['shape'], case['shape'] + '2']
  if f in RAGGED_KERNEL:
    return ragged_images(case['dtype'], case['fmt'], case['launch'])
  return LUT_IMAGES if f == 'lut' else CODES_IMAGES


def without_ys(case):
  """once per pass and tap format the call is repeated with ys = NULL (taps only): the mixed launch, or the fp16 call"""
  f = case['family']
  if case.get('fmt', TAP_NONE) == TAP_NONE:
    return False
  if f == 'dense_taps':
    return case['dtype'] == 'f16' and case['shape'] == 'S'
  if f in RAGGED_KERNEL:
    return case['launch'] == 'mixed'
  return f in CODES_KERNEL and case['dtype'] == 'f16' and (case['ct'], case['c']) == ('u8', 3)


def _paths_cells(inst, vec_bits):
  return {(inst, 'vector' if v else 'element') for v in vec_bits}


def case_cells(case, stream_min_bytes, ys=True):
  """The cells one case's call selects under a threshold (ys=False: its repetition without outputs)."""
  f = case['family']
  io = lambda nbytes: 'stream' if nbytes >= stream_min_bytes else 'cached'  # noqa: E731
  keys = case_images(case)
  if f in ('dense', 'dense_taps'):
    t, fmt = case['dtype'], case['fmt']
    (h, w, x, y, taps), = addresses(keys[:1], SIZEOF[t])
    ppv = 2 if t == 'f16' else 1
    ptrs = [x, y if ys else 0] + ([taps] if tap_vector_stored(t, fmt) and fmt != TAP_NONE else [])
    vec = (h * w) % ppv == 0 and all(p % 4 == 0 for p in ptrs)
    stream = vec and len(keys) * h * w * 3 * SIZEOF[t] >= stream_min_bytes
    path = ('vector' if vec else 'element', 'stream' if stream else 'cached')
    if f == 'dense':
      return {('chain_fused_fwd_kernel', t) + path}
    return {('chain_fused_fwd_taps_kernel', t) + path + (fmt,)}
  if f in RAGGED_KERNEL:
    t, fmt = case['dtype'], case['fmt']
    cells = set()
    for launch in ragged_plan(t, fmt, addresses(keys, SIZEOF[t]), ys, stream_min_bytes):
      inst = (RAGGED_KERNEL[f], t, 'stream' if launch['stream'] else 'cached', launch['any_slow'])
      cells.add(inst if f == 'ragged' else inst + (fmt,))
    return cells
  ct, c = case['ct'], case['c']
  sizes = [size_of(k)[0] * size_of(k)[1] for k in keys]
  code_bytes = sum(sizes) * c * SIZEOF[ct]
  if f in CODES_KERNEL:
    t, fmt = case['dtype'], case['fmt']
    cells = set()
    for launch in ragged_plan(t, fmt, addresses(keys, SIZEOF[t], SIZEOF[ct]), ys, stream_min_bytes):
      inst = (CODES_KERNEL[f], ct, c, t, 'stream' if launch['stream'] else 'cached', fmt)
      cells |= _paths_cells(inst, [(launch['vec'] >> j) & 1 for j in range(launch['n'])])
    return cells
  codes_aligned = [k[1:] != 'c' for k in keys]
  if f == 'decode':
    t = case['dtype']
    ppv = 2 if t == 'f16' else 1
    pol = io(code_bytes + sum(sizes) * 3 * SIZEOF[t])
    cells = _paths_cells(('decode_kernel', ct, c, t, case['norm'], pol),
                         [a and hw % ppv == 0 for a, hw in zip(codes_aligned, sizes)])
    if case['norm']:
      cells |= {cell + ('decode_ragged',) for cell in _paths_cells(('decode_max_kernel', ct, c, pol), codes_aligned)}
    return cells
  if f in ('decode_tables', 'codes_max'):
    entry = 'decode_tables' if f == 'decode_tables' else 'codes_max_ragged'
    return {cell + (entry,) for cell in _paths_cells(('decode_max_kernel', ct, c, io(code_bytes)), codes_aligned)}
  assert f == 'lut'
  ot = case['ot']
  ppv = 12 // (3 * SIZEOF[ot])
  inst = ('codes_lut_kernel', ct, c, ot, io(code_bytes + sum(sizes) * 3 * SIZEOF[ot]), case['lds16'])
  return _paths_cells(inst, [a and hw % ppv == 0 for a, hw in zip(codes_aligned, sizes)])


def cells_run(cases=None):
  """every cell the cases select, in the parent (default threshold) and in the EXPO_STREAM_MIN_BYTES=1 child together"""
  cells = set()
  for case in (CASES if cases is None else cases):
    for smb in THRESHOLDS:
      cells |= case_cells(case, smb)
      if without_ys(case):
        cells |= case_cells(case, smb, ys=False)
  return cells


def family_counts():
  """{kernel: (cells run, cells enumerated)} for the commit message and DESIGN.md"""
  run, out = cells_run(), {}
  for cell in sorted(all_cells(), key=repr):
    inst = cell if not isinstance(cell[0], tuple) else cell[0]
    r, n = out.get(inst[0], (0, 0))
    out[inst[0]] = (r + (cell in run), n + 1)
  return out
