"""Helper of tests/test_hip_policy_matrix.py (not a test module), modelled on tests/_chain_bwd_pairs_child.py.

EXPO_STREAM_MIN_BYTES is read once per process, so the IoStream instantiations of the cases run in ONE child process:

    EXPO_STREAM_MIN_BYTES=1 python tests/_policy_matrix_child.py OUT.npz

runs every case of tests/_policy_matrix_cases.py::CASES and writes every output -- each image's y and tap planes, the
decoded images, tables, maxima and pictures -- to OUT.npz under '<case id>|<name>', plus 'env', the EXPO_* variables the
child saw.  The parent runs the same function (run_case) in process, under the default threshold.

The module also holds what both sides and the references share: the inputs, the drawn parameter rows, load_image's
float32 maths with the normalisation as a flag, and the float64 chains."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import _policy_matrix_cases as pm  # noqa: E402

NP_T = {'f16': np.float16, 'f32': np.float32, 'u8': np.uint8, 'u16': np.uint16}
KEPT = [k for k in range(pm.STEPS) if (pm.TAP_MASK >> k) & 1]
# which reference chain a family's outputs are held to
CHAIN_OF = {'dense': 'p24', 'dense_taps': 'p24', 'ragged': 'p24', 'ragged_taps': 'p24', 'codes': 'p24',
            'masked': 'masked', 'curves': 'curves', 'curves_codes': 'curves'}


# ---------------------------------------------------------------------------------------------------------------------
# inputs and parameter rows (host arrays, made once)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_image(key):
  """(h, w, 3) fp16 values, which the fp32 runs take as they are: tests/test_hip_chain_taps.py::inputs -- values past 1,
  below 0 and on .5/255 ties"""
  import torch
  from tests.test_hip_chain_taps import inputs
  h, w = pm.size_of(key)
  return inputs(np.random.default_rng(9100 + pm.IMAGE_KEYS.index(key)), (h, w, 3), torch.float16).numpy()


@functools.lru_cache(maxsize=None)
def code_image(ct, c, key):
  """(h, w, c) codes, none of them 0 in every sample (an all-zero image normalises to NaN)"""
  h, w = pm.size_of(key)
  rng = np.random.default_rng(9300 + 1000 * pm.CODE_TYPES.index(ct) + 100 * c + pm.IMAGE_KEYS.index(key))
  return np.maximum(rng.integers(0, 256 if ct == 'u8' else 65536, (h, w, c), dtype=NP_T[ct]), 1)


@functools.lru_cache(maxsize=None)
def rows(chain):
  """The rows of every image key, in pm.IMAGE_KEYS order: {'ids' (n, 5)} and 'p' (n, 5, 24) from synthetic.make_params;
  'masked': also 'mp' and the oracle's 'raw' (tests/test_hip_masked_chain.py::make_rows); 'curves': 'p' (n, 5, 48) from
  the oracle's regressors with cfg.curve_steps = 5 (tests/test_hip_curves_chain.py::make_rows)"""
  ids = np.array([pm.SEQUENCES[k] for k in pm.IMAGE_KEYS], dtype=np.int32)
  rng = np.random.default_rng({'p24': 9501, 'masked': 9502, 'curves': 9503}[chain])
  if chain == 'p24':
    from tests.test_hip_masked_chain import make_rows
    return {'ids': ids, 'p': make_rows(rng, ids)[0]}
  if chain == 'masked':
    from tests.test_hip_masked_chain import make_rows
    p, mp, raw = make_rows(rng, ids)
    return {'ids': ids, 'p': p, 'mp': mp, 'raw': raw}
  from tests.test_hip_curves_chain import make_rows
  return {'ids': ids, 'p': make_rows(rng, ids, pm.CURVE_STEPS)}


def c3(codes):
  """the codes of the three output channels (C = 1: replicated; C = 4: alpha dropped)"""
  return np.repeat(codes, 3, axis=2) if codes.shape[2] == 1 else codes[:, :, :3]


def host_decode(codes, kind, normalize):
  """load_image's float32 expressions on (H, W, C) codes, its scaling by 1 / (2 max) as a flag: with the kind's own flag
  (evaluate.DECODE_NORMALIZE) this is tests/test_hip_decode.py::host_math"""
  from exposure_amd import evaluate
  v = c3(codes).astype(np.float32) / (255.0 if kind == 'srgb8' else 65535.0)
  img = evaluate.linearize_ProPhotoRGB(v) if kind == 'prophoto16' else v**2.2
  return img / (2 * img.max()) if normalize else img


@functools.lru_cache(maxsize=None)
def decoded_input(ct, c, dtype, key):
  """what a pass from codes gathers: the decoded image in the storage dtype"""
  from exposure_amd import evaluate
  kind = pm.codes_kind(ct, c)
  return host_decode(code_image(ct, c, key), kind, evaluate.DECODE_NORMALIZE[kind]).astype(NP_T[dtype])


# ---------------------------------------------------------------------------------------------------------------------
# the float64 references
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(chain, source, key):
  """The float64 image after every step of image `key`'s sequence, no rounding between steps.  source: 'float' (the
  fp16-valued float_image) or (ct, c, dtype) (decoded_input)."""
  from oracle import filters_np as fnp
  x = float_image(key) if source == 'float' else decoded_input(*source, key)
  r = rows(chain)
  i = pm.IMAGE_KEYS.index(key)
  ids, p = r['ids'][i], r['p'][i]
  if chain == 'masked':
    from tests.test_hip_masked_chain import oracle_steps
    return oracle_steps(x, ids, p, r['raw'][i])
  if chain == 'curves':
    from tests.test_hip_curves_chain import oracle_steps
    return oracle_steps(x, ids, p, pm.CURVE_STEPS)
  cur, out = np.asarray(x, dtype=np.float64)[None], []
  for k, fid in enumerate(ids):  # tests/test_hip_ragged_chain.py::test_ragged_matches_the_float64_chain
    fid = int(fid)
    cur = np.zeros_like(cur) if fid < 0 else fnp.process_packed(fid, cur, p[k:k + 1, :fnp.NUM_PARAMS[fid]].astype(
        np.float64))
    out.append(cur[0])
  return out


def source_of(case):
  return (case['ct'], case['c'], case['dtype']) if case['family'] in pm.CODES_KERNEL else 'float'


def references_used():
  """every (chain, source, key) some case is compared with"""
  used = set()
  for case in pm.CASES:
    if case['family'] in CHAIN_OF:
      used |= {(CHAIN_OF[case['family']], source_of(case), key) for key in pm.case_images(case)}
  return sorted(used, key=repr)


def lut_tables(case):
  """a random table per image, every entry drawn on its own, so a wrong entry cannot hide"""
  n, entries = len(pm.LUT_IMAGES), 1 << (8 * pm.SIZEOF[case['ct']])
  rng = np.random.default_rng(9700 + pm.CASE_IDS.index(case['id']))
  return rng.integers(0, 1 << (8 * pm.SIZEOF[case['ot']]), (n, entries)).astype(NP_T[case['ot']])


# ---------------------------------------------------------------------------------------------------------------------
# one case on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def run_case(case, dev):
  """Runs the case's call (and, where pm.without_ys says so, its repetition with ys = NULL) under this process's cache
  policy -> {name: host array}.  Outputs and tap planes sit in guarded buffers, and the guards are checked; every base
  has the alignment the ledger assumes."""
  import torch
  from exposure_amd import _cabi, evaluate
  from tests.test_hip_fused_decode import guarded, guards_intact
  TT = {'f16': torch.float16, 'f32': torch.float32, 'u8': torch.uint8, 'u16': torch.uint16}
  f = case['family']
  keys = pm.case_images(case)
  out, bufs = {}, []

  def host(t):
    return evaluate._host_codes(t) if t.dtype in (torch.uint8, torch.uint16) else t.cpu().numpy()

  def place(a, off=0):
    """a's values in a device buffer of their own, `off` elements in"""
    src = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    buf = torch.empty(off + src.numel(), dtype=src.dtype, device=dev)
    t = buf[off:off + src.numel()].view(src.shape)
    t.copy_(src)
    assert t.data_ptr() % 4 == (off * src.element_size()) % 4
    return t

  def guard(shape, dtype, off=0):
    b, t = guarded(shape, dtype, off)
    assert t.data_ptr() % 4 == (off * t.element_size()) % 4
    bufs.append((b, t, dtype))
    return t

  def check_guards():
    torch.cuda.synchronize()
    for b, t, dtype in bufs:
      assert guards_intact(b, t, dtype), '%s: guard elements overwritten' % case['id']

  if f in CHAIN_OF:
    t = case['dtype']
    fmt = case['fmt']
    tdt = {pm.TAP_NONE: None, pm.TAP_STORAGE: TT[t], pm.TAP_U8: torch.uint8, pm.TAP_U16: torch.uint16}[fmt]
    mask = pm.TAP_MASK if tdt is not None else 0
    r = rows(CHAIN_OF[f])
    sel = [pm.IMAGE_KEYS.index(k) for k in keys]
    ids = torch.from_numpy(np.ascontiguousarray(r['ids'][sel])).to(dev)
    p = torch.from_numpy(np.ascontiguousarray(r['p'][sel])).to(dev)

    if f in ('dense', 'dense_taps'):
      x = place(np.stack([float_image(k) for k in keys]).astype(NP_T[t]))
      for name, with_y in [('', True)] + ([('_only', False)] if pm.without_ys(case) else []):
        y = guard(tuple(x.shape), TT[t]) if with_y else None
        taps = guard((len(KEPT),) + tuple(x.shape), tdt) if mask else None
        if f == 'dense':
          _cabi.chain_fused_fwd(ids, p, x, y)
        else:
          _cabi.chain_fused_fwd_taps(ids, p, x, y, mask, taps)
        check_guards()
        for i, k in enumerate(keys):
          if with_y:
            out['%s.y' % k] = host(y[i])
          if mask:
            out['%s.tap%s' % (k, name)] = host(taps[:, i])
      return out

    if f in pm.CODES_KERNEL:
      ct, c = case['ct'], case['c']
      kind = pm.codes_kind(ct, c)
      xs = [place(code_image(ct, c, k), int(k[1:] == 'c')) for k in keys]
      tables, stride = _cabi.decode_tables(xs, evaluate.decode_table(kind, dev), evaluate.DECODE_NORMALIZE[kind], TT[t])
    else:
      xs = [place(float_image(k).astype(NP_T[t]), int(k[1:] == 'x')) for k in keys]
    for name, with_y in [('', True)] + ([('_only', False)] if pm.without_ys(case) else []):
      ys = [guard(pm.size_of(k) + (3,), TT[t], int(k[1:] == 'y')) for k in keys] if with_y else None
      taps = [guard((len(KEPT),) + pm.size_of(k) + (3,), tdt, int(k[1:] == 't')) for k in keys] if mask else None
      if f == 'ragged':
        _cabi.chain_fused_fwd_ragged(ids, p, xs, ys)
      elif f == 'ragged_taps':
        _cabi.chain_fused_fwd_ragged_taps(ids, p, xs, ys, mask, taps)
      elif f == 'masked':
        mp = torch.from_numpy(np.ascontiguousarray(r['mp'][sel])).to(dev)
        _cabi.chain_fused_masked_fwd_ragged(ids, p, mp, xs, ys, pm.SHARP, pm.MIN_STRENGTH, mask, taps)
      elif f == 'curves':
        _cabi.chain_fused_curves_fwd_ragged(ids, p, pm.CURVE_STEPS, xs, ys, mask, taps)
      elif f == 'codes':
        _cabi.chain_fused_fwd_ragged_codes(ids, p, xs, tables, stride, ys, mask, taps)
      else:
        _cabi.chain_fused_curves_fwd_ragged_codes(ids, p, pm.CURVE_STEPS, xs, tables, stride, ys, mask, taps)
      check_guards()
      for i, k in enumerate(keys):
        if with_y:
          out['%s.y' % k] = host(ys[i])
        if mask:
          out['%s.tap%s' % (k, name)] = host(taps[i])
    return out

  ct, c = case['ct'], case['c']
  cs = [place(code_image(ct, c, k), int(k[1:] == 'c')) for k in keys]
  if f == 'decode':
    kind = pm.DECODE_KIND[(ct, case['norm'])]
    ys = [guard(pm.size_of(k) + (3,), TT[case['dtype']]) for k in keys]
    _cabi.decode_ragged(cs, evaluate.decode_table(kind, dev), int(case['norm']), ys)
    check_guards()
    return {'%s.y' % k: host(y) for k, y in zip(keys, ys)}
  if f == 'decode_tables':
    table = evaluate.decode_table(pm.DECODE_KIND[(ct, True)], dev)
    tables, stride = _cabi.decode_tables(cs, table, 1, TT[TABLES_DTYPE[ct]])
    torch.cuda.synchronize()
    assert stride == tables.shape[1]
    return {'tables': host(tables)}
  if f == 'codes_max':
    return {'maxima': host(_cabi.codes_max_ragged(cs))}
  assert f == 'lut'
  luts = torch.from_numpy(lut_tables(case)).to(dev)
  assert luts.data_ptr() % 16 == 0 and luts.shape[1] % 16 == 0  # what the LDS-staged kernel asks of its tables
  ys = [guard(pm.size_of(k) + (3,), TT[case['ot']]) for k in keys]
  before = os.environ.get('EXPO_CODES_LUT_LDS16')
  os.environ['EXPO_CODES_LUT_LDS16'] = '1' if case['lds16'] else '0'  # (read at every call)
  try:
    _cabi.codes_lut_ragged(cs, luts, luts.shape[1], ys)
  finally:
    if before is None:
      del os.environ['EXPO_CODES_LUT_LDS16']
    else:
      os.environ['EXPO_CODES_LUT_LDS16'] = before
  check_guards()
  return {'%s.y' % k: host(y) for k, y in zip(keys, ys)}


TABLES_DTYPE = {'u8': 'f16', 'u16': 'f32'}  # decode_tables' storage dtype is no parameter of decode_max_kernel


def main(argv):
  import torch
  dev = torch.device('cuda:0')
  out = {'env': np.array(json.dumps({k: v for k, v in os.environ.items() if k.startswith('EXPO_')}))}
  for case in pm.CASES:
    for name, a in run_case(case, dev).items():
      out['%s|%s' % (case['id'], name)] = a
  np.savez(argv[1], **out)
  return 0


if __name__ == '__main__':
  sys.exit(main(sys.argv))
