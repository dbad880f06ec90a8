"""Static checks of csrc/chain_steps_bwd_seq.hip in the style of tests/test_isa_chain_steps_bwd_rc.py (CPU-only:
cross-compiles with -S, runs nothing): one kernel per (entry of EXPO_RUN_SEQUENCES, cache policy), every one without
scratch and without a spilled register, the dwordx3 streaming access pattern of a run that loads one pair per group and
stores every step's dx, and the conversions to half of the per-step backward AND forward kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only']  # csrc/build.sh, both units
FILTERS = {0: 'ExposureF', 1: 'GammaF', 2: 'WhiteBalanceF', 3: 'SatPlusF', 8: 'LevelF'}  # EXPO_RUN_FILTERS
STORAGE = {'half_t': 'DF16_', 'float': 'f'}
KERNEL = r'_ZN4expo26chain_steps_bwd_seq_kernel\w+'


def table():
  """The entries of EXPO_RUN_SEQUENCES that are on: [(mangled storage type, hsv_grad_mode, ids from the head down)]."""
  src = open(os.path.join(CSRC, 'chain_steps_bwd_seq.hip')).read()
  macro = re.search(r'#define EXPO_RUN_SEQUENCES\(X\)(.*?)\n\n', src, flags=re.S).group(1)
  rows = re.findall(r'X\((\w+), EXPO_F(?:16|32), ([01]), ([01]), ([\d, ]+)\)', macro)
  assert len(rows) == macro.count('X(') >= 3
  return [(STORAGE[t], int(mode), tuple(int(i) for i in ids.split(','))) for t, mode, on, ids in rows if on == '1']


def kernel_name(storage, mode, io, ids):
  return '_ZN4expo26chain_steps_bwd_seq_kernelI%sLi%dENS_8%sEJ%sEEEvNS_17ChainStepsBwdArgsIXsZT2_EEE' % (
      storage, mode, io, ''.join('Li%dE' % i for i in ids))


def listing(unit, out):
  subprocess.check_call([HIPCC] + FLAGS + [os.path.join(CSRC, unit), '-o', out], stderr=subprocess.DEVNULL)
  return open(out).read()


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip('hipcc not available')
  txt = listing('chain_steps_bwd_seq.hip', str(tmp_path_factory.mktemp('isa') / 'chain_steps_bwd_seq.s'))
  found = {}
  for m in re.finditer(r'^(%s):[^\n]*\n(.*?)\n\s*s_endpgm' % KERNEL, txt, flags=re.S | re.M):
    found[m.group(1)] = m.group(2)
  meta = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, flags=re.S)}
  notes = {}
  for m in re.finditer(r'\.name:\s+(%s)\n(.*?)\.wavefront_size' % KERNEL, txt, flags=re.S):
    notes[m.group(1)] = m.group(2)
  return found, meta, notes


def test_the_required_entries_are_on():
  rows = table()
  for want in (('DF16_', 0, (3, 2, 1, 0)), ('DF16_', 1, (3, 2, 1, 0)), ('f', 0, (3, 2, 1, 0))):
    assert want in rows, (want, rows)
  assert len(set(rows)) == len(rows)


def test_build_script_compiles_the_unit_with_the_streaming_kernels_flags():
  sh = open(os.path.join(CSRC, 'build.sh')).read()
  line = [l for l in sh.splitlines() if 'chain_steps_bwd_seq.hip' in l and l.lstrip().startswith('"$HIPCC"')]
  ref = [l for l in sh.splitlines() if '/exposure_hip.hip' in l and l.lstrip().startswith('"$HIPCC"')]
  assert len(line) == 1 and len(ref) == 1 and '-f' not in line[0].split('"$@"')[0].replace('"${FLAGS[@]}"', ''), line
  assert line[0].split(' -c ')[0] == ref[0].split(' -c ')[0]
  assert '"$TMP/chain_steps_bwd_seq.o"' in sh.split('-shared')[1]


def test_one_kernel_per_entry_and_cache_policy(kernels):
  found, meta, notes = kernels
  want = {kernel_name(s, mode, io, ids) for s, mode, ids in table() for io in ('IoStream', 'IoCached')}
  assert set(found) == set(meta) == set(notes) == want, sorted(set(found) ^ want)


def test_no_scratch_no_spills(kernels, capsys):
  found, meta, notes = kernels
  rows = []
  for name in sorted(found):
    scratch = re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', meta[name])
    assert scratch is not None and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
    assert 'scratch_' not in found[name], name
    for key in ('sgpr_spill_count', 'vgpr_spill_count'):
      got = re.search(r'\.%s:\s+(\d+)' % key, notes[name])
      assert got is not None and int(got.group(1)) == 0, (name, key, got and got.group(1))
    assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', notes[name]).group(1)) == 0, name
    # (gfx950: .vgpr_count is the unified count, accumulation registers included; allocated in blocks of 8 of the 512
    # a SIMD lane has, at most 8 waves)
    total = int(re.search(r'\.vgpr_count:\s+(\d+)', notes[name]).group(1))
    assert 0 < total <= 512, (name, total)
    waves = min(8, 512 // (-(-total // 8) * 8))
    # the accumulators are registers here: no LDS but block_reduce_record's own, and at least two waves per SIMD
    assert waves >= 2, (name, total)
    rows.append((name, total, int(re.search(r'\.sgpr_count:\s+(\d+)', notes[name]).group(1)), waves))
  with capsys.disabled():  # the record: registers and the waves per SIMD they leave
    for name, total, sgprs, waves in rows:
      print('\n%s: %d registers (%d scalar), %d waves per SIMD' % (name, total, sgprs, waves), end='')


def test_the_streaming_access_pattern(kernels):
  for name, body in kernels[0].items():
    ns = len(re.search(r'EJ((?:Li\dE)+)EEEv', name).group(1)) // 4
    # loads: the first group's pair (the head's dy, the lowest step's x) and the next group's pair, four dwordx3 each.
    # stores: every step's dx (the steps are straight-line code), four dwordx3 each
    assert len(re.findall(r'buffer_load_dwordx3', body)) == 4 * (2 + 2), name
    assert len(re.findall(r'buffer_store_dwordx3', body)) == 4 * ns, name
    stream = 'IoStream' in name
    for line in body.splitlines():
      if 'buffer_load_dwordx3' in line:
        assert (' nt' in line) == stream, (name, line.strip())
      if 'buffer_store_dwordx3' in line:
        assert (' sc1' in line) == stream, (name, line.strip())
      m = re.search(r'buffer_store_dword(?:x(\d))?\s+(?:v(\d+)|v\[(\d+):(\d+)\]), v(\d+), s\[', line)
      if m:  # no store takes its address from its own data registers (tests/test_isa_sanity.py)
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = int(m.group(2) if m.group(2) is not None else m.group(4))
        assert not (lo <= int(m.group(5)) <= hi), '%s stores its own address register: %s' % (name, line.strip())


def test_steps_round_to_half_with_the_instructions_of_the_per_step_kernels(kernels, tmp_path):
  """v_fma_mixlo_f16 / v_fma_mixhi_f16 round a * b + c once, v_fma_f32 + v_cvt_pk_f16_f32 twice (csrc/chain_steps.hip).
  An fp16 kernel holds every step's backward body once, converting like filter_bwd_kernel<F, half, VEC, HAS_DX, MODE of
  that filter, IO>, and the forward body of every step below the head once, converting like filter_fwd_kernel<F, half,
  VEC, IO>.  Totals only; the guard that decides is the GPU comparison of tests/test_hip_chain_bwd_seq.py and the
  'large' shapes of tests/test_hip_chain_bwd_runs.py."""
  txt = listing('exposure_hip.hip', str(tmp_path / 'exposure_hip.s'))
  pats = (r'v_fma_mixlo_f16', r'v_fma_mixhi_f16', r'v_cvt_pk_f16_f32', r'v_cvt_f16_f32')

  def per_step(regex):
    got = re.findall(r'^(%s\w+):[^\n]*\n(.*?)\n\s*s_endpgm' % regex, txt, flags=re.S | re.M)
    assert len(got) == 1, (regex, [name for name, _ in got])
    return got[0][1]

  checked = 0
  for storage, mode, ids in table():
    if storage != 'DF16_':
      continue
    for io in ('IoStream', 'IoCached'):
      parts = []
      for k, fid in enumerate(ids):
        f = FILTERS[fid]
        parts.append(per_step(r'_ZN4expo17filter_bwd_kernelINS_%d%sEDF16_Lb1ELb1ELi%dENS_8%sE'
                              % (len(f), f, mode if f == 'SatPlusF' else 0, io)))
        if k > 0:  # a step below the head: its forward is swept
          parts.append(per_step(r'_ZN4expo17filter_fwd_kernelINS_%d%sEDF16_Lb1ENS_8%sE' % (len(f), f, io)))
      body = kernels[0][kernel_name(storage, mode, io, ids)]
      for pat in pats:
        want = sum(len(re.findall(pat, part)) for part in parts)
        assert len(re.findall(pat, body)) == want, (storage, mode, io, ids, pat, want, len(re.findall(pat, body)))
      checked += 1
  assert checked >= 4
