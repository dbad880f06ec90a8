"""Static checks of csrc/chain_steps_bwd_rc.hip in the style of tests/test_isa_chain_steps_bwd.py (CPU-only:
cross-compiles with -S, runs nothing): every kernel without scratch and without a spilled register, the dwordx3 streaming
access pattern of a run that loads one pair per group, and the conversions to half of the per-step backward AND forward
kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only']  # csrc/build.sh, both units
RUN_FILTERS = ('ExposureF', 'GammaF', 'WhiteBalanceF', 'SatPlusF', 'LevelF')  # EXPO_RUN_FILTERS
# EXPO_RC_FILTERS of the unit: the forwards the kernel recomputes, per storage type
RC_FILTERS = {'DF16_': ('ExposureF', 'GammaF', 'WhiteBalanceF', 'SatPlusF', 'LevelF'),
              'f': ('ExposureF', 'GammaF', 'WhiteBalanceF', 'SatPlusF', 'LevelF')}
RUN_LENGTHS = range(2, 9)  # one instantiation per run length, 2 .. kChainFuseMax
KERNEL = r'_ZN4expo25chain_steps_bwd_rc_kernel\w+'


def listing(unit, out):
  subprocess.check_call([HIPCC] + FLAGS + [os.path.join(CSRC, unit), '-o', out], stderr=subprocess.DEVNULL)
  return open(out).read()


def run_length(name):
  return int(re.search(r'Li(\d)EEEvNS', name).group(1))


def storage(name):
  return 'DF16_' if 'kernelIDF16_' in name else 'f'


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip('hipcc not available')
  txt = listing('chain_steps_bwd_rc.hip', str(tmp_path_factory.mktemp('isa') / 'chain_steps_bwd_rc.s'))
  found = {}
  for m in re.finditer(r'^(%s):[^\n]*\n(.*?)\n\s*s_endpgm' % KERNEL, txt, flags=re.S | re.M):
    found[m.group(1)] = m.group(2)
  meta = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, flags=re.S)}
  notes = {}
  for m in re.finditer(r'\.name:\s+(%s)\n(.*?)\.wavefront_size' % KERNEL, txt, flags=re.S):
    notes[m.group(1)] = m.group(2)
  # fp16 / fp32 x hsv_grad_mode 0 / 1 x IoStream / IoCached x run length
  assert len(found) == 8 * len(RUN_LENGTHS) and set(found) == set(meta) == set(notes), (len(found), len(meta), len(notes))
  return found, meta, notes


def test_build_script_compiles_the_unit_with_the_streaming_kernels_flags():
  sh = open(os.path.join(CSRC, 'build.sh')).read()
  line = [l for l in sh.splitlines() if 'chain_steps_bwd_rc.hip' in l and l.lstrip().startswith('"$HIPCC"')]
  ref = [l for l in sh.splitlines() if '/exposure_hip.hip' in l and l.lstrip().startswith('"$HIPCC"')]
  assert len(line) == 1 and len(ref) == 1 and '-f' not in line[0].split('"$@"')[0].replace('"${FLAGS[@]}"', ''), line
  assert line[0].split(' -c ')[0] == ref[0].split(' -c ')[0]
  assert '"$TMP/chain_steps_bwd_rc.o"' in sh.split('-shared')[1]


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
    rows.append((name, total, min(8, 512 // (-(-total // 8) * 8))))
  with capsys.disabled():  # the record: registers and the waves per SIMD they leave
    for name, total, waves in rows:
      print('\n%s: %d registers, %d waves per SIMD' % (name, total, waves), end='')


def test_the_streaming_access_pattern(kernels):
  for name, body in kernels[0].items():
    ns = int(run_length(name))
    # loads: the first group's pair (the head's dy, the lowest step's x) and the next group's pair, four dwordx3 each;
    # where the table leaves a forward out, a kept load per slot above the lowest, for the first and for the next group.
    # stores: the running step's dx (the backward step loop is rolled) -- whatever the run's length
    kept = 0 if set(RC_FILTERS[storage(name)]) == set(RUN_FILTERS) else ns - 1
    assert len(re.findall(r'buffer_load_dwordx3', body)) == 4 * (2 + 2 + 2 * kept), name
    assert len(re.findall(r'buffer_store_dwordx3', body)) == 4, name
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
  The backward step loop is rolled: the kernel holds each run filter's backward body once, converting like
  filter_bwd_kernel<F, half, VEC, HAS_DX, MODE of that filter, IO>.  The forward sweep is unrolled over the NS - 1 slots
  above the lowest step, and every slot holds the forward body of each filter of the recomputable table once, converting
  like filter_fwd_kernel<F, half, VEC, IO>.  Totals only; the guard that decides is the GPU comparison on the 'large'
  shapes of tests/test_hip_chain_bwd_runs.py and tests/test_hip_chain_bwd_recompute.py."""
  txt = listing('exposure_hip.hip', str(tmp_path / 'exposure_hip.s'))
  pats = (r'v_fma_mixlo_f16', r'v_fma_mixhi_f16', r'v_cvt_pk_f16_f32', r'v_cvt_f16_f32')
  for io in ('IoStream', 'IoCached'):
    fwd = []
    for f in RC_FILTERS['DF16_']:
      got = re.findall(r'^(_ZN4expo17filter_fwd_kernelINS_%d%sEDF16_Lb1ENS_8%sE\w+):[^\n]*\n(.*?)\n\s*s_endpgm'
                       % (len(f), f, io), txt, flags=re.S | re.M)
      assert len(got) == 1, (f, io, [name for name, _ in got])
      fwd.append(got[0][1])
    for mode in (0, 1):
      bwd = []
      for f in RUN_FILTERS:
        m = mode if f == 'SatPlusF' else 0
        got = re.findall(r'^(_ZN4expo17filter_bwd_kernelINS_%d%sEDF16_Lb1ELb1ELi%dENS_8%sE\w+):[^\n]*\n(.*?)\n\s*s_endpgm'
                         % (len(f), f, m, io), txt, flags=re.S | re.M)
        assert len(got) == 1, (f, m, io, [name for name, _ in got])
        bwd.append(got[0][1])
      fused = {name: body for name, body in kernels[0].items() if 'IDF16_Li%dENS_8%sE' % (mode, io) in name}
      assert len(fused) == len(RUN_LENGTHS)
      for pat in pats:
        per_bwd = sum(len(re.findall(pat, body)) for body in bwd)
        per_fwd = sum(len(re.findall(pat, body)) for body in fwd)
        for name, body in fused.items():
          want = per_bwd + (run_length(name) - 1) * per_fwd
          assert len(re.findall(pat, body)) == want, (name, pat, want, len(re.findall(pat, body)))
