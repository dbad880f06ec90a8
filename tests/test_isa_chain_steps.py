"""The static ISA checks of tests/test_isa_sanity.py for csrc/chain_steps.hip (CPU-only: cross-compiles with -S, runs
nothing): no store whose address register lies inside its own data tuple, no scratch, and the kernels really are the
dwordx3 streaming kernels they claim to be (one group load per chunk, four 12-byte stores per step)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip('hipcc not available')
  out = str(tmp_path_factory.mktemp('isa') / 'chain_steps.s')
  # the flags csrc/build.sh compiles this unit with
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                         os.path.join(CSRC, 'chain_steps.hip'), '-o', out], stderr=subprocess.DEVNULL)
  txt = open(out).read()
  found = {}
  for m in re.finditer(r'^(_ZN4expo22chain_steps_fwd_kernel\w+):[^\n]*\n(.*?)\n\s*s_endpgm', txt, flags=re.S | re.M):
    found[m.group(1)] = m.group(2)
  meta = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, flags=re.S)}
  assert len(found) == 4 and set(found) == set(meta), (sorted(found), sorted(meta))  # fp16 / fp32 x IoStream / IoCached
  return found, meta


def test_build_script_compiles_the_unit_with_the_streaming_kernels_flags():
  sh = open(os.path.join(CSRC, 'build.sh')).read()
  line = [l for l in sh.splitlines() if 'chain_steps.hip' in l and l.lstrip().startswith('"$HIPCC"')]
  assert len(line) == 1 and '-fno-' not in line[0], line
  assert '"$TMP/chain_steps.o"' in sh.split('-shared')[1]


def test_no_store_takes_its_address_from_its_own_data_registers(kernels):
  checked = 0
  for name, body in kernels[0].items():
    for line in body.splitlines():
      m = re.search(r'buffer_store_dword(?:x(\d))?\s+(?:v(\d+)|v\[(\d+):(\d+)\]), v(\d+), s\[', line)
      if m:
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = int(m.group(2) if m.group(2) is not None else m.group(4))
        checked += 1
        assert not (lo <= int(m.group(5)) <= hi), '%s stores its own address register: %s' % (name, line.strip())
  assert checked >= 16


def test_no_scratch_and_the_streaming_access_pattern(kernels):
  found, meta = kernels
  for name, body in found.items():
    scratch = re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', meta[name])
    assert scratch is not None and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
    assert 'scratch_' not in body, name
    # the step loop is rolled: ONE group load and one group store in the code, whatever the number of steps
    assert len(re.findall(r'buffer_load_dwordx3', body)) == 4, name
    assert len(re.findall(r'buffer_store_dwordx3', body)) == 4, name
    policy = 'nt' if 'IoStream' in name else None
    for line in body.splitlines():
      if 'buffer_load_dwordx3' in line:
        assert (' nt' in line) == (policy == 'nt'), (name, line.strip())
      if 'buffer_store_dwordx3' in line:
        assert (' sc1' in line) == (policy == 'nt'), (name, line.strip())


def test_steps_round_to_half_with_the_instructions_of_the_per_step_kernels(kernels, tmp_path):
  """v_fma_mixlo_f16 / v_fma_mixhi_f16 round a * b + c once, v_fma_f32 + v_cvt_pk_f16_f32 twice (csrc/chain_steps.hip):
  a step of the fused kernel must convert with the same instructions as the per-step kernel of its filter.  The fused
  kernel holds each filter's step once, so its counts are the sums over the nine per-step forward kernels.  Totals only:
  two compensating changes in two filters would pass here.  The guard that decides is the GPU comparison on the 'large'
  shape of tests/test_hip_chain_fuse.py, which has to run after every compiler update."""
  out = str(tmp_path / 'exposure_hip.s')
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                         os.path.join(CSRC, 'exposure_hip.hip'), '-o', out], stderr=subprocess.DEVNULL)
  txt = open(out).read()
  pats = (r'v_fma_mixlo_f16', r'v_fma_mixhi_f16', r'v_cvt_pk_f16_f32', r'v_cvt_f16_f32', r'v_pk_\w+_f16')
  for io in ('IoStream', 'IoCached'):
    per_step = re.findall(r'^(_ZN4expo17filter_fwd_kernelI\w+DF16_Lb1ENS_8%sE\w+):[^\n]*\n(.*?)\n\s*s_endpgm' % io, txt,
                          flags=re.S | re.M)
    assert len(per_step) == 9, [name for name, _ in per_step]
    fused = [body for name, body in kernels[0].items() if 'DF16_' in name and io in name]
    assert len(fused) == 1
    for pat in pats:
      want = sum(len(re.findall(pat, body)) for _, body in per_step)
      assert len(re.findall(pat, fused[0])) == want, (io, pat, want)
