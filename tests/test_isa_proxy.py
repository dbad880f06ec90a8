"""The static ISA checks of tests/test_isa_sanity.py for csrc/proxy.hip (CPU-only: cross-compiles with -S, runs
nothing): no scratch, no store whose address registers lie inside its own data tuple, and -- the unit's contract is
"every float32 operation rounded on its own" -- no fused multiply-add anywhere in the kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def build_line():
  sh = open(os.path.join(CSRC, 'build.sh')).read()
  line = [l for l in sh.splitlines() if 'proxy.hip' in l and l.lstrip().startswith('"$HIPCC"')]
  assert len(line) == 1, line
  return sh, line[0]


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip('hipcc not available')
  # the flags on the unit's line of csrc/build.sh, beyond the common ones
  extra = [f for f in build_line()[1].split() if f.startswith('-f')]
  assert extra == ['-ffp-contract=off'], extra
  out = str(tmp_path_factory.mktemp('isa') / 'proxy.s')
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only'] + extra +
                        [os.path.join(CSRC, 'proxy.hip'), '-o', out], stderr=subprocess.DEVNULL)
  txt = open(out).read()
  found = {m.group(1): m.group(2)
           for m in re.finditer(r'^(_ZN4expo\w*bilinear_resize_kernel\w+):[^\n]*\n(.*?)\n\s*s_endpgm', txt, flags=re.S | re.M)}
  meta = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, flags=re.S)}
  assert len(found) == 4 and set(found) == set(meta), (sorted(found), sorted(meta))  # fp16 / fp32 in x fp16 / fp32 out
  return found, meta, txt


def test_build_script_compiles_the_unit_without_contraction_and_links_it():
  sh, line = build_line()
  assert '-ffp-contract=off' in line and '-fno-' not in line and '-ffast-math' not in line, line
  assert '"$TMP/proxy.o"' in sh.split('-shared')[1]


def test_no_scratch_and_no_spills(kernels):
  found, meta, txt = kernels
  for name, body in found.items():
    scratch = re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', meta[name])
    assert scratch is not None and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
    assert 'scratch_' not in body, name
  spills = re.findall(r'\.[sv]gpr_spill_count:\s+(\d+)', txt)  # the kernels' metadata: two counts each
  assert len(spills) == 8 and all(int(c) == 0 for c in spills), spills


def test_no_store_takes_its_address_from_its_own_data_registers(kernels):
  """The dwordx3 address / data overlap scan of tests/test_isa_sanity.py, for the forms this unit stores with: a
  global store's address is a register pair, a buffer store's one register."""
  checked = 0
  for name, body in kernels[0].items():
    for line in body.splitlines():
      m = re.search(r'global_store_\w+\s+v\[(\d+):(\d+)\], (?:v(\d+)|v\[(\d+):(\d+)\]), ', line)
      if m:
        alo, ahi = int(m.group(1)), int(m.group(2))
        lo = int(m.group(3) if m.group(3) is not None else m.group(4))
        hi = int(m.group(3) if m.group(3) is not None else m.group(5))
        checked += 1
        assert ahi < lo or alo > hi, '%s stores its own address registers: %s' % (name, line.strip())
      m = re.search(r'buffer_store_dword(?:x(\d))?\s+(?:v(\d+)|v\[(\d+):(\d+)\]), v(\d+), s\[', line)
      if m:
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = int(m.group(2) if m.group(2) is not None else m.group(4))
        checked += 1
        assert not (lo <= int(m.group(5)) <= hi), '%s stores its own address register: %s' % (name, line.strip())
    assert not re.search(r'flat_store', body), name
  assert checked >= 4  # every kernel stores, and the patterns still match what the compiler prints


def test_nothing_is_contracted(kernels):
  for name, body in kernels[0].items():
    for op in ('v_fma_f32', 'v_fmac_f32', 'v_mad_f32', 'v_pk_fma_f32', 'v_fma_mix', 'v_fma_f16', 'v_mac_f32'):
      assert op not in body, (name, op)
    # the arithmetic that must be there instead: separate multiplies and adds
    assert re.search(r'v_(pk_)?mul_f32', body) and re.search(r'v_(pk_)?add_f32', body), name


def test_a_threads_taps_are_loaded_before_the_first_is_used(kernels):
  """Latency-bound: no wait on a vector-memory counter before the last global load of the kernel has been issued."""
  for name, body in kernels[0].items():
    lines = body.splitlines()
    loads = [i for i, l in enumerate(lines) if re.search(r'\bglobal_load_', l)]
    assert loads, name
    waits = [i for i, l in enumerate(lines) if 'vmcnt' in l]
    assert waits and min(waits) > max(loads), (name, min(waits), max(loads))
