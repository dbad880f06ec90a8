"""The static ISA checks of tests/test_isa_curves_chain.py for csrc/chain_fused_curves_codes.hip (CPU-only:
cross-compiles with -S, runs nothing): the unit is built and linked with chain_fused.hip's flags, instantiates its 96
kernels and nothing else, none of them uses scratch or spills a vector register, no store takes its address from inside
its own data registers, and the table gather of the 16-bit kernels stays a global load (nothing in the
unit pins a pointer or a value into a register by hand)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
UNIT = 'chain_fused_curves_codes.hip'


def build_line(unit=UNIT):
  sh = open(os.path.join(CSRC, 'build.sh')).read()
  line = [l for l in sh.splitlines() if '/%s"' % unit in l and l.lstrip().startswith('"$HIPCC"')]
  assert len(line) == 1, line
  return sh, line[0]


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip('hipcc not available')
  extra = [f for f in build_line()[1].split() if f.startswith('-f')]  # the flags beyond the common ones
  out = str(tmp_path_factory.mktemp('isa') / 'chain_fused_curves_codes.s')
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only'] + extra +
                        [os.path.join(CSRC, UNIT), '-o', out], stderr=subprocess.DEVNULL)
  txt = open(out).read()
  found = {m.group(1): m.group(2)
           for m in re.finditer(r'^(_ZN4expo\w*chain_fused_fwd_ragged_codes_kernel\w+):[^\n]*\n(.*?)\n\s*s_endpgm', txt,
                                flags=re.S | re.M)}
  meta = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, flags=re.S)}
  return found, meta, txt


def test_build_script_compiles_the_unit_with_the_fused_passes_flags_and_links_it():
  sh, line = build_line()
  fused = [f for f in build_line('chain_fused.hip')[1].split() if f.startswith('-f')]
  assert [f for f in line.split() if f.startswith('-f')] == fused == ['-fno-slp-vectorize', '-fno-honor-nans'], line
  assert '"$TMP/chain_fused_curves_codes.o"' in sh.split('-shared')[1]
  # the units it shares code with keep one build line each (their own tests filter by name)
  for unit in ('chain_fused_curves.hip', 'chain_fused_codes.hip'):
    build_line(unit)


def test_96_kernels_and_nothing_else(kernels):
  found, meta, txt = kernels
  # <u8, u16 codes> x <1, 3, 4 channels> x <fp16, fp32> x <cached, streaming> x <no taps, storage, u8, u16>
  assert len(found) == 96 and set(found) == set(meta), (sorted(found), sorted(meta))
  assert txt.count('.amdhsa_kernel ') == 96
  assert 'chain_fused_curves_ragged_kernel' not in txt and 'chain_fused_fwd_ragged_taps_kernel' not in txt


def test_no_scratch_and_no_vector_spills(kernels):
  found, meta, txt = kernels
  for name, body in found.items():
    scratch = re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', meta[name])
    assert scratch is not None and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
    assert 'scratch_' not in body, name
  spills = re.findall(r'\.vgpr_spill_count:\s+(\d+)', txt)  # the kernels' metadata
  assert len(spills) == 96 and all(int(c) == 0 for c in spills), spills


def test_no_store_takes_its_address_from_its_own_data_registers(kernels):
  """The address / data overlap scan of tests/test_isa_curves_chain.py: the buffer stores of the vector path and the
  staged taps (one address register), the global stores of the element-wise path (a register pair)."""
  checked = {'buffer': 0, 'global': 0}
  for name, body in kernels[0].items():
    per_kernel = 0
    for line in body.splitlines():
      m = re.search(r'global_store_\w+\s+v\[(\d+):(\d+)\], (?:v(\d+)|v\[(\d+):(\d+)\]), ', line)
      if m:
        alo, ahi = int(m.group(1)), int(m.group(2))
        lo = int(m.group(3) if m.group(3) is not None else m.group(4))
        hi = int(m.group(3) if m.group(3) is not None else m.group(5))
        checked['global'] += 1
        per_kernel += 1
        assert ahi < lo or alo > hi, '%s stores its own address registers: %s' % (name, line.strip())
      m = re.search(r'buffer_store_(?:dword(?:x(\d))?|short|byte)\s+(?:v(\d+)|v\[(\d+):(\d+)\]), v(\d+), s\[', line)
      if m:
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = int(m.group(2) if m.group(2) is not None else m.group(4))
        checked['buffer'] += 1
        per_kernel += 1
        assert not (lo <= int(m.group(5)) <= hi), '%s stores its own address register: %s' % (name, line.strip())
    assert not re.search(r'flat_store', body), name
    assert per_kernel >= 4, name  # every kernel stores, and the patterns still match what the compiler prints
  assert checked['buffer'] >= 96 * 4 and checked['global'] >= 96


def test_the_table_gather_is_a_global_load_and_nothing_is_pinned_by_hand(kernels):
  """what chain_fused_codes.hip compiles to: a 16-bit table is read with global loads (an 8-bit one from LDS), never
  through a flat load; the unit's own source holds no inline assembly"""
  for name, body in kernels[0].items():
    assert 'flat_load' not in body, name
    if 'ItLi' in name:  # <unsigned short, ...>: the 16-bit codes
      assert re.search(r'global_load_(?:ushort|short_d16|dword)', body), name
  src = open(os.path.join(CSRC, UNIT)).read()
  code = '\n'.join(l.split('//')[0] for l in src.splitlines())
  assert not re.search(r'\basm\b|__asm', code)
  assert sum('ItLi' in name for name in kernels[0]) == 48
