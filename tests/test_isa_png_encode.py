"""The static checks of tests/test_isa_curves_chain.py for csrc/png_encode.hip (CPU-only: cross-compiles with -S, runs
nothing): the unit is compiled with the default flags and linked, it has its four kernels, and none of them uses scratch
or spills a register."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
UNIT = 'png_encode.hip'
KERNELS = ('png_row_types_kernel', 'png_segment_kernel', 'png_scan_kernel', 'png_gather_kernel')


def build_line(unit=UNIT):
  sh = open(os.path.join(CSRC, 'build.sh')).read()
  line = [l for l in sh.splitlines() if '/%s"' % unit in l and l.lstrip().startswith('"$HIPCC"')]
  assert len(line) == 1, line
  return sh, line[0]


@pytest.fixture(scope='module')
def listing(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
    pytest.skip('hipcc not available')
  extra = [f for f in build_line()[1].split() if f.startswith('-f')]
  out = str(tmp_path_factory.mktemp('isa') / 'png_encode.s')
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only'] + extra +
                        [os.path.join(CSRC, UNIT), '-o', out], stderr=subprocess.DEVNULL)
  return open(out).read()


def test_build_script_compiles_the_unit_with_default_flags_and_links_it():
  sh, line = build_line()
  assert [f for f in line.split() if f.startswith('-f')] == [], line
  assert '"$TMP/png_encode.o"' in line and '"$TMP/png_encode.o"' in sh.split('-shared')[1]
  assert 'png_encode.hip, the twentieth' in sh
  waited = re.search(r'-c "\$HERE/png_encode\.hip".*?\n(p\d+)=\$!', sh, flags=re.S).group(1)
  assert re.search(r'^wait \$%s$' % waited, sh, flags=re.M)  # a failed compile stops the script


def test_four_kernels_without_scratch_or_spills(listing):
  meta = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', listing, flags=re.S)}
  assert len(meta) == len(KERNELS) and all(any(k in name for name in meta) for k in KERNELS), sorted(meta)
  for name, body in meta.items():
    scratch = re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body)
    assert scratch is not None and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
    text = re.search(r'^%s:[^\n]*\n(.*?)\n\s*s_endpgm' % re.escape(name), listing, flags=re.S | re.M)
    assert text is not None and 'scratch_' not in text.group(1), name
  notes = re.findall(r'- \.agpr_count:.*?\.wavefront_size:', listing, flags=re.S)
  assert len(notes) == len(KERNELS)
  for n in notes:
    name = re.search(r'\.name:\s+(\S+)', n).group(1)
    assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', n).group(1)) == 0, name
    assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', n).group(1)) == 0, name
    assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', n).group(1)) == 0, name
    assert int(re.search(r'\.vgpr_count:\s+(\d+)', n).group(1)) <= 128, name  # two blocks of 256 threads per SIMD set


def test_no_global_atomic_and_no_float_in_the_unit(listing):
  """the design's promises that the listing can show: the atomics are LDS ones (ds_*), and no float instruction"""
  for name in KERNELS:
    text = re.search(r'^(\S*%s\S*):[^\n]*\n(.*?)\n\s*s_endpgm' % name, listing, flags=re.S | re.M).group(2)
    assert not re.search(r'\b(global|flat|buffer)_atomic', text), name
    assert not re.search(r'\bv_(add|mul|fma|mac|sub)_f(16|32|64)\b', text), name
