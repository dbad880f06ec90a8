"""The static checks of tests/test_isa_jpeg_decode.py for csrc/jpeg_decode_sync.hip (CPU-only: cross-compiles with -S,
runs nothing): the unit is compiled with the default flags, linked and waited for, and its four kernels have exactly
the resources of the table in DESIGN.md §3.36 -- VGPRs, LDS bytes per block, no scratch, no spills, wave 64."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'exposure_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
UNIT = 'jpeg_decode_sync.hip'
# kernel (a part of its mangled name) -> (VGPRs, LDS bytes per block); scratch is zero for all
TABLE = {
    'jpeg_sync_settle_kernel': (52, 2304),
    'jpeg_sync_scan_kernel': (34, 8208),
    'jpeg_sync_emit_kernel': (42, 0),
    'jpeg_sync_serial_kernel': (70, 9216),
}


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
  out = str(tmp_path_factory.mktemp('isa') / 'jpeg_decode_sync.s')
  subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only'] + extra +
                        [os.path.join(CSRC, UNIT), '-o', out], stderr=subprocess.DEVNULL)
  return open(out).read()


def test_build_script_compiles_the_unit_with_default_flags_and_links_it():
  sh, line = build_line()
  assert [f for f in line.split() if f.startswith('-f')] == [], line
  assert '"$TMP/jpeg_decode_sync.o"' in line and '"$TMP/jpeg_decode_sync.o"' in sh.split('-shared')[1]
  assert ', and jpeg_decode_sync.hip, the twenty-fifth' in sh
  waited = re.search(r'-c "\$HERE/jpeg_decode_sync\.hip".*?\n(p\d+)=\$!', sh, flags=re.S).group(1)
  assert waited == 'p25' and re.search(r'^wait \$%s$' % waited, sh, flags=re.M)  # a failed compile stops the script
  # the digest behind the binary covers every .hip and .h of the directory, so also the new unit and its header
  assert 'ls *.hip *.h build.sh' in sh and os.path.exists(os.path.join(CSRC, 'jpeg_decode_sync.h'))
  # the serial decoder's header is read, not edited: the walk is built from its reader and its symbol rules
  assert '#include "jpeg_decode.h"' in open(os.path.join(CSRC, 'jpeg_decode_sync.h')).read()


def test_resource_table_of_the_design_document(listing):
  notes = re.findall(r'- \.agpr_count:.*?\.wavefront_size:\s+\d+', listing, flags=re.S)
  assert len(notes) == len(TABLE)
  got = {}
  for n in notes:
    name = re.search(r'\.name:\s+(\S+)', n).group(1)
    key = [k for k in TABLE if k in name]
    assert len(key) == 1, name
    assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', n).group(1)) == 0, name
    assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', n).group(1)) == 0, name
    assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', n).group(1)) == 0, name
    assert int(re.search(r'\.wavefront_size:\s+(\d+)', n).group(1)) == 64, name
    got[key[0]] = (int(re.search(r'\.vgpr_count:\s+(\d+)', n).group(1)),
                   int(re.search(r'\.group_segment_fixed_size:\s+(\d+)', n).group(1)))
  assert got == TABLE
  doc = open(os.path.join(ROOT, 'DESIGN.md')).read()
  section = doc[doc.index('### 3.36'):]
  for key, (vgprs, lds) in TABLE.items():
    assert re.search(r'\| *`%s` *\| *\d+ *\| *%d *\| *%s *\| *0 *\|' % (key, vgprs, '{:,}'.format(lds).replace(',', ' ')), section), (key, vgprs, lds)
