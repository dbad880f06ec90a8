"""CPU: the host-side launch scaffold of the six fused ragged inference passes (csrc/ragged_launch.h).
tools/ragged_rehearse.cpp -- a stand-alone host program built with AddressSanitizer and UBSan, no GPU, no HIP call --
runs ragged_launches with the units' own tables and fills and prints what every launch would have been handed.  The
expectation below restates the rule from its description (chain_fused.hip's "ragged" comment):

  * a call is cut into launches of 64 images, in order; a launch's rows of ids / params start `base` images in;
  * image j of a launch owns ceil(ceil(hw / PPL) / 256) blocks (PPL 8 pixels per lane in fp16, 4 in fp32), laid end
    to end: first[j] is its first block, first[n] the 1-D grid;
  * it takes the vector path when hw is a whole number of 12-byte vectors (2 pixels in fp16, 1 in fp32) and its input,
    its output (if any) and -- for storage taps, and u16 taps of fp16 -- its tap plane are 4-byte aligned;
  * the launch is the ANY_SLOW kind when some image of it is not on the vector path;
  * the cache policy is the whole call's: streaming when its pixels hold at least EXPO_STREAM_MIN_BYTES in the storage
    dtype.
"""
import os
import shutil
import subprocess

import pytest

from tests._policy_matrix_cases import TAP_NONE, TAP_STORAGE, TAP_U8, TAP_U16, ragged_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, TAPS = 0x10000, 0x20000, 0x30000  # aligned bases; an image's addresses are spaced out from them


def test_tap_format_values_are_the_header_s():
  header = open(os.path.join(ROOT, 'include', 'exposure_hip.h')).read()
  for name, value in (('EXPO_TAP_STORAGE', TAP_STORAGE), ('EXPO_TAP_U8', TAP_U8), ('EXPO_TAP_U16', TAP_U16)):
    assert ('#define %s %d' % (name, value)) in ' '.join(header.split()), name


@pytest.fixture(scope='module')
def rehearse(tmp_path_factory):
  hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
  if not os.path.exists(hipcc):
    pytest.skip('no hipcc')
  exe = str(tmp_path_factory.mktemp('ragged') / 'ragged_rehearse')
  subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host',
                         '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                         os.path.join(ROOT, 'tools', 'ragged_rehearse.cpp'), '-o', exe], stderr=subprocess.DEVNULL)

  def run(table, dtype, fmt, images, ys=True, stream_min_bytes=None):
    env = {k: v for k, v in os.environ.items() if k != 'EXPO_STREAM_MIN_BYTES'}
    if stream_min_bytes is not None:
      env['EXPO_STREAM_MIN_BYTES'] = str(stream_min_bytes)
    text = ''.join('%d %d %x %x %x\n' % im for im in images)
    p = subprocess.run([exe, table, dtype, str(fmt), str(int(ys))], input=text.encode(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode()

  return run


def expected(table, dtype, fmt, images, ys=True, stream_min_bytes=8 << 20):
  """the rehearsal's text for the launches of the restated rule (tests/_policy_matrix_cases.py::ragged_plan, which
  tests/test_hip_policy_matrix.py's ledger is computed from)"""
  out = []
  for launch in ragged_plan(dtype, fmt, images, ys, stream_min_bytes):
    first = launch['first']
    out.append('launch stream=%d any_slow=%d grid=%d,1,1 base=%d n=%d first=%s vec=0x%x' %
               (launch['stream'], launch['any_slow'], first[-1], launch['base'], launch['n'],
                ','.join(map(str, first)), launch['vec']))
    for j, x, y, h, w, taps in launch['slots']:
      size_text = 'h=%d w=%d' % (h, w) if table == 'masked' else 'hw=%d' % (h * w)
      out.append('  slot %d %s=0x%x y=0x%x %s%s' % (j, 'codes' if table == 'codes' else 'x', x, y, size_text,
                                                   '' if table == 'ragged' else ' taps=0x%x' % taps))
  return '\n'.join(out) + '\n'


def image(i, h, w, dx=0, dy=0, dt=0):
  return (h, w, X + 0x100 * i + dx, Y + 0x100 * i + dy, TAPS + 0x100 * i + dt)


def check(rehearse, table, dtype, fmt, images, **kw):
  got = rehearse(table, dtype, fmt, images, **kw)
  want = expected(table, dtype, fmt, images, **{k: v for k, v in kw.items() if v is not None})
  assert got == want, (table, dtype, fmt, kw)
  return got


@pytest.mark.parametrize('n', [1, 64, 65, 130])
def test_split_into_launches_of_64(rehearse, n):
  # sizes of a few pixels, two of them with more than one block (fp16: 2048 pixels a block)
  images = [image(i, 1 + i % 5, 2 + i % 7) for i in range(n)]
  images[0] = image(0, 41, 50)                    # 2050 pixels: two blocks
  images[n - 1] = image(n - 1, 3, 1367)           # 4101 pixels: three blocks, the call's last image
  got = check(rehearse, 'taps', 'f16', TAP_U8, images)
  launches = [l for l in got.split('\n') if l.startswith('launch')]
  assert len(launches) == -(-n // 64)
  for k, l in enumerate(launches):  # every launch restarts its block count and carries its place in the call
    assert (' base=%d ' % (64 * k)) in l and ' first=0,' in l and (' n=%d ' % min(64, n - 64 * k)) in l


@pytest.mark.parametrize('table, fmt', [('ragged', TAP_NONE), ('taps', TAP_STORAGE), ('masked', TAP_U16),
                                        ('masked', TAP_NONE), ('codes', TAP_U8), ('codes', TAP_NONE)])
@pytest.mark.parametrize('dtype', ['f16', 'f32'])
def test_each_table_type(rehearse, table, fmt, dtype):
  images = [image(0, 4, 6), image(1, 3, 5), image(2, 2, 2, dx=2), image(3, 33, 63)]
  check(rehearse, table, dtype, fmt, images)
  if fmt != TAP_NONE:
    check(rehearse, table, dtype, fmt, images, ys=False)


def test_odd_pixel_count_is_element_wise_in_fp16_only(rehearse):
  images = [image(0, 3, 5)]
  assert ' any_slow=1 ' in check(rehearse, 'ragged', 'f16', TAP_NONE, images)
  got = check(rehearse, 'ragged', 'f32', TAP_NONE, images)
  assert ' any_slow=0 ' in got and ' vec=0x1\n' in got


@pytest.mark.parametrize('dtype', ['f16', 'f32'])
@pytest.mark.parametrize('fmt', [TAP_STORAGE, TAP_U8, TAP_U16])
def test_each_address_misaligned_in_turn(rehearse, dtype, fmt):
  tap_counts = fmt == TAP_STORAGE or (fmt == TAP_U16 and dtype == 'f16')
  for table in ('taps', 'masked', 'codes'):
    for which, slow in (('dx', True), ('dy', True), ('dt', tap_counts)):
      images = [image(0, 4, 6), image(1, 4, 6, **{which: 2}), image(2, 2, 8)]
      got = check(rehearse, table, dtype, fmt, images)
      assert (' vec=0x5\n' if slow else ' vec=0x7\n') in got, (table, which)
      if which == 'dy':  # without ys the output's address is out of the test
        assert ' vec=0x7\n' in check(rehearse, table, dtype, fmt, images, ys=False)


def test_launches_all_vector_all_slow_and_mixed(rehearse):
  fast, slow = (lambda i: image(i, 4, 6)), (lambda i: image(i, 3, 5))
  for kinds, any_slow, vec in (((fast, fast, fast), 0, 7), ((slow, slow, slow), 1, 0), ((fast, slow, fast), 1, 5)):
    got = check(rehearse, 'taps', 'f16', TAP_U8, [k(i) for i, k in enumerate(kinds)])
    assert (' any_slow=%d ' % any_slow) in got and (' vec=0x%x\n' % vec) in got
  # the kind is a launch's own: 64 vector images, then a launch with an element-wise one
  got = check(rehearse, 'ragged', 'f16', TAP_NONE, [fast(i) for i in range(64)] + [slow(64), fast(65)])
  first, second = [l for l in got.split('\n') if l.startswith('launch')]
  assert ' any_slow=0 ' in first and ' vec=0xffffffffffffffff' in first
  assert ' any_slow=1 ' in second and ' vec=0x2' in second


@pytest.mark.parametrize('dtype, nbytes', [('f16', 2 * 3 * (24 + 15)), ('f32', 4 * 3 * (24 + 15))])
def test_cache_policy_at_the_threshold(rehearse, dtype, nbytes):
  images = [image(0, 4, 6), image(1, 3, 5)]
  for table, fmt in (('ragged', TAP_NONE), ('codes', TAP_U16)):
    assert ' stream=1 ' in check(rehearse, table, dtype, fmt, images, stream_min_bytes=nbytes)
    assert ' stream=0 ' in check(rehearse, table, dtype, fmt, images, stream_min_bytes=nbytes + 1)
    assert ' stream=0 ' in check(rehearse, table, dtype, fmt, images)  # the default threshold is far away
