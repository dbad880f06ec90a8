#!/usr/bin/env python3
"""Compare two `hipcc -S --cuda-device-only` listings of one translation unit symbol by symbol.

  python tools/listing_symbols.py before.s after.s

A change that touches host code only may still make the compiler emit a unit's kernels in another order (the order in
which the host code first names them).  Then the two files differ as text, while every kernel is the same.  This tool
cuts each listing into one piece per kernel -- its body, its .amdhsa_kernel block and resource comments, and its entry
in the metadata -- keyed by the symbol, drops what only counts the kernels (the N of .LBB<N>_ / .Lfunc_end<N>, in labels
and in comments) and the per-compilation __hip_cuid_* lines, and compares the pieces.  It prints what differs and exits
1, or one line and 0.
"""
import re
import sys

START = re.compile(r'^\t\.section\t\.text\.([^,\s]+),')
COUNTERS = re.compile(r'(\.L(?:BB|func_begin|func_end|tmp)|\bBB)\d+(?=_|\b)')
PAD = re.compile(r'\s+;')  # a label's comment is padded to a column: the label's length moves it


def pieces(path):
  lines = [l for l in open(path).read().split('\n') if '__hip_cuid_' not in l]
  meta = lines.index('\t.amdgpu_metadata')
  out, key, order = {'': []}, '', []
  for i, line in enumerate(lines[:meta]):
    m = START.match(line)
    # a kernel's piece opens at its section line followed by its .globl / .protected (the same section is re-entered
    # after the .amdhsa_kernel block: that line stays inside the piece)
    if m and re.match(r'^\t\.(globl|protected|weak)\t' + re.escape(m.group(1)) + r'\b', lines[i + 1]):
      key = m.group(1)
      order.append(key)
      assert key not in out, key
      out[key] = []
    out[key].append(PAD.sub(' ;', COUNTERS.sub(lambda c: c.group(1), line)))
  entry = None
  for line in lines[meta:]:
    if line.startswith('  - .'):  # a new entry of amdhsa.kernels
      entry = []
      out.setdefault(('meta', len(out)), entry)
    elif not line.startswith('    '):
      entry = None
    if entry is None:
      out[''].append(line)
    else:
      entry.append(line)
      if line.startswith('    .name:'):
        out[('meta', line.split()[1])] = entry
  named = {k: v for k, v in out.items() if not (isinstance(k, tuple) and isinstance(k[1], int))}
  assert sum(1 for k in named if isinstance(k, tuple)) == len(order), 'every kernel has one metadata entry'
  return named, order


def main(a, b):
  pa, oa = pieces(a)
  pb, ob = pieces(b)
  bad = sorted(str(k) for k in set(pa) ^ set(pb)) + sorted(str(k) for k in set(pa) & set(pb) if pa[k] != pb[k])
  for k in bad:
    print('differs:', k or '(outside the kernels)')
  if bad:
    return 1
  print('%d kernels, each identical (body, .amdhsa_kernel block, metadata entry); order %s' %
        (len(oa), 'unchanged' if oa == ob else 'changed'))
  return 0


if __name__ == '__main__':
  sys.exit(main(sys.argv[1], sys.argv[2]))
