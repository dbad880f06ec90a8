"""A NumPy restatement of the file expo_png_encode_ragged writes (include/exposure_hip.h), written from
the format alone: the PNG row filters and libpng's heuristic, an optimal Huffman code by a heap (with the length limit
f = (f + 1) // 2 when it is deeper than 15 bits), the rule dynamic against stored, the chunk layout.  And a parser that
splits a file into chunks and checks every CRC-32 against zlib's.  The GPU tests compare the device's files with it
through independent decoders (zlib, PIL); an optimal code's cost is unique, so the file LENGTHS must agree exactly
whatever the tie-breaking, the bytes need not."""
import heapq
import struct
import zlib

import numpy as np

SEG = 16384  # expo_png_segment_bytes() of the library as it stands; the callers pass the library's own value
SIGNATURE = b'\x89PNG\r\n\x1a\n'
HEADER_BITS = 3 + 14 + 19 * 3 + 258 * 4
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FILTERS = ('none', 'sub', 'up', 'average', 'paeth', 'adaptive')


def stream_bytes(h, w):
  return h * (1 + 3 * w)


def bound(h, w, seg=SEG):
  s = stream_bytes(h, w)
  return 75 + 17 * (-(-s // seg)) + s


def filtered_stream(pic, filt):
  """Row r: its type byte, then its 3 W filtered bytes (bpp = 3).  filt 0..4: that type for every row; 5: per row the
  type with the smallest sum of min(b, 256 - b), ties to the lowest.  -> (uint8 stream, the row types)"""
  pic = np.asarray(pic)
  assert pic.dtype == np.uint8 and pic.ndim == 3 and pic.shape[2] == 3
  h, w, _ = pic.shape
  x = pic.reshape(h, 3 * w).astype(np.int32)
  a = np.zeros_like(x)
  a[:, 3:] = x[:, :-3]
  b = np.zeros_like(x)
  b[1:] = x[:-1]
  c = np.zeros_like(x)
  c[1:, 3:] = x[:-1, :-3]
  p = a + b - c
  pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
  paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
  every = np.stack([(x - pred) & 255 for pred in (np.zeros_like(x), a, b, (a + b) >> 1, paeth)])  # (5, h, 3w)
  if filt == 5:
    types = np.minimum(every, 256 - every).sum(axis=2, dtype=np.int64).argmin(axis=0)  # the first of equal sums
  else:
    assert 0 <= filt <= 4
    types = np.full((h,), filt, dtype=np.int64)
  rows = every[types, np.arange(h)]
  return np.concatenate([types[:, None], rows], axis=1).astype(np.uint8).ravel(), types


def unfilter(stream, h, w):
  """the picture of a filtered stream, by the PNG specification's reconstruction (plain integers, row by row)"""
  n = 3 * w
  raw = bytes(stream)
  assert len(raw) == h * (1 + n)
  out = np.zeros((h, n), dtype=np.uint8)
  prev = bytearray(n)
  for r in range(h):
    t, line = raw[r * (1 + n)], bytearray(raw[r * (1 + n) + 1:(r + 1) * (1 + n)])
    if t == 1:
      for i in range(3, n):
        line[i] = (line[i] + line[i - 3]) & 255
    elif t == 2:
      for i in range(n):
        line[i] = (line[i] + prev[i]) & 255
    elif t == 3:
      for i in range(n):
        line[i] = (line[i] + (((line[i - 3] if i >= 3 else 0) + prev[i]) >> 1)) & 255
    elif t == 4:
      for i in range(n):
        a, b, c = (line[i - 3] if i >= 3 else 0), prev[i], (prev[i - 3] if i >= 3 else 0)
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        line[i] = (line[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
    else:
      assert t == 0, t
    out[r] = np.frombuffer(bytes(line), dtype=np.uint8)
    prev = line
  return out.reshape(h, w, 3)


def huffman_lengths(freq):
  """Code lengths of an optimal prefix code of the symbols with freq > 0 (at least two), by a heap -> (lengths, depth)"""
  freq = [int(f) for f in freq]
  live = [s for s, f in enumerate(freq) if f > 0]
  assert len(live) >= 2
  heap = [(freq[s], s, (s,)) for s in live]  # (weight, tie-break, the leaves below)
  heapq.heapify(heap)
  lengths = [0] * len(freq)
  tick = len(freq)
  while len(heap) > 1:
    w1, _, l1 = heapq.heappop(heap)
    w2, _, l2 = heapq.heappop(heap)
    for s in l1 + l2:
      lengths[s] += 1
    heapq.heappush(heap, (w1 + w2, tick, l1 + l2))
    tick += 1
  return lengths, max(lengths)


def limited_lengths(freq):
  """-> (lengths of at most 15 bits, the depth of the optimal code before any limit)"""
  lengths, depth = huffman_lengths(freq)
  unlimited = depth
  f = [int(v) for v in freq]
  while depth > 15:
    f = [(v + 1) // 2 for v in f]
    lengths, depth = huffman_lengths(f)
  return lengths, unlimited


def canonical_codes(lengths):
  """RFC 1951 §3.2.2"""
  count = [0] * 16
  for l in lengths:
    count[l] += 1
  count[0] = 0
  code, nxt = 0, [0] * 16
  for bits in range(1, 16):
    code = (code + count[bits - 1]) << 1
    nxt[bits] = code
  codes = [0] * len(lengths)
  for s, l in enumerate(lengths):
    if l:
      codes[s] = nxt[l]
      nxt[l] += 1
  return codes


def _reverse(v, n):
  return int(format(v, '0%db' % n)[::-1], 2) if n else 0


def segment_plan(seg, final):
  """-> (stored?, data bytes, lengths, depth before the limit) of one segment"""
  freq = np.bincount(seg, minlength=257)
  freq[256] = 1  # end-of-block, once
  lengths, unlimited = limited_lengths(freq)
  bits = HEADER_BITS + int((freq * np.asarray(lengths)).sum())
  dyn = (bits + 7) // 8 if final else (bits + 3 + 7) // 8 + 4
  sto = 5 + len(seg)
  return dyn >= sto, (sto if dyn >= sto else dyn), lengths, unlimited


def deflate_segment(seg, final):
  """One segment's deflate bytes: a dynamic block of literals (and zlib's sync flush unless final), or a stored block"""
  seg = np.asarray(seg, dtype=np.uint8)
  stored, size, lengths, _ = segment_plan(seg, final)
  if stored:
    n = len(seg)
    return bytes([1 if final else 0]) + struct.pack('<HH', n, n ^ 0xFFFF) + seg.tobytes()
  bits = np.zeros((size * 8,), dtype=np.uint8)
  at = 0

  def put(value, n):  # least significant bit first
    nonlocal at
    for k in range(n):
      bits[at + k] = (value >> k) & 1
    at += n

  put(1 if final else 0, 1)
  put(2, 2)  # BTYPE 10
  put(0, 5)  # HLIT: 257 codes
  put(0, 5)  # HDIST: 1 code
  put(15, 4)  # HCLEN: 19 lengths
  for sym in CL_ORDER:
    put(4 if sym <= 15 else 0, 3)
  for l in list(lengths) + [1]:  # the 257 literal lengths and the distance code's, each as its own 4-bit code
    put(_reverse(l, 4), 4)
  assert at == HEADER_BITS
  codes = canonical_codes(lengths)
  rev = np.array([_reverse(c, l) for c, l in zip(codes, lengths)], dtype=np.int64)
  ls = np.asarray(lengths, dtype=np.int64)
  l_of, c_of = ls[seg], rev[seg]
  pos = at + np.concatenate([[0], np.cumsum(l_of)[:-1]])
  for k in range(15):
    m = l_of > k
    bits[pos[m] + k] = (c_of[m] >> k) & 1
  at += int(l_of.sum())
  put(int(rev[256]), lengths[256])
  if not final:
    put(0, 3)  # an empty stored block
    at = (at + 7) // 8 * 8
    put(0xFFFF0000, 32)
  assert (at + 7) // 8 == size, (at, size)
  return np.packbits(bits, bitorder='little').tobytes()


def chunk(kind, data):
  return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def encode(pic, filt=5, seg=SEG):
  """The whole file"""
  h, w, _ = pic.shape
  stream, _ = filtered_stream(pic, filt)
  parts = [SIGNATURE, chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)), chunk(b'IDAT', b'\x78\x01')]
  n = -(-len(stream) // seg)
  for k in range(n):
    parts.append(chunk(b'IDAT', deflate_segment(stream[k * seg:(k + 1) * seg], k == n - 1)))
  parts.append(chunk(b'IDAT', struct.pack('>I', zlib.adler32(stream.tobytes()))))
  parts.append(chunk(b'IEND', b''))
  return b''.join(parts)


def file_plan(pic, filt=5, seg=SEG):
  """-> (the file's length, per segment stored?, the deepest optimal code before any limit, the filtered stream)
  without packing a bit"""
  stream, _ = filtered_stream(pic, filt)
  n = -(-len(stream) // seg)
  total, stored, depth = 75, [], 0
  for k in range(n):
    st, size, _, d = segment_plan(stream[k * seg:(k + 1) * seg], k == n - 1)
    total += 12 + size
    stored.append(st)
    depth = max(depth, d)
  return total, stored, depth, stream


def parse(data):
  """-> [(type, payload)] of a PNG file; asserts the signature, every chunk's CRC-32 (zlib's) and that nothing follows"""
  assert data[:8] == SIGNATURE
  at, chunks = 8, []
  while at < len(data):
    n, kind = struct.unpack('>I4s', data[at:at + 8])
    payload = data[at + 8:at + 8 + n]
    assert len(payload) == n
    (crc,) = struct.unpack('>I', data[at + 8 + n:at + 12 + n])
    assert crc == zlib.crc32(kind + payload), (kind, at)
    chunks.append((kind, payload))
    at += 12 + n
  assert at == len(data)
  return chunks


def idat_payloads(data):
  return [p for kind, p in parse(data) if kind == b'IDAT']


def check_structure(data, h, w, seg=SEG):
  """the chunk order and the fixed chunks of the format -> the concatenated IDAT payloads (a zlib stream)"""
  chunks = parse(data)
  nseg = -(-stream_bytes(h, w) // seg)
  assert [k for k, _ in chunks] == [b'IHDR'] + [b'IDAT'] * (nseg + 2) + [b'IEND']
  assert chunks[0][1] == struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)
  assert chunks[1][1] == b'\x78\x01' and len(chunks[-2][1]) == 4 and chunks[-1][1] == b''
  return b''.join(p for _, p in chunks[1:-1])


def deep_picture():
  """The 1 x 1925 picture whose filter-None stream (5776 bytes) holds the byte values 16, 15, .., 0 with the counts
  1, 1, 3, 4, 7, 11, ..., 1364, 2207 (the type byte is one of the zeros): with end-of-block counted once the optimal
  code is 17 bits deep, so the length limit must act."""
  counts = [1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2207]
  values = np.concatenate([np.full((c - (1 if v == 0 else 0),), v, dtype=np.uint8)
                           for v, c in zip(range(16, -1, -1), counts)])
  assert values.size == 1925 * 3
  pic = values.reshape(1, 1925, 3)
  _, _, depth, _ = file_plan(pic, 0)
  assert depth > 15, depth  # the case cannot go stale
  return pic


def contents(h, w, seed):
  """the four pictures of a shape: seeded noise, zeros, 255s, a smooth gradient with noise of amplitude 2"""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  smooth = ((yy + 2 * xx)[:, :, None] // 4 + np.arange(3) * 40 + rng.integers(-2, 3, (h, w, 3))) % 256
  return {'noise': rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'zeros': np.zeros((h, w, 3), np.uint8),
          'ones': np.full((h, w, 3), 255, np.uint8), 'smooth': smooth.astype(np.uint8)}
