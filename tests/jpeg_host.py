"""A NumPy restatement of the device's baseline JPEG file, written from the format's text, not from
the HIP code: ``encode`` makes the file of a picture byte for byte, with the restart interval ``ri`` as a parameter;
``parse`` takes a file apart into its header fields and per-interval payloads, and ``decode_coefficients`` runs its own
Huffman decoder over them.  Integer arithmetic only (int64 arrays; the format promises that nothing leaves int32, which
``encode`` asserts)."""
import functools
import io

import numpy as np

HEADER_BYTES = 629
SUBSAMPLINGS = (0, 2)  # 4:4:4, 4:2:0 (PIL's numbers)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 Annex K.1 and K.2, natural order
QUANT_BASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
     80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
     95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
     99, 99] + [99] * 32])

# T.81 Annex K.3 - K.6: (BITS, HUFFVAL); luma then chroma
DC_TABLES = [([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
             ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))]
AC_TABLES = [
    ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
     [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
      0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
      0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
      0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
      0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
      0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
      0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
      0xf9, 0xfa]),
    ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
     [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
      0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
      0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
      0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
      0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
      0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
      0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
      0xf9, 0xfa])]


def cosine_table():
  """C[u][x] = rint(2^13 k_u cos((2x + 1) u pi / 16)) in float64, as integers"""
  u, x = np.mgrid[0:8, 0:8]
  k = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5)
  return np.rint(8192.0 * k * np.cos((2 * x + 1) * u * np.pi / 16.0)).astype(np.int64)


COS = cosine_table()


def canonical_codes(bits, vals):
  """T.81 Annex C: symbol -> (code, length)"""
  out, code, k = {}, 0, 0
  for length in range(1, 17):
    for _ in range(bits[length - 1]):
      out[vals[k]] = (code, length)
      code += 1
      k += 1
    code <<= 1
  return out


DC_CODES = [canonical_codes(*t) for t in DC_TABLES]
AC_CODES = [canonical_codes(*t) for t in AC_TABLES]


def quant_table(table, quality):
  """the 64 values of table 0 (luma) / 1 (chroma) at quality 1..100, natural order"""
  scale = 5000 // quality if quality < 50 else 200 - 2 * quality
  return np.clip((QUANT_BASE[table] * scale + 50) // 100, 1, 255)


def dht_segments():
  """the four DHT segments in the file's order: DC0, AC0, DC1, AC1"""
  out = []
  for t in range(2):
    for cls, (bits, vals) in ((0, DC_TABLES[t]), (1, AC_TABLES[t])):
      body = bytes([cls << 4 | t]) + bytes(bits) + bytes(vals)
      out.append(b'\xff\xc4' + (len(body) + 2).to_bytes(2, 'big') + body)
  return out


def header(h, w, quality, subsampling, ri):
  out = b'\xff\xd8' + b'\xff\xe0' + (16).to_bytes(2, 'big') + b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])
  for t in range(2):
    out += b'\xff\xdb' + (67).to_bytes(2, 'big') + bytes([t]) + bytes(quant_table(t, quality)[ZIGZAG].tolist())
  out += b'\xff\xc0' + (17).to_bytes(2, 'big') + bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3])
  out += bytes([1, 0x11 if subsampling == 0 else 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
  out += b''.join(dht_segments())
  out += b'\xff\xdd' + (4).to_bytes(2, 'big') + ri.to_bytes(2, 'big')
  out += b'\xff\xda' + (12).to_bytes(2, 'big') + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
  assert len(out) == HEADER_BYTES
  return out


def planes(pic, subsampling):
  """the level-shifted component planes over whole MCUs: Y (H, W), Cb and Cr (H, W) or (H / 2, W / 2)"""
  h, w, _ = pic.shape
  side = 8 if subsampling == 0 else 16
  hh, ww = -(-h // side) * side, -(-w // side) * side
  ext = pic[np.minimum(np.arange(hh), h - 1)][:, np.minimum(np.arange(ww), w - 1)].astype(np.int64)
  r, g, b = ext[..., 0], ext[..., 1], ext[..., 2]
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
  if subsampling == 2:
    cb = (cb[0::2, 0::2] + cb[0::2, 1::2] + cb[1::2, 0::2] + cb[1::2, 1::2] + 2) >> 2
    cr = (cr[0::2, 0::2] + cr[0::2, 1::2] + cr[1::2, 0::2] + cr[1::2, 1::2] + 2) >> 2
  return y - 128, cb - 128, cr - 128


def transform_quantise(plane, q):
  """(H, W) level-shifted samples -> (H / 8, W / 8, 8, 8) quantised coefficients [v][u]; q: 64 values, natural order"""
  hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
  s = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3)  # [by][bx][y][x]
  acc = np.einsum('ux,abyx->abyu', COS, s)
  assert np.abs(acc).max() <= 128 * 32136
  t = (acc + 1024) >> 11
  f = np.einsum('vy,abyu->abvu', COS, t)
  assert np.abs(f).max() < 2 ** 27
  qq = q.reshape(8, 8)
  mag = (np.abs(f) + (qq << 14)) // (qq << 15)
  return np.sign(f) * mag


def mcu_blocks(pic, quality, subsampling):
  """-> (nmcu, blocks per MCU, 64) quantised coefficients in natural order, MCUs in raster order, the blocks of an MCU
  in the order of the scan, and per block of an MCU its component (0 Y, 1 Cb, 2 Cr)"""
  y, cb, cr = planes(pic, subsampling)
  qy, qc = quant_table(0, quality), quant_table(1, quality)
  by, bb, br = transform_quantise(y, qy), transform_quantise(cb, qc), transform_quantise(cr, qc)
  my, mx = bb.shape[:2] if subsampling == 2 else by.shape[:2]
  if subsampling == 0:
    blocks = np.stack([by, bb, br], axis=2)  # [my][mx][3][8][8]
    comps = [0, 1, 2]
  else:
    yq = by.reshape(my, 2, mx, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my, mx, 4, 8, 8)  # Y00 Y01 Y10 Y11
    blocks = np.concatenate([yq, bb[:, :, None], br[:, :, None]], axis=2)
    comps = [0, 0, 0, 0, 1, 2]
  return blocks.reshape(my * mx, len(comps), 64), comps


def category(v):
  return int(abs(int(v))).bit_length()


def block_symbols(zz, pred, table):
  """one block's symbols: [(kind, symbol, value, size)], kind 'dc' / 'ac'; zz the 64 coefficients in zigzag order"""
  diff = int(zz[0]) - pred
  out = [('dc', category(diff), diff, category(diff))]
  run = 0
  for k in range(1, 64):
    v = int(zz[k])
    if v == 0:
      run += 1
      continue
    while run >= 16:
      out.append(('ac', 0xF0, 0, 0))
      run -= 16
    n = category(v)
    out.append(('ac', run << 4 | n, v, n))
    run = 0
  if run:
    out.append(('ac', 0x00, 0, 0))
  return out


class BitWriter:
  def __init__(self):
    self.acc, self.n = 0, 0

  def put(self, v, n):
    self.acc = (self.acc << n) | v
    self.n += n

  def finish(self):
    """-> the bytes, padded with 1-bits, and the number of padding bits"""
    pad = -self.n % 8
    self.put((1 << pad) - 1, pad)
    return self.acc.to_bytes(self.n // 8, 'big'), pad


def encode_full(pic, quality, subsampling, ri):
  """-> dict(file, intervals (unstuffed payloads), paddings, symbols (per interval, per block), blocks, comps)"""
  pic = np.asarray(pic)
  assert pic.dtype == np.uint8 and pic.ndim == 3 and pic.shape[2] == 3 and 1 <= quality <= 100 and subsampling in SUBSAMPLINGS
  h, w, _ = pic.shape
  blocks, comps = mcu_blocks(pic, quality, subsampling)
  nmcu = blocks.shape[0]
  zz = blocks[:, :, ZIGZAG]
  out = [header(h, w, quality, subsampling, ri)]
  intervals, paddings, symbols = [], [], []
  nint = -(-nmcu // ri)
  for k in range(nint):
    bw = BitWriter()
    pred = [0, 0, 0]
    syms = []
    for m in range(k * ri, min(nmcu, (k + 1) * ri)):
      for j, c in enumerate(comps):
        table = 0 if c == 0 else 1
        s = block_symbols(zz[m, j], pred[c], table)
        pred[c] = int(zz[m, j, 0])
        syms.append(s)
        for kind, sym, v, n in s:
          code, length = (DC_CODES if kind == 'dc' else AC_CODES)[table][sym]
          bw.put(code, length)
          if n:
            bw.put(v if v >= 0 else v + (1 << n) - 1, n)
    data, pad = bw.finish()
    intervals.append(data)
    paddings.append(pad)
    symbols.append(syms)
    out.append(data.replace(b'\xff', b'\xff\x00'))
    out.append(b'\xff\xd9' if k == nint - 1 else bytes([0xFF, 0xD0 + k % 8]))
  return dict(file=b''.join(out), intervals=intervals, paddings=paddings, symbols=symbols, blocks=blocks, comps=comps)


def encode(pic, quality, subsampling, ri):
  return encode_full(pic, quality, subsampling, ri)['file']


def parse(data):
  """a file -> dict(segments [(marker, body)], h, w, sampling (the Y component's byte), ri, dqt {id: 64 zigzag values},
  intervals: the unstuffed payloads, markers: the marker byte behind each)"""
  assert data[:2] == b'\xff\xd8'
  at, segments, out = 2, [], dict(dqt={})
  while True:
    assert data[at] == 0xFF
    marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], 'big')
    body = data[at + 4:at + 2 + length]
    segments.append((marker, body))
    at += 2 + length
    if marker == 0xDB:
      out['dqt'][body[0]] = list(body[1:65])
    elif marker == 0xC0:
      out['h'], out['w'], out['sampling'] = int.from_bytes(body[1:3], 'big'), int.from_bytes(body[3:5], 'big'), body[7]
    elif marker == 0xDD:
      out['ri'] = int.from_bytes(body, 'big')
    elif marker == 0xDA:
      break
  out['segments'], out['header_bytes'] = segments, at
  intervals, markers, cur = [], [], bytearray()
  while True:
    b = data[at]
    if b != 0xFF:
      cur.append(b)
      at += 1
    elif data[at + 1] == 0:
      cur.append(0xFF)
      at += 2
    else:
      intervals.append(bytes(cur))
      markers.append(data[at + 1])
      cur = bytearray()
      at += 2
      if markers[-1] == 0xD9:
        break
  assert at == len(data)
  out['intervals'], out['markers'] = intervals, markers
  return out


def decode_coefficients(parsed, nmcu, subsampling):
  """its own Huffman decoder over the parsed intervals -> (nmcu, blocks per MCU, 64) coefficients, natural order"""
  comps = [0, 1, 2] if subsampling == 0 else [0, 0, 0, 0, 1, 2]
  ri = parsed['ri']
  lookup = [[{(length, code): sym for sym, (code, length) in t.items()} for t in (DC_CODES[i], AC_CODES[i])] for i in range(2)]
  out = np.zeros((nmcu, len(comps), 64), np.int64)
  for k, payload in enumerate(parsed['intervals']):
    bits = int.from_bytes(payload, 'big')
    left = 8 * len(payload)

    def take(n):
      nonlocal left
      left -= n
      assert left >= 0
      return (bits >> left) & ((1 << n) - 1)

    def symbol(table):
      code = 0
      for length in range(1, 17):
        code = code << 1 | take(1)
        if (length, code) in table:
          return table[(length, code)]
      raise AssertionError('no code')

    def value(n):
      v = take(n) if n else 0
      return v if n == 0 or v >> (n - 1) else v - (1 << n) + 1

    pred = [0, 0, 0]
    for m in range(k * ri, min(nmcu, (k + 1) * ri)):
      for j, c in enumerate(comps):
        dc, ac = lookup[0 if c == 0 else 1]
        zz = [0] * 64
        pred[c] += value(symbol(dc))
        zz[0] = pred[c]
        at = 1
        while at < 64:
          s = symbol(ac)
          if s == 0x00:
            break
          if s == 0xF0:
            at += 16
            continue
          at += s >> 4
          zz[at] = value(s & 15)
          at += 1
        assert at <= 64
        out[m, j, ZIGZAG] = zz
    pad = left
    assert pad < 8 and take(pad) == (1 << pad) - 1  # the padding: 1-bits
  return out


def contents(h, w, seed):
  """the test pictures of a size: zeros, 255s, a smooth ramp plus sine with sigma-4 noise, uniform noise, a 0 / 255
  checkerboard with complementary green (its swing is in the chroma: AC size 10 in 4:4:4, averaged away in 4:2:0), and,
  added to the set so that 4:2:0 reaches AC size 10 as well, the same checkerboard in grey (its swing is in the luma)"""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  ramp = 40.0 + 150.0 * (xx + yy) / max(h + w - 2, 1) + 30.0 * np.sin(xx / 5.0) * np.cos(yy / 7.0)
  smooth = ramp[:, :, None] + np.array([0.0, 12.0, -9.0]) + rng.normal(0.0, 4.0, (h, w, 3))
  check = ((xx + yy) & 1).astype(np.uint8) * 255
  return {
      'zeros': np.zeros((h, w, 3), np.uint8),
      'ones': np.full((h, w, 3), 255, np.uint8),
      'smooth': np.clip(np.rint(smooth), 0, 255).astype(np.uint8),
      'noise': rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
      'checker': np.stack([check, 255 - check, check], axis=2),
      'grey_checker': np.stack([check, check, check], axis=2),
  }


QUALITIES = (1, 50, 90, 100)


def shapes(ri):
  return [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (64, 64), (16, 16 * (9 * ri + 1))]


@functools.lru_cache(maxsize=None)
def case_pictures(ri):
  """[(shape, name, picture)] of the case set for a restart interval"""
  return [(shape, name, pic) for shape in shapes(ri)
          for name, pic in contents(shape[0], shape[1], seed=shape[0] * 100003 + shape[1]).items()]


@functools.lru_cache(maxsize=None)
def case_files(quality, subsampling, ri):
  """the restatement of every case picture at a quality and sampling, computed once: [encode_full(...)]"""
  return [encode_full(pic, quality, subsampling, ri) for _, _, pic in case_pictures(ri)]


def psnr(a, b):
  err = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
  return 99.0 if err == 0 else 10.0 * np.log10(255.0 ** 2 / err)


def pil_decode(data):
  from PIL import Image
  return np.array(Image.open(io.BytesIO(data)).convert('RGB'))
