"""A NumPy restatement of the device's baseline JPEG decoder, written from the section's text, not from
the HIP code: its own parser, its own Huffman decoder with the status rules, the "islow" inverse transform with 13-bit
constants, the triangle-filter chroma upsampling and the colour conversion, all in integers (int64 arrays; the section
promises that nothing leaves int32 for |d| < 2^15, which ``idct`` asserts).  ``decode(data)`` gives what
``PIL.Image.open(...).convert('RGB')`` gives, bit for bit, on the case set below (tests/test_jpeg_decode_host.py holds
it to that), and it is the device's yardstick.  It also holds that case set and the three malformed files."""
import functools
import io

import numpy as np

from tests import jpeg_host

TRUNCATED, BAD_CODE, BAD_RUN = 1, 2, 4
ZIGZAG = jpeg_host.ZIGZAG
SAMPLINGS = {(1, 1): 0, (2, 1): 1, (2, 2): 2}  # Y's (h, v) -> PIL's subsampling number


class Refused(ValueError):
  """the restatement's own refusal of a file outside the accepted set"""


# ---------------------------------------------------------------------------------------------------------- the parser
def parse(data):
  """a file -> dict(h, w, ncomp, sampling (0 / 1 / 2), ri, quant {id: 64 values, natural order}, huff {(class, id):
  (bits, vals)}, comps [(tq, td, ta)], segments [(begin, end)]: each restart interval's stuffed bytes in the file)"""
  data = bytes(data)
  if data[:2] != b'\xff\xd8':
    raise Refused('no SOI')
  out = dict(quant={}, huff={}, ri=0)
  at, sof, adobe = 2, None, None
  while True:
    if at + 4 > len(data) or data[at] != 0xFF:
      raise Refused('no marker where one must be')
    marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], 'big')
    body = data[at + 4:at + 2 + length]
    if length < 2 or len(body) != length - 2:
      raise Refused('a segment runs past the file')
    at += 2 + length
    if 0xE0 <= marker <= 0xEF or marker == 0xFE:
      if marker == 0xEE and body[:5] == b'Adobe' and len(body) >= 12:
        adobe = body[11]
    elif marker == 0xDB:
      while body:
        if body[0] >> 4:
          raise Refused('16-bit DQT')
        if (body[0] & 15) > 3 or len(body) < 65:
          raise Refused('bad DQT')
        q = np.zeros(64, np.int64)
        q[ZIGZAG] = list(body[1:65])
        out['quant'][body[0] & 15] = q
        body = body[65:]
    elif marker == 0xC4:
      while body:
        cls, ident = body[0] >> 4, body[0] & 15
        if cls > 1 or ident > 1 or len(body) < 17:
          raise Refused('bad DHT')
        bits = list(body[1:17])
        if len(body) < 17 + sum(bits) or sum(bits) > 256:
          raise Refused('bad DHT')
        out['huff'][(cls, ident)] = (bits, list(body[17:17 + sum(bits)]))
        body = body[17 + sum(bits):]
    elif marker == 0xDD:
      out['ri'] = int.from_bytes(body[:2], 'big')
    elif marker == 0xC0:
      if sof is not None:
        raise Refused('two frames')
      sof = body
    elif marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
      raise Refused('not baseline: marker %02X' % marker)
    elif marker == 0xDA:
      sos = body
      break
    else:
      raise Refused('marker %02X' % marker)
  if sof is None:
    raise Refused('no frame')
  if sof[0] != 8:
    raise Refused('%d-bit samples' % sof[0])
  out['h'], out['w'], ncomp = int.from_bytes(sof[1:3], 'big'), int.from_bytes(sof[3:5], 'big'), sof[5]
  if out['h'] == 0:
    raise Refused('DNL')
  if out['w'] == 0:
    raise Refused('no width')
  if ncomp not in (1, 3):
    raise Refused('%d components' % ncomp)
  if adobe == 0 and ncomp == 3:
    raise Refused('Adobe transform 0')
  frame = [(sof[6 + 3 * c], sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15, sof[8 + 3 * c]) for c in range(ncomp)]
  if (frame[0][1], frame[0][2]) not in SAMPLINGS or any((f[1], f[2]) != (1, 1) for f in frame[1:]):
    raise Refused('sampling')
  if ncomp == 1 and (frame[0][1], frame[0][2]) != (1, 1):
    raise Refused('sampling')
  out['ncomp'], out['sampling'] = ncomp, SAMPLINGS[(frame[0][1], frame[0][2])]
  if sos[0] != ncomp:
    raise Refused('more than one scan')
  if tuple(sos[1 + 2 * ncomp:4 + 2 * ncomp]) != (0, 63, 0):
    raise Refused('not a sequential scan')
  comps = []
  for c in range(ncomp):
    if sos[1 + 2 * c] != frame[c][0]:
      raise Refused('scan order')
    tq, td, ta = frame[c][3], sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15
    if tq not in out['quant'] or (0, td) not in out['huff'] or (1, ta) not in out['huff']:
      raise Refused('a table the scan names is not defined')
    comps.append((tq, td, ta))
  out['comps'] = comps
  for bits, vals in out['huff'].values():
    code = 0
    for n in bits:
      code = (code + n) << 1
      if code > 1 << 17:
        raise Refused('bad DHT')
    left = 0
    for length, n in enumerate(bits, 1):
      left = left * 2 + n
      if left > 1 << length:
        raise Refused('over-subscribed DHT')
  # the entropy data: every FF that no 00 follows is a marker; RSTm in order, then EOI (or the end of a cut file)
  hs, vs = [(1, 1), (2, 1), (2, 2)][out['sampling']]
  mcus = -(-out['h'] // (8 * vs)) * -(-out['w'] // (8 * hs))
  nseg = -(-mcus // out['ri']) if out['ri'] else 1
  segments, begin, stop = [], at, len(data)
  for p in range(at, len(data) - 1):
    if data[p] != 0xFF or data[p + 1] == 0:
      continue
    m = data[p + 1]
    if m == 0xD9:
      if p + 2 != len(data):
        raise Refused('bytes behind EOI')
      stop = p
      break
    if m != 0xD0 + len(segments) % 8 or len(segments) >= nseg - 1:
      raise Refused('more than one scan' if m in (0xDA, 0xC4, 0xDB) else 'marker %02X in the scan' % m)
    segments.append((begin, p))
    begin = p + 2
  segments.append((begin, stop))
  segments += [(stop, stop)] * (nseg - len(segments))  # a cut file: the intervals that are not there are empty
  out['segments'], out['mcus'], out['blocks_per_mcu'] = segments, mcus, (hs * vs + 2 if ncomp == 3 else 1)
  return out


# ------------------------------------------------------------------------------------------------- entropy decoding
@functools.lru_cache(maxsize=None)
def _lookup(bits, vals):
  """16-bit window -> (symbol, length), length 0 where no code matches (T.81 Annex C's canonical codes)"""
  sym, length = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
  code, k = 0, 0
  for n in range(1, 17):
    for _ in range(bits[n - 1]):
      lo = code << (16 - n)
      sym[lo:lo + (1 << (16 - n))] = vals[k]
      length[lo:lo + (1 << (16 - n))] = n
      code += 1
      k += 1
    code <<= 1
  return sym.tolist(), length.tolist()


class _Stop(Exception):
  def __init__(self, flag):
    self.flag = flag


class _Bits:
  """a segment's bits after unstuffing; past the end the window reads zeros"""

  def __init__(self, stuffed):
    raw = stuffed.replace(b'\xff\x00', b'\xff')
    self.total = 8 * len(raw)
    self.value = int.from_bytes(raw + b'\0\0\0\0', 'big')
    self.used = 0
    self.stuffed_ff = len(stuffed) - len(raw)

  def window(self):
    return (self.value >> (self.total + 32 - self.used - 16)) & 0xFFFF

  def symbol(self, table, track):
    syms, lengths = table
    w = self.window()
    n = lengths[w]
    left = self.total - self.used
    if n == 0:
      raise _Stop(TRUNCATED if left < 16 else BAD_CODE)
    if n > left:
      raise _Stop(TRUNCATED)
    self.used += n
    track['longest'] = max(track['longest'], n)
    return syms[w]

  def value_of(self, n):
    if n == 0:
      return 0
    if n > self.total - self.used:
      raise _Stop(TRUNCATED)
    v = (self.value >> (self.total + 32 - self.used - n)) & ((1 << n) - 1)
    self.used += n
    return v if v >> (n - 1) else v - (1 << n) + 1


def decode_coefficients(parsed, data):
  """-> (coefficients (mcus, blocks per MCU, 64) in natural order, status, what the walk met: a dict of counters)"""
  ncomp, bpm, mcus = parsed['ncomp'], parsed['blocks_per_mcu'], parsed['mcus']
  comp_of = [0] * (bpm - 2) + [1, 2] if ncomp == 3 else [0]
  tables = {key: _lookup(tuple(b), tuple(v)) for key, (b, v) in parsed['huff'].items()}
  ri = parsed['ri'] or mcus
  coef = np.zeros((mcus, bpm, 64), np.int64)
  status = 0
  met = dict(longest=0, zrl=0, eob=0, last=0, stuffed=0, resets=0)
  for k, (begin, end) in enumerate(parsed['segments']):
    bits = _Bits(bytes(data[begin:end]))
    met['stuffed'] += bits.stuffed_ff
    met['resets'] += k > 0
    pred = [0, 0, 0]
    try:
      for m in range(k * ri, min(mcus, (k + 1) * ri)):
        for j in range(bpm):
          c = comp_of[j]
          _, td, ta = parsed['comps'][c]
          zz = [0] * 64
          s = bits.symbol(tables[(0, td)], met)
          if s > 15:
            raise _Stop(BAD_CODE)
          pred[c] += bits.value_of(s)
          zz[0] = pred[c]
          at = 1
          while at < 64:
            s = bits.symbol(tables[(1, ta)], met)
            run, size = s >> 4, s & 15
            if size == 0:
              if run != 15:
                met['eob'] += 1
                break
              met['zrl'] += 1
              at += 16
              if at > 64:
                raise _Stop(BAD_RUN)
              continue
            at += run
            if at > 63:
              raise _Stop(BAD_RUN)
            zz[at] = bits.value_of(size)
            met['last'] += at == 63
            at += 1
          coef[m, j, ZIGZAG] = zz
    except _Stop as stop:
      status |= stop.flag
  return coef, status, met


# ---------------------------------------------------------------------------------------------------- reconstruction
C0_298, C0_390, C0_541, C0_765, C0_899, C1_175 = 2446, 3196, 4433, 6270, 7373, 9633
C1_501, C1_847, C1_961, C2_053, C2_562, C3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def idct_pass(i, s):
  """one 8-point pass over axis 0 of eight arrays"""
  i0, i1, i2, i3, i4, i5, i6, i7 = i
  z1 = (i2 + i6) * C0_541
  t2 = z1 - i6 * C1_847
  t3 = z1 + i2 * C0_765
  t0 = (i0 + i4) << 13
  t1 = (i0 - i4) << 13
  t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
  a, b, c, e = i7, i5, i3, i1
  z1, z2, z3, z4 = a + e, b + c, a + c, b + e
  z5 = (z3 + z4) * C1_175
  a, b, c, e = a * C0_298, b * C2_053, c * C3_072, e * C1_501
  z1, z2, z3, z4 = z1 * -C0_899, z2 * -C2_562, z3 * -C1_961 + z5, z4 * -C0_390 + z5
  a, b, c, e = a + z1 + z3, b + z2 + z4, c + z2 + z3, e + z1 + z4
  out = [t10 + e, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - e]
  for o in out + [t10, t11, t12, t13, a, b, c, e, z5]:
    assert np.abs(o).max(initial=0) < 2 ** 31
  return [(o + (1 << (s - 1))) >> s for o in out]


def idct(d):
  """(..., 8, 8) dequantised blocks [v][u] -> samples 0..255"""
  cols = np.stack(idct_pass([d[..., v, :] for v in range(8)], 11), axis=-2)  # over v for every column
  rows = np.stack(idct_pass([cols[..., :, u] for u in range(8)], 18), axis=-1)
  return np.clip(rows + 128, 0, 255)


def planes(parsed, coef):
  """the component planes, cropped to their real samples"""
  h, w, ncomp, bpm = parsed['h'], parsed['w'], parsed['ncomp'], parsed['blocks_per_mcu']
  hs, vs = [(1, 1), (2, 1), (2, 2)][parsed['sampling']]
  my, mx = -(-h // (8 * vs)), -(-w // (8 * hs))
  out = []
  for c in range(ncomp):
    q = parsed['quant'][parsed['comps'][c][0]]
    if c == 0:
      blocks = coef[:, :hs * vs].reshape(my, mx, vs, hs, 8, 8) * q.reshape(8, 8)
      full = idct(blocks).transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)
      out.append(full[:h, :w])
    else:
      blocks = coef[:, hs * vs + c - 1].reshape(my, mx, 8, 8) * q.reshape(8, 8)
      full = idct(blocks).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)
      out.append(full[:-(-h // vs), :-(-w // hs)])
  return out


def upsample(p, sampling, h, w, met=None):
  """a chroma plane of real samples -> (h, w), libjpeg's "fancy" triangle filter with clamped indices"""
  if sampling == 0:
    return p
  dh, dw = p.shape
  xs = np.arange(dw)
  left, right = np.maximum(xs - 1, 0), np.minimum(xs + 1, dw - 1)
  if met is not None:
    met.update(left=bool((xs - 1 < 0).any()), right=bool((xs + 1 > dw - 1).any()), inner_x=dw > 2)
  if sampling == 1:
    out = np.empty((dh, 2 * dw), np.int64)
    out[:, 0::2] = (3 * p + p[:, left] + 1) >> 2
    out[:, 1::2] = (3 * p + p[:, right] + 2) >> 2
    return out[:h, :w]
  ys = np.arange(dh)
  up, down = np.maximum(ys - 1, 0), np.minimum(ys + 1, dh - 1)
  if met is not None:
    met.update(up=True, down=True, inner_y=dh > 2)
  r = np.empty((2 * dh, dw), np.int64)
  r[0::2] = 3 * p + p[up]
  r[1::2] = 3 * p + p[down]
  out = np.empty((2 * dh, 2 * dw), np.int64)
  out[:, 0::2] = (3 * r + r[:, left] + 8) >> 4
  out[:, 1::2] = (3 * r + r[:, right] + 7) >> 4
  return out[:h, :w]


def colour(y, cb, cr, met=None):
  cb, cr = cb - 128, cr - 128
  raw = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                  y + ((116130 * cb + 32768) >> 16)], axis=-1)
  if met is not None:
    met['below'] = met.get('below', False) or bool((raw < 0).any())
    met['above'] = met.get('above', False) or bool((raw > 255).any())
  return np.clip(raw, 0, 255)


def decode_full(data):
  """-> dict(rgb (H, W, 3) uint8, status, parsed, met)"""
  parsed = parse(data)
  coef, status, met = decode_coefficients(parsed, data)
  pl = planes(parsed, coef)
  h, w = parsed['h'], parsed['w']
  if parsed['ncomp'] == 1:
    rgb = np.repeat(pl[0][:, :, None], 3, axis=2)
  else:
    rgb = colour(pl[0], upsample(pl[1], parsed['sampling'], h, w, met), upsample(pl[2], parsed['sampling'], h, w), met)
  return dict(rgb=rgb.astype(np.uint8), status=status, parsed=parsed, met=met)


def decode(data):
  return decode_full(data)['rgb']


def pil_decode(data):
  from PIL import Image
  return np.array(Image.open(io.BytesIO(data)).convert('RGB'))


# -------------------------------------------------------------------------------------------------------- the case set
SHAPES = ((1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (33, 50), (64, 64))
QUALITIES = (1, 50, 90, 100)
VARIANTS = (('default', {}), ('optimize', dict(optimize=True)), ('rst3', dict(restart_marker_blocks=3)),
            ('rstrow', dict(restart_marker_rows=1)))
CONTENTS = ('smooth', 'noise', 'checker', 'grey_checker')


def pil_encode(pic, mode='RGB', **kw):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(pic, mode).save(buf, 'JPEG', **kw)
  return buf.getvalue()


def merge_tables(data):
  """byte surgery: both DQT tables into one segment, all four DHT tables into one"""
  segs, at = [], 2
  while True:
    marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], 'big')
    segs.append((marker, data[at + 4:at + 2 + length]))
    at += 2 + length
    if marker == 0xDA:
      break
  out, done = b'\xff\xd8', set()
  for marker, body in segs:
    if marker in (0xDB, 0xC4):
      if marker in done:
        continue
      done.add(marker)
      body = b''.join(b for m, b in segs if m == marker)
    out += bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + body
  assert sum(m == 0xDB for m, _ in segs) >= 2 and sum(m == 0xC4 for m, _ in segs) >= 4
  return out + data[at:]


@functools.lru_cache(maxsize=None)
def case_files():
  """[(name, file bytes)]: every file of the case set, made once"""
  out, k = [], 0
  for shape in SHAPES:
    pics = jpeg_host.contents(shape[0], shape[1], seed=shape[0] * 100003 + shape[1])
    for quality in QUALITIES:
      for sub in (0, 1, 2):
        for vname, kw in VARIANTS:
          content = CONTENTS[k % len(CONTENTS)]
          k += 1
          out.append(('%dx%d-%s-q%d-s%d-%s' % (shape + (content, quality, sub, vname)),
                      pil_encode(pics[content], quality=quality, subsampling=sub, **kw)))
    for quality in (50, 100):
      for vname, kw in VARIANTS[:3]:
        out.append(('%dx%d-L-q%d-%s' % (shape + (quality, vname)),
                    pil_encode(np.ascontiguousarray(pics['noise'][..., 1]), 'L', quality=quality, **kw)))
    for sub, ri in ((0, 16), (2, 8)):
      out.append(('%dx%d-own-s%d' % (shape + (sub,)), jpeg_host.encode(pics['smooth'], 90, sub, ri)))
  wide = jpeg_host.contents(8, 1040, seed=8 * 100003 + 1040)['noise']
  out.append(('8x1040-rst1', pil_encode(wide, quality=90, subsampling=0, restart_marker_blocks=1)))
  pics = jpeg_host.contents(33, 50, seed=77)
  out.append(('33x50-comment-exif', pil_encode(pics['smooth'], quality=90, comment=b'a comment', exif=b'Exif\0\0MM\0*\0\0\0\x08\0\0\0\0\0\0')))
  out.append(('33x50-merged-s2', merge_tables(pil_encode(pics['noise'], quality=50, subsampling=2))))
  out.append(('17x33-merged-s0', merge_tables(pil_encode(jpeg_host.contents(17, 33, seed=78)['noise'], quality=90, subsampling=0, optimize=True))))
  return out


@functools.lru_cache(maxsize=None)
def case_decoded():
  """the restatement of every case file, computed once and shared: [decode_full(file)]"""
  return [decode_full(data) for _, data in case_files()]


def entropy_start(data):
  """the offset of the first entropy-coded byte"""
  at = 2
  while True:
    marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], 'big')
    at += 2 + length
    if marker == 0xDA:
      return at


@functools.lru_cache(maxsize=None)
def malformed_files():
  """[(name, file bytes)]: ordinary malformed inputs that the decoder must bound -- entropy data cut in half, a payload
  of FF 00 repeated (sixteen 1-bits match no code of Annex K's tables), a payload of seeded random bytes (stuffed)"""
  good = pil_encode(jpeg_host.contents(33, 50, seed=79)['noise'], quality=90, subsampling=2)
  start = entropy_start(good)
  rng = np.random.default_rng(2024)
  noise = rng.integers(0, 256, 600, dtype=np.uint8).tobytes().replace(b'\xff', b'\xff\x00')
  return [('cut', good[:start + (len(good) - 2 - start) // 2]),
          ('ones', good[:start] + b'\xff\x00' * 300 + b'\xff\xd9'),
          ('random', good[:start] + noise + b'\xff\xd9')]
