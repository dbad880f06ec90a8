"""Baseline JPEG input files decoded on the device: the file's bytes are uploaded as they are and
``expo_jpeg_decode_ragged`` makes the (H, W, 3) uint8 codes that ``PIL.Image.open(...).convert('RGB')`` makes, bit for bit.

``parse`` is the host's share: the header fields, the tables, and the byte range of every restart interval, found with
a vectorised search for the markers (a byte scan, not a codec).  It refuses, with ``UnsupportedJpeg`` and a reason,
every file outside the accepted set before anything is enqueued; such a file goes through PIL as before.
"""
import numpy as np

from . import _cabi

TRUNCATED, BAD_CODE, BAD_RUN = 1, 2, 4  # the flags of a picture's status word
STATUS_NAMES = ((TRUNCATED, 'TRUNCATED'), (BAD_CODE, 'BAD_CODE'), (BAD_RUN, 'BAD_RUN'))
PLAN_HEAD_BYTES = 1808
SUB_BYTES = 128  # the subsequence of the parallel entropy walk; the fastest of 64..512 on smooth 16 x 512x512 files, not on noise: profiles/jpeg_decode.md
GRID_ROUNDS = 4  # further settle launches, each carries a state across one more boundary between workgroups; not swept
SYNC_MIN_BYTES = 4096  # 'auto': a file whose one segment has at least this many bytes takes the parallel walk; not swept (noise-like files lose 0.60x - 0.79x by it)
MAX_BYTES = 1 << 30  # the workspace of one call (coefficients and planes: 3.5 to 5 bytes per pixel), as datasets.MAX_BYTES

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                    14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                    46, 53, 60, 61, 54, 47, 55, 62, 63])
_SAMPLINGS = {(1, 1): 0, (2, 1): 1, (2, 2): 2}  # Y's (h, v) -> PIL's subsampling number
_NOT_BASELINE = {0xC1: 'extended sequential (SOF1)', 0xC2: 'progressive (SOF2)', 0xC3: 'lossless (SOF3)',
                 0xC5: 'differential (SOF5)', 0xC6: 'differential progressive (SOF6)', 0xC7: 'differential lossless (SOF7)',
                 0xC9: 'arithmetic coding (SOF9)', 0xCA: 'arithmetic coding (SOF10)', 0xCB: 'arithmetic coding (SOF11)',
                 0xCC: 'arithmetic coding (DAC)', 0xCD: 'arithmetic coding (SOF13)', 0xCE: 'arithmetic coding (SOF14)',
                 0xCF: 'arithmetic coding (SOF15)'}


class UnsupportedJpeg(ValueError):
  """a file outside the set the device decoder accepts (the reason is the message): use the PIL path"""


class JpegDataError(ValueError):
  """entropy-coded data that did not decode: the message names the files and their status flags"""


def status_text(status):
  return '|'.join(name for flag, name in STATUS_NAMES if status & flag) or 'OK'


def is_jpeg_path(path):
  return str(path).lower().endswith(('.jpg', '.jpeg'))


class Plan(object):
  """what ``parse`` found: h, w, ncomp (1 or 3), sampling (PIL's 0 / 1 / 2), ri (0: no DRI), quant {id: 64 values in
  natural order}, huff {(class, id): (BITS, HUFFVAL)}, comps [(tq, td, ta)], segments (nsegs, 2) int32 byte ranges of
  the restart intervals' stuffed bytes, nbytes (the file's length), and ``blob``: the device decoder's plan as uint8"""

  def __init__(self, **kw):
    self.__dict__.update(kw)

  @property
  def nsegs(self):
    return int(self.segments.shape[0])

  @property
  def segment_bytes(self):
    """the bytes of the one segment of a file without restart markers, as the device clamps them; 0 for other files"""
    if self.nsegs != 1:
      return 0
    begin = min(max(int(self.segments[0, 0]), 0), self.nbytes)
    return min(max(int(self.segments[0, 1]), begin), self.nbytes) - begin

  def nsubs(self, sub_bytes):
    """the subsequences of ``sub_bytes`` bytes of a file without restart markers (at least one); 1 for other files"""
    return 1 if self.segment_bytes <= sub_bytes else -(-self.segment_bytes // int(sub_bytes))


def _huff_arrays(bits, vals):
  """T.81 Annex C -> (limit[16], offs[16], vals[256]) of csrc/jpeg_decode.h, or None for an impossible table"""
  limit, offs, code, k = np.zeros(16, np.uint32), np.zeros(16, np.int32), 0, 0
  for length in range(1, 17):
    offs[length - 1] = k - code  # VALPTR - MINCODE
    code += bits[length - 1]
    k += bits[length - 1]
    if code > 1 << length:
      return None
    limit[length - 1] = code << (16 - length)
    code <<= 1
  out = np.zeros(256, np.uint8)
  out[:len(vals)] = vals
  return limit, offs, out


def parse(data):
  """the bytes of a file -> ``Plan``, or ``UnsupportedJpeg``"""
  d = np.frombuffer(bytes(data), np.uint8)
  n = d.size
  if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
    raise UnsupportedJpeg('not a JPEG file (no SOI)')
  quant, huff, ri, sof, sos, adobe, at = {}, {}, 0, None, None, None, 2
  while sos is None:
    if at + 4 > n or d[at] != 0xFF:
      raise UnsupportedJpeg('no marker segment at byte %d' % at)
    marker, length = int(d[at + 1]), int(d[at + 2]) << 8 | int(d[at + 3])
    body = d[at + 4:at + 2 + length]
    if length < 2 or body.size != length - 2:
      raise UnsupportedJpeg('a marker segment runs past the end of the file')
    at += 2 + length
    if marker in _NOT_BASELINE:
      raise UnsupportedJpeg(_NOT_BASELINE[marker])
    if 0xE0 <= marker <= 0xEF or marker == 0xFE:
      if marker == 0xEE and body.size >= 12 and body[:5].tobytes() == b'Adobe':
        adobe = int(body[11])
    elif marker == 0xDB:
      while body.size:
        if body[0] >> 4:
          raise UnsupportedJpeg('16-bit quantiser table')
        if (body[0] & 15) > 3 or body.size < 65:
          raise UnsupportedJpeg('malformed DQT')
        q = np.zeros(64, np.uint8)
        q[_ZIGZAG] = body[1:65]
        quant[int(body[0] & 15)] = q
        body = body[65:]
    elif marker == 0xC4:
      while body.size:
        cls, ident = int(body[0] >> 4), int(body[0] & 15)
        if cls > 1 or ident > 1 or body.size < 17:
          raise UnsupportedJpeg('Huffman table class %d id %d' % (cls, ident))
        bits = body[1:17].astype(np.int64)
        count = int(bits.sum())
        if count > 256 or body.size < 17 + count:
          raise UnsupportedJpeg('malformed DHT')
        huff[(cls, ident)] = (bits.tolist(), body[17:17 + count].tolist())
        body = body[17 + count:]
    elif marker == 0xDD:
      if body.size < 2:
        raise UnsupportedJpeg('malformed DRI')
      ri = int(body[0]) << 8 | int(body[1])
    elif marker == 0xC0:
      if sof is not None:
        raise UnsupportedJpeg('more than one frame')
      sof = body
    elif marker == 0xDA:
      sos = body
    else:
      raise UnsupportedJpeg('marker FF%02X' % marker)
  if sof is None or sof.size < 6 or sof.size < 6 + 3 * int(sof[5]):
    raise UnsupportedJpeg('no frame header before the scan')
  if sof[0] != 8:
    raise UnsupportedJpeg('%d-bit samples' % sof[0])
  h, w, ncomp = int(sof[1]) << 8 | int(sof[2]), int(sof[3]) << 8 | int(sof[4]), int(sof[5])
  if h == 0:
    raise UnsupportedJpeg('the height comes in a DNL segment (h = 0)')
  if w == 0:
    raise UnsupportedJpeg('zero width')
  if ncomp not in (1, 3):
    raise UnsupportedJpeg('%d components' % ncomp)
  if adobe == 0 and ncomp == 3:
    raise UnsupportedJpeg('Adobe APP14 with transform 0 (RGB, not YCbCr)')
  frame = [(int(sof[6 + 3 * c]), int(sof[7 + 3 * c] >> 4), int(sof[7 + 3 * c] & 15), int(sof[8 + 3 * c])) for c in range(ncomp)]
  y_sampling = (frame[0][1], frame[0][2])
  if y_sampling not in _SAMPLINGS or any((f[1], f[2]) != (1, 1) for f in frame[1:]) or (ncomp == 1 and y_sampling != (1, 1)):
    raise UnsupportedJpeg('sampling %s' % ', '.join('%dx%d' % (f[1], f[2]) for f in frame))
  sampling = _SAMPLINGS[y_sampling]
  if sos.size < 1 or sos[0] != ncomp or sos.size < 4 + 2 * ncomp:
    raise UnsupportedJpeg('more than one scan (the first holds %d of %d components)' % (sos[0] if sos.size else 0, ncomp))
  if tuple(int(v) for v in sos[1 + 2 * ncomp:4 + 2 * ncomp]) != (0, 63, 0):
    raise UnsupportedJpeg('not a sequential scan (Ss, Se, Ah/Al)')
  comps = []
  for c in range(ncomp):
    if sos[1 + 2 * c] != frame[c][0]:
      raise UnsupportedJpeg('the scan does not hold the components in the frame\'s order')
    tq, td, ta = frame[c][3], int(sos[2 + 2 * c] >> 4), int(sos[2 + 2 * c] & 15)
    if tq not in quant or (0, td) not in huff or (1, ta) not in huff:
      raise UnsupportedJpeg('the scan names a table that no segment defines')
    comps.append((tq, td, ta))
  tables = {}
  for key, (bits, vals) in huff.items():
    tables[key] = _huff_arrays(bits, vals)
    if tables[key] is None:
      raise UnsupportedJpeg('over-subscribed Huffman table')
  # the entropy-coded data: every FF that is not the last byte and that no 00 follows is a marker
  hs, vs = ((1, 1), (2, 1), (2, 2))[sampling]
  mcus = -(-h // (8 * vs)) * -(-w // (8 * hs))
  nsegs = -(-mcus // ri) if ri else 1
  rest = d[at:]
  where = at + np.flatnonzero((rest[:-1] == 0xFF) & (rest[1:] != 0)) if rest.size > 1 else np.zeros(0, np.int64)
  found = d[where + 1].astype(np.int64)
  stop, ends = n, np.flatnonzero(found == 0xD9)
  if ends.size:
    stop = int(where[ends[0]])
    if stop + 2 != n:
      raise UnsupportedJpeg('bytes behind EOI')
    where, found = where[:ends[0]], found[:ends[0]]
  if where.size > nsegs - 1 or np.any(found != 0xD0 + np.arange(where.size) % 8):
    odd = found[found != 0xD0 + np.arange(found.size) % 8]
    odd = int(odd[0]) if odd.size else int(found[nsegs - 1])
    raise UnsupportedJpeg('more than one scan' if odd in (0xDA, 0xC4, 0xDB) else 'marker FF%02X inside the scan' % odd)
  segments = np.full((nsegs, 2), stop, np.int64)  # a cut file: the intervals that are not there are empty
  segments[:where.size + 1, 0] = np.concatenate([[at], where + 2])
  segments[:where.size, 1] = where
  if n >= 1 << 31:
    raise UnsupportedJpeg('a file of 2 GiB or more')
  blob = np.zeros(PLAN_HEAD_BYTES + (nsegs * 8 + 15) // 16 * 16, np.uint8)
  blob[0:4] = np.array([ri], '<i4').view(np.uint8)
  for c, (tq, td, ta) in enumerate(comps):
    blob[4 + c], blob[8 + c], blob[12 + c] = tq, td, ta
  for ident, q in quant.items():
    blob[16 + 64 * ident:16 + 64 * ident + 64] = q
  for (cls, ident), (limit, offs, vals) in tables.items():
    o = 272 + 384 * (2 * cls + ident)
    blob[o:o + 64] = limit.astype('<u4').view(np.uint8)
    blob[o + 64:o + 128] = offs.astype('<i4').view(np.uint8)
    blob[o + 128:o + 384] = vals
  blob[PLAN_HEAD_BYTES:PLAN_HEAD_BYTES + nsegs * 8] = segments.astype('<i4').reshape(-1).view(np.uint8)
  return Plan(h=h, w=w, ncomp=ncomp, sampling=sampling, ri=ri, quant=quant, huff=huff, comps=comps,
              segments=segments.astype(np.int32), nbytes=n, mcus=mcus, blob=blob)


def workspace_bytes(plans, sub_bytes=None):
  """the scratch of one call on these files: the serial call's, or with ``sub_bytes`` the parallel call's"""
  if sub_bytes is None:
    return _cabi.jpeg_decode_workspace_bytes([p.h for p in plans], [p.w for p in plans], [p.sampling for p in plans],
                                             [p.ncomp for p in plans])
  return _cabi.jpeg_decode_sync_workspace_bytes([p.h for p in plans], [p.w for p in plans], [p.sampling for p in plans],
                                                [p.ncomp for p in plans], [p.nsegs for p in plans],
                                                [p.nsubs(sub_bytes) for p in plans])


def decode_jpeg_batch(datas, device, errors='raise', plans=None, max_bytes=MAX_BYTES, names=None, sync='auto',
                      sub_bytes=SUB_BYTES, grid_rounds=GRID_ROUNDS, sync_min_bytes=SYNC_MIN_BYTES, info=False):
  """the bytes of N baseline JPEG files -> (N contiguous (H, W, 3) uint8 tensors on ``device``, their status words as a
  list of ints).  ``parse`` runs on every file first (``UnsupportedJpeg`` propagates; pass ``plans=`` to reuse earlier
  results), then the files and plans are uploaded in one copy and decoded in as few calls as a workspace of
  ``max_bytes`` allows (a picture that needs more on its own gets a call of its own).  errors='raise': a non-zero
  status raises ``JpegDataError`` naming the files (``names``, default their indices); 'return': the caller looks.
  sync: True decodes through ``expo_jpeg_decode_sync_ragged`` (a file without restart markers is walked
  by a lane per subsequence of ``sub_bytes`` bytes, with ``grid_rounds`` further settle launches), False through
  ``expo_jpeg_decode_ragged`` (a lane per file for such files), 'auto' through the former when a file of the call has
  one segment of at least ``sync_min_bytes`` bytes; the tensors and status words are the same either way.  info=True
  also returns the info words as a third list (0 a lane per segment, 1 verified subsequences, 2 the serial fallback;
  all 0 through the serial call)."""
  import torch
  if errors not in ('raise', 'return'):
    raise ValueError("errors must be 'raise' or 'return'")
  if sync not in ('auto', True, False):
    raise ValueError("sync must be 'auto', True or False")
  device = torch.device(device)
  datas = [bytes(x) for x in datas]
  plans = [parse(x) for x in datas] if plans is None else list(plans)
  if len(plans) != len(datas):
    raise ValueError('datas and plans must have the same length')
  n = len(datas)
  if n == 0:
    return ([], [], []) if info else ([], [])
  if sync == 'auto':
    sync = any(p.nsegs == 1 and p.segment_bytes >= sync_min_bytes for p in plans)
  # one upload: every plan at a multiple of 16 bytes, then the files back to back
  offs, at = [], 0
  for p in plans:
    offs.append(at)
    at += p.blob.size  # a multiple of 16
  foffs = []
  for x in datas:
    foffs.append(at)
    at += len(x)
  host = np.empty(max(at, 1), np.uint8)
  for o, p in zip(offs, plans):
    host[o:o + p.blob.size] = p.blob
  for o, x in zip(foffs, datas):
    host[o:o + len(x)] = np.frombuffer(x, np.uint8)
  blob = torch.from_numpy(host).to(device)
  outs = [torch.empty((p.h, p.w, 3), dtype=torch.uint8, device=device) for p in plans]
  status = torch.empty((n,), dtype=torch.int32, device=device)
  words = torch.zeros((n,), dtype=torch.int32, device=device) if info else None
  each = [workspace_bytes([p], sub_bytes if sync else None) for p in plans]  # a call's workspace is at most the sum of its pictures'
  start = 0
  while start < n:
    stop, total = start + 1, each[start]
    while stop < n and total + each[stop] <= max_bytes:
      total += each[stop]
      stop += 1
    sel = range(start, stop)
    args = ([blob[foffs[i]:foffs[i] + len(datas[i])] for i in sel], [blob[offs[i]:offs[i] + plans[i].blob.size] for i in sel],
            [plans[i].h for i in sel], [plans[i].w for i in sel], [plans[i].sampling for i in sel],
            [plans[i].ncomp for i in sel], [plans[i].nsegs for i in sel])
    if sync:
      _cabi.jpeg_decode_sync_ragged(*args, [plans[i].nsubs(sub_bytes) for i in sel], sub_bytes, grid_rounds,
                                    [outs[i] for i in sel], status[start:stop], words[start:stop] if info else None)
    else:
      _cabi.jpeg_decode_ragged(*args, [outs[i] for i in sel], status[start:stop])
    start = stop
  statuses = [int(s) for s in status.cpu().tolist()]
  if errors == 'raise' and any(statuses):
    names = list(range(n)) if names is None else list(names)
    raise JpegDataError('JPEG entropy data did not decode: ' +
                        ', '.join('%s (%s)' % (names[i], status_text(s)) for i, s in enumerate(statuses) if s))
  return (outs, statuses, [int(v) for v in words.cpu().tolist()]) if info else (outs, statuses)
