"""A Python restatement of the parallel entropy decoding of files without restart markers, written from
the section's text, not from the HIP code, on top of tests/jpeg_decode_host.py: the subsequences of a segment, the walk
of one subsequence from an entry state, the schedule by which the lanes agree (rounds inside a workgroup of W
subsequences, then further launches that carry a workgroup's last exit to the next), the verification with its prefix
sums and the good_blocks rule, the second walk that stores, and the serial fallback.  ``decode_sync`` returns the
coefficients, the status word, the info word and what the schedule did; tests/test_jpeg_sync_host.py holds it to
``decode_coefficients`` and the device and the rehearsal program to it."""
import numpy as np

from tests import jpeg_decode_host as host

TRUNCATED, BAD_CODE, BAD_RUN = host.TRUNCATED, host.BAD_CODE, host.BAD_RUN
DEAD = 'dead'  # the one dead state; a live state is (p, j, k)
START = (0, 0, 0)
BLOCK_CAP = 1 << 30


def nsubs_of(length, sub_bytes):
  return 1 if length <= sub_bytes else -(-length // sub_bytes)


def wrap16(v):
  return ((v + 32768) & 0xFFFF) - 32768


class SyncFile:
  """one one-segment file cut into subsequences of ``sub_bytes``; ``walk`` is memoised: it depends on (i, entry) alone"""

  def __init__(self, parsed, data, sub_bytes):
    assert len(parsed['segments']) == 1 and sub_bytes % 16 == 0 and 32 <= sub_bytes <= 65536
    self.parsed, self.sub_bytes = parsed, sub_bytes
    begin, end = parsed['segments'][0]
    stuffed = bytes(data[begin:end])
    self.stuffed = stuffed
    # a byte is dropped when it is a 00 directly behind an FF
    keep = [not (b == 0 and at > 0 and stuffed[at - 1] == 0xFF) for at, b in enumerate(stuffed)]
    raw = bytes(b for b, k in zip(stuffed, keep) if k)
    assert raw == stuffed.replace(b'\xff\x00', b'\xff')
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)  # data bytes in front of every position
    self.n = nsubs_of(len(stuffed), sub_bytes)
    self.start_bit = [8 * int(before[min(i * sub_bytes, len(stuffed))]) for i in range(self.n + 1)]  # U_i = the differences
    self.first_dropped = [0 < i * sub_bytes < len(stuffed) and not keep[i * sub_bytes] for i in range(self.n)]
    self.last_is_ff = [len(stuffed) > 0 and stuffed[min((i + 1) * sub_bytes, len(stuffed)) - 1] == 0xFF for i in range(self.n)]
    self.total = 8 * len(raw)
    self.value = int.from_bytes(raw + b'\0\0\0\0', 'big')
    self.bpm = parsed['blocks_per_mcu']
    self.comp_of = [0] * (self.bpm - 2) + [1, 2] if parsed['ncomp'] == 3 else [0]
    self.tables = {key: host._lookup(tuple(b), tuple(v)) for key, (b, v) in parsed['huff'].items()}
    self.memo = {}
    self.walks = 0

  def _symbol(self, used, table):
    syms, lengths = table
    w = (self.value >> (self.total + 32 - used - 16)) & 0xFFFF
    n, left = lengths[w], self.total - used
    if n == 0:
      return None, TRUNCATED if left < 16 else BAD_CODE
    if n > left:
      return None, TRUNCATED
    return syms[w], n

  def _value(self, used, n):
    if n > self.total - used:
      return None
    v = (self.value >> (self.total + 32 - used - n)) & ((1 << n) - 1)
    return v if v >> (n - 1) else v - (1 << n) + 1

  def walk(self, i, entry):
    """-> (exit, n, dc (three wrapping sums), flag, events): events are the stores of ``emit`` in the walk's order,
    (blocks ended so far, None, component, the sum of that component's differences so far) for a DC and (blocks ended
    so far, zigzag index, value) for an AC coefficient"""
    key = (i, entry)
    if key in self.memo:
      return self.memo[key]
    self.walks += 1
    out = self._walk(i, entry)
    self.memo[key] = out
    return out

  def _walk(self, i, entry):
    if entry == DEAD:
      return DEAD, 0, (0, 0, 0), 0, ()
    p, j, k = entry
    start, stop = self.start_bit[i], self.start_bit[i + 1]
    n, dc, events = 0, [0, 0, 0], []
    if p > self.total - start:
      return DEAD, 0, (0, 0, 0), TRUNCATED, ()
    used = start + p
    dead = lambda flag: (DEAD, n, tuple(dc), flag, tuple(events))
    for _ in range(8 * self.sub_bytes + 1):
      if used >= stop:
        break
      c = self.comp_of[j]
      _, td, ta = self.parsed['comps'][c]
      if k == 0:
        s, got = self._symbol(used, self.tables[(0, td)])
        if s is None:
          return dead(got)
        if s > 15:
          return dead(BAD_CODE)
        used += got
        v = 0
        if s:
          v = self._value(used, s)
          if v is None:
            return dead(TRUNCATED)
          used += s
        dc[c] = (dc[c] + v) & 0xFFFFFFFF
        events.append((n, None, c, dc[c]))
        k = 1
        continue
      s, got = self._symbol(used, self.tables[(1, ta)])
      if s is None:
        return dead(got)
      used += got
      run, size = s >> 4, s & 15
      if size == 0:
        if run != 15:
          k = 64  # EOB
        else:
          k += 16
          if k > 64:
            return dead(BAD_RUN)
      else:
        k += run
        if k > 63:
          return dead(BAD_RUN)
        v = self._value(used, size)
        if v is None:
          return dead(TRUNCATED)
        used += size
        events.append((n, k, v))
        k += 1
      if k == 64:
        n, k, j = n + 1, 0, (j + 1) % self.bpm
    assert used >= stop and used - stop < 32
    return (used - stop, j, k), n, tuple(dc), 0, tuple(events)


def settle(f, W, grid_rounds):
  """the schedule of the settle launches -> (ins, outs, per launch the rounds every workgroup ran, walks per subsequence)"""
  n = f.n
  ins, outs = [START] * n, [None] * n
  groups = -(-n // W)
  edge = [[None] * groups, [None] * groups]
  walks = [0] * n
  launches = []
  for r in range(grid_rounds + 1):
    rounds = []
    for wg in range(groups):  # the workgroups of a launch see only what the launch before left
      lo, hi = wg * W, min(n, wg * W + W)
      changed = [False] * (hi - lo)
      if r == 0:
        changed = [True] * (hi - lo)
      elif wg > 0 and edge[(r - 1) & 1][wg - 1] != ins[lo]:
        ins[lo], changed[0] = edge[(r - 1) & 1][wg - 1], True
      for lane in range(hi - lo):
        if changed[lane]:
          outs[lo + lane] = f.walk(lo + lane, ins[lo + lane])[0]
          walks[lo + lane] += 1
      ran = 0
      for _ in range(W):
        if not any(changed):
          break
        ran += 1
        shown = outs[lo:hi]
        changed = [lane > 0 and shown[lane - 1] != ins[lo + lane] for lane in range(hi - lo)]
        for lane in range(hi - lo):
          if changed[lane]:
            ins[lo + lane] = shown[lane - 1]
            outs[lo + lane] = f.walk(lo + lane, ins[lo + lane])[0]
            walks[lo + lane] += 1
      rounds.append(ran)
      if hi - lo == W:
        edge[r & 1][wg] = outs[hi - 1]
    launches.append(rounds)
  return ins, outs, launches, walks


def scan(f, ins, outs):
  """-> dict(settled, good_blocks, last, status, first_block [..], pred [..]) by the verification's rules"""
  blocks = f.parsed['mcus'] * f.bpm
  first, pred, ended, sums, dead_at, flag = [], [], 0, [0, 0, 0], None, 0
  for i in range(f.n):
    if ins[i] != (outs[i - 1] if i else START):
      return dict(settled=False)
    _, n, dc, fl, _ = f.walk(i, ins[i])
    first.append(min(ended, BLOCK_CAP))
    pred.append(tuple(sums))
    ended = min(ended + n, BLOCK_CAP)
    sums = [(a + b) & 0xFFFFFFFF for a, b in zip(sums, dc)]
    if outs[i] == DEAD:
      dead_at, flag = i, fl
      break
  if dead_at is None:
    flag = TRUNCATED  # no error and too few blocks: the serial walk's next symbol finds no bits
  return dict(settled=True, good_blocks=min(ended, blocks), status=flag if ended < blocks else 0,
              last=f.n - 1 if dead_at is None else dead_at, first_block=first, pred=pred)


def emit(f, ins, verdict):
  coef = np.zeros((f.parsed['mcus'] * f.bpm, 64), np.int64)
  good = verdict['good_blocks']
  for i in range(verdict['last'] + 1):
    base, pred = verdict['first_block'][i], verdict['pred'][i]
    for ev in f.walk(i, ins[i])[4]:
      if base + ev[0] >= good:
        continue
      if ev[1] is None:
        v = (pred[ev[2]] + ev[3]) & 0xFFFFFFFF
        coef[base + ev[0], 0] = wrap16(v)
      else:
        coef[base + ev[0], host.ZIGZAG[ev[1]]] = wrap16(ev[2])
  return coef.reshape(f.parsed['mcus'], f.bpm, 64)


def decode_sync(parsed, data, sub_bytes, W=256, grid_rounds=4, cache=None):
  """-> dict(coef (mcus, blocks per MCU, 64), status, info, nsubs, launches, walks, file): info 0 for a file with restart
  intervals or of one subsequence (the lane per segment), 1 through verified subsequences, 2 the serial fallback.
  ``cache`` ({}) keeps the cut files, so that a grid over W and grid_rounds walks every (subsequence, entry) once"""
  serial = lambda info, **kw: dict(zip(('coef', 'status'), host.decode_coefficients(parsed, data)[:2]), info=info, **kw)
  if len(parsed['segments']) != 1:
    return serial(0, nsubs=1)
  begin, end = parsed['segments'][0]
  if nsubs_of(end - begin, sub_bytes) == 1:
    return serial(0, nsubs=1)
  key = (id(parsed), sub_bytes)
  f = cache.get(key) if cache is not None else None
  if f is None:
    f = SyncFile(parsed, data, sub_bytes)
    if cache is not None:
      cache[key] = f
  ins, outs, launches, walks = settle(f, W, grid_rounds)
  verdict = scan(f, ins, outs)
  extra = dict(nsubs=f.n, launches=launches, walks=walks, file=f, ins=ins, outs=outs)
  if not verdict['settled']:
    return serial(2, **extra)
  return dict(coef=emit(f, ins, verdict), status=verdict['status'], info=1, verdict=verdict, **extra)


def decode_full_sync(data, sub_bytes, W=256, grid_rounds=4):
  """the picture as tests/jpeg_decode_host.decode_full makes it, from ``decode_sync``'s coefficients"""
  parsed = host.parse(data)
  got = decode_sync(parsed, data, sub_bytes, W, grid_rounds)
  pl = host.planes(parsed, got['coef'])
  h, w = parsed['h'], parsed['w']
  if parsed['ncomp'] == 1:
    rgb = np.repeat(pl[0][:, :, None], 3, axis=2)
  else:
    rgb = host.colour(pl[0], host.upsample(pl[1], parsed['sampling'], h, w), host.upsample(pl[2], parsed['sampling'], h, w))
  return dict(rgb=rgb.astype(np.uint8), status=got['status'], info=got['info'], parsed=parsed)
