// jpeg_decode_sync.h -- the serial integer routines of csrc/jpeg_decode_sync.hip, written so that they
// also compile for the host: tools/jpeg_sync_rehearse.cpp runs them under -fsanitize=address,undefined over whole files.
// No float, no state.  A file without restart markers is one segment; these routines cut it into subsequences of
// sub_bytes file bytes, walk one subsequence from a given entry state (`walk`), and walk it again storing coefficients
// (`emit`).  The symbol, value and status rules are jpeg_decode.h's own functions: a walk is decode_block's loop turned
// into one loop over symbols with a count of the bits it consumed.
//
// Subsequence i of the segment [begin, end) is the file bytes [begin + i B, min(begin + (i + 1) B, end)).  Its bits are
// those bytes with the byte behind every FF dropped, the reader's rule; its first byte is dropped when it is a 00 and
// the byte before it is an FF at or behind `begin`.  U_i is the number of those bits.  A symbol (a code and its
// appended bits, at most 31 bits) belongs to the subsequence in which it starts.
//
// A state is one packed word: p (bits 0..4) the bits past the subsequence's own start, j (bits 5..7) the block in the
// MCU, k (bits 8..13) the next coefficient index (0: a DC symbol is due), dead (bit 14; a dead state is kDead alone).
// The payload beside a state's exit is four words: n | flag << 28 (the blocks that ended during the walk; after an
// error the flag, and n counts the blocks that ended before it) and the wrapping sums of the DC differences read
// during the walk, per component.
#pragma once
#include "jpeg_decode.h"

namespace expo {
namespace jpegsync {

using namespace jpegdec;

constexpr int kMinSubBytes = 32, kMaxSubBytes = 65536;
constexpr int kMaxGridRounds = 16;
constexpr uint32_t kDead = 1u << 14;
constexpr uint32_t kCountMask = (1u << 28) - 1;
constexpr int64_t kBlockCap = int64_t(1) << 30;  // prefix sums of n saturate here: above any picture's blocks (< 2^28)

EXPO_HD bool valid_sub_bytes(int64_t b) { return b >= kMinSubBytes && b <= kMaxSubBytes && b % 16 == 0; }
EXPO_HD uint32_t pack_state(int p, int j, int k) { return uint32_t(p) | uint32_t(j) << 5 | uint32_t(k) << 8; }

struct Payload {
  uint32_t n;  // blocks | flag << 28
  uint32_t dc[3];
};
static_assert(sizeof(Payload) == 16, "the payload's layout");

// the segment of a one-segment picture, clamped to the file as open_bits clamps it
struct Segment {
  int64_t begin, end;
};
EXPO_HD Segment plan_segment(const uint8_t* planp, int64_t file_bytes) {
  const int32_t* range = reinterpret_cast<const int32_t*>(planp + sizeof(PlanHead));
  Segment s;
  s.begin = range[0] < 0 ? 0 : range[0] > file_bytes ? file_bytes : range[0];
  s.end = range[1] < s.begin ? s.begin : range[1] > file_bytes ? file_bytes : range[1];
  return s;
}
// the subsequences of a segment of `bytes` bytes: at least one
EXPO_HD int64_t sub_count(int64_t bytes, int64_t sub_bytes) { return bytes <= sub_bytes ? 1 : (bytes + sub_bytes - 1) / sub_bytes; }

// where subsequence i's bits start in the file and how many they are (U_i); at most sub_bytes byte reads
struct SubBits {
  int64_t pos;
  int bits;
};
EXPO_HD SubBits sub_bits(const uint8_t* file, const Segment& seg, int sub_bytes, int64_t i) {
  int64_t s = seg.begin + i * sub_bytes;
  s = s > seg.end ? seg.end : s;
  const int64_t e = s + sub_bytes < seg.end ? s + sub_bytes : seg.end;
  SubBits u;
  u.pos = s > seg.begin && s < e && file[s] == 0 && file[s - 1] == 0xFFu ? s + 1 : s;
  int count = 0;
  int64_t q = u.pos;
  for (int t = 0; t < sub_bytes && q < e; ++t) {
    q += file[q] == 0xFFu ? 2 : 1;
    ++count;
  }
  u.bits = 8 * count;
  return u;
}

// One walk of subsequence `u` from `entry`: the exit state, the payload in *pay.  With kEmit it also stores the
// coefficients it meets: a DC as int16(pred[c] + the differences read so far) and an AC coefficient through the zigzag,
// into block first_block + (blocks ended so far) of `coef` (int16, 64 per block), only below good_blocks.  At most
// 8 sub_bytes + 1 symbols whatever the data; every read is inside the file (open_bits clamps).
template <bool kEmit>
EXPO_HD uint32_t walk_or_emit(const uint8_t* file, int64_t file_bytes, const uint8_t* planp, const Geometry& g, const Segment& seg,
                              int sub_bytes, const SubBits& u, uint32_t entry, Payload* pay, int64_t first_block,
                              const uint32_t* pred, int64_t good_blocks, int16_t* coef) {
  const PlanHead* plan = reinterpret_cast<const PlanHead*>(planp);
  uint32_t dc0 = 0, dc1 = 0, dc2 = 0;
  int n = 0, st = 0;
  bool dead = (entry & kDead) != 0;
  int j = int(entry >> 5) & 7, k = int(entry >> 8) & 63;
  if (j >= g.bpm) j = 0;
  int consumed = int(entry & 31u);
  if constexpr (kEmit) dc0 = pred[0], dc1 = pred[1], dc2 = pred[2];
  if (!dead) {
    BitReader r = open_bits(file, file_bytes, u.pos, seg.end);
    fill(r);
    if (consumed > r.nbits) {
      st |= kTruncated;
      dead = true;
    } else {
      skip(r, consumed);
    }
    const int most = 8 * sub_bytes + 1;
    for (int e = 0; e < most && !dead && consumed < u.bits; ++e) {
      const int c = block_component(g, j);
      fill(r);
      const int before = r.nbits;
      int v = 0;
      bool ended = false;
      if (k == 0) {
        const int s = symbol(r, plan->huff[plan->td[c & 3] & 1], &st);
        if (s < 0) {
          dead = true;
        } else if (s > 15) {
          st |= kBadCode;
          dead = true;
        } else if (s && !value(r, s, &v, &st)) {
          dead = true;
        } else {
          dc0 += c == 0 ? uint32_t(v) : 0u, dc1 += c == 1 ? uint32_t(v) : 0u, dc2 += c == 2 ? uint32_t(v) : 0u;
          if constexpr (kEmit)
            if (first_block + n < good_blocks) coef[(first_block + n) * 64] = int16_t(int(c == 0 ? dc0 : c == 1 ? dc1 : dc2));
          k = 1;
        }
      } else {
        const int s = symbol(r, plan->huff[2 + (plan->ta[c & 3] & 1)], &st);
        const int run = s >> 4, size = s & 15;
        if (s < 0) {
          dead = true;
        } else if (size == 0) {
          if (run != 15) {
            ended = true;  // EOB
          } else {
            k += 16;  // ZRL
            if (k > 64) {
              st |= kBadRun;
              dead = true;
            }
            ended = k == 64;
          }
        } else {
          k += run;
          if (k > 63) {
            st |= kBadRun;
            dead = true;
          } else if (!value(r, size, &v, &st)) {
            dead = true;
          } else {
            if constexpr (kEmit)
              if (first_block + n < good_blocks) coef[(first_block + n) * 64 + kZigzag[k]] = int16_t(v);
            ++k;
            ended = k == 64;
          }
        }
      }
      if (ended && !dead) {
        ++n;
        k = 0;
        j = j + 1 == g.bpm ? 0 : j + 1;
      }
      consumed += before - r.nbits;
    }
    if (!dead && consumed < u.bits) {  // not reached: every symbol consumes a bit
      st |= kTruncated;
      dead = true;
    }
  }
  if constexpr (!kEmit) {
    pay->n = uint32_t(n) | uint32_t(st) << 28;
    pay->dc[0] = dc0, pay->dc[1] = dc1, pay->dc[2] = dc2;
  }
  return dead ? kDead : pack_state(consumed - u.bits, j, k);
}

EXPO_HD uint32_t walk(const uint8_t* file, int64_t file_bytes, const uint8_t* planp, const Geometry& g, const Segment& seg,
                      int sub_bytes, const SubBits& u, uint32_t entry, Payload* pay) {
  return walk_or_emit<false>(file, file_bytes, planp, g, seg, sub_bytes, u, entry, pay, 0, nullptr, 0, nullptr);
}
EXPO_HD void emit(const uint8_t* file, int64_t file_bytes, const uint8_t* planp, const Geometry& g, const Segment& seg,
                  int sub_bytes, const SubBits& u, uint32_t entry, int64_t first_block, const uint32_t* pred,
                  int64_t good_blocks, int16_t* coef) {
  walk_or_emit<true>(file, file_bytes, planp, g, seg, sub_bytes, u, entry, nullptr, first_block, pred, good_blocks, coef);
}

// ------------------------------------------------------------------------------------------------------- the workspace
// Behind the launch group's pictures (jpegdec::layout, one after another) every sync picture -- one segment, more than
// one subsequence -- has, each piece rounded up to 16 bytes: in[nsubs] and out[nsubs] (uint32 states), pay[nsubs]
// (Payload), first[nsubs] (first_block, pred[3]: four uint32), edge[2][ceil(nsubs / W)] (the ping-pong boundary words)
// and the picture's results (settled, good_blocks, last: the last subsequence that emits, and a spare word).
constexpr int kGroup = 256;  // W: the subsequences of a settle workgroup
struct SyncLayout {
  int64_t in, out, pay, first, edge, result, end;
};
EXPO_HD int64_t sync_groups(int64_t nsubs) { return (nsubs + kGroup - 1) / kGroup; }
EXPO_HD SyncLayout sync_layout(int64_t base, int64_t nsubs) {
  SyncLayout l;
  l.in = base;
  l.out = l.in + align16(nsubs * 4);
  l.pay = l.out + align16(nsubs * 4);
  l.first = l.pay + nsubs * 16;
  l.edge = l.first + nsubs * 16;
  l.result = l.edge + align16(2 * sync_groups(nsubs) * 4);
  l.end = l.result + 16;
  return l;
}
EXPO_HD bool is_sync(int64_t nsegs, int64_t nsubs) { return nsegs == 1 && nsubs > 1; }

}  // namespace jpegsync
}  // namespace expo
