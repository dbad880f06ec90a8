// png_deflate.h -- the serial integer routines of csrc/png_encode.hip, written so that they also
// compile for the host: tools/png_rehearse.cpp runs them under -fsanitize=address,undefined and writes whole files
// with them.  No float, no state: sizes of the file and of the workspace, the filters of the PNG specification,
// Huffman code lengths and their limit, canonical codes (RFC 1951 §3.2.2), Adler-32 and CRC-32 combination.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EXPO_HD __host__ __device__ inline
#else
#define EXPO_HD inline
#endif

namespace expo {
namespace png {

constexpr int kSeg = 16384;            // stream bytes per deflate segment (16384 <= SEG <= 65535: a stored block's LEN)
constexpr int kSyms = 257;             // the 256 byte values and end-of-block
constexpr int kMaxBits = 15;           // deflate's longest code
constexpr int kHeaderBits = 1106;      // 3 + 14 + 19 * 3 + 258 * 4: the dynamic block's header, always
constexpr int kFixedBytes = 75;        // signature 8, IHDR 25, zlib header IDAT 14, Adler IDAT 16, IEND 12
constexpr int kSegOverhead = 17;       // IDAT length, type and CRC 12, the stored block's 5
constexpr int kFirstIdat = 47;         // file offset of the first segment's chunk
constexpr int kSlot = kSeg + 32;       // a segment's chunk in the workspace: at most SEG + 17 bytes, then read slack
constexpr uint32_t kAdlerMod = 65521u;
constexpr uint32_t kCrcPoly = 0xEDB88320u;  // CRC-32, reflected
static_assert(kSeg >= 16384 && kSeg <= 65535 && kSeg % 1024 == 0, "SEG");

// S = h * (1 + 3 w), the filtered stream; -1 when h or w is below 1 or S >= 2^31
EXPO_HD int64_t stream_bytes(int h, int w) {
  if (h < 1 || w < 1) return -1;
  const int64_t s = int64_t(h) * (1 + 3 * int64_t(w));
  return s < (int64_t(1) << 31) ? s : -1;
}
EXPO_HD int64_t segments(int64_t s) { return (s + kSeg - 1) / kSeg; }
// the largest file: every segment stored
EXPO_HD int64_t file_bound(int64_t s) { return kFixedBytes + kSegOverhead * segments(s) + s; }

// One image's part of the workspace, 16-byte aligned pieces: the row types, a slot per segment (the finished IDAT
// chunk), a record per segment (chunk bytes, Adler A, Adler B, stream bytes) and the chunk's offset in the file.
struct Layout {
  int64_t types, slots, recs, offs, end;
};
EXPO_HD int64_t align16(int64_t x) { return (x + 15) & ~int64_t(15); }
EXPO_HD Layout layout(int64_t base, int h, int64_t nseg) {
  Layout l;
  l.types = base;
  l.slots = l.types + align16(h);
  l.recs = l.slots + nseg * kSlot;
  l.offs = l.recs + nseg * 16;
  l.end = l.offs + align16(nseg * 8);
  return l;
}

EXPO_HD int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// the filtered byte of type t (0 None 1 Sub 2 Up 3 Average 4 Paeth): x the byte, a left, b above, c above left
EXPO_HD int filter_byte(int t, int x, int a, int b, int c) {
  const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : paeth(a, b, c);
  return (x - pred) & 255;
}
// libpng's heuristic: a filtered byte counts as its distance from zero
EXPO_HD int filter_cost(int v) { return v < 128 ? v : 256 - v; }

// Code lengths of a minimum-redundancy code, in place (Moffat and Katajainen 1995): a[0..n) holds the frequencies in
// non-decreasing order, all positive, n >= 2; on return a[i] is the length of symbol i's code, non-increasing.
EXPO_HD void huffman_lengths_sorted(int* a, int n) {
  a[0] += a[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < n - 1; ++next) {
    if (leaf >= n || a[root] < a[leaf]) {
      a[next] = a[root];
      a[root++] = next;
    } else {
      a[next] = a[leaf++];
    }
    if (leaf >= n || (root < next && a[root] < a[leaf])) {
      a[next] += a[root];
      a[root++] = next;
    } else {
      a[next] += a[leaf++];
    }
  }
  a[n - 2] = 0;
  for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
  int avbl = 1, used = 0, dpth = 0;
  root = n - 2;
  int next = n - 1;
  while (avbl > 0) {
    while (root >= 0 && a[root] == dpth) {
      ++used;
      --root;
    }
    while (avbl > used) {
      a[next--] = dpth;
      --avbl;
    }
    avbl = 2 * used;
    ++dpth;
    used = 0;
  }
}
// The same with the length limit: f[0..n) sorted frequencies (changed: halved, rounding up, while the code is deeper
// than kMaxBits), len[0..n) the lengths.  A complete code whatever the limit did: every pass is a Huffman code.
EXPO_HD void huffman_lengths_limited(int* f, int* len, int n) {
  for (;;) {
    for (int i = 0; i < n; ++i) len[i] = f[i];
    huffman_lengths_sorted(len, n);
    if (len[0] <= kMaxBits) return;
    for (int i = 0; i < n; ++i) f[i] = (f[i] + 1) >> 1;
  }
}

// RFC 1951 §3.2.2: the first code of every length from the count of codes per length
EXPO_HD void canonical_first_codes(const int* count /*[16]*/, int* first /*[16]*/) {
  int code = 0;
  first[0] = 0;
  for (int b = 1; b <= kMaxBits; ++b) {
    code = (code + (b == 1 ? 0 : count[b - 1])) << 1;
    first[b] = code;
  }
}
// deflate sends Huffman codes from their most significant bit, everything else from the least
EXPO_HD uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// bytes of one segment's deflate data: the dynamic form with B = 1106 + sum f l bits, the stored form, and the rule
EXPO_HD int dynamic_bytes(int64_t bits, bool final) { return final ? int((bits + 7) >> 3) : int((bits + 3 + 7) >> 3) + 4; }
EXPO_HD int stored_bytes(int len) { return 5 + len; }

// Adler-32 of a concatenation: (A1, B1) then (A2, B2) over len2 bytes, everything below 65521
EXPO_HD void adler_combine(uint32_t* a1, uint32_t* b1, uint32_t a2, uint32_t b2, uint32_t len2) {
  const uint32_t am1 = (*a1 + kAdlerMod - 1) % kAdlerMod;
  *b1 = uint32_t((uint64_t(*b1) + b2 + uint64_t(len2 % kAdlerMod) * am1) % kAdlerMod);
  *a1 = (am1 + a2) % kAdlerMod;
}

// CRC-32 as polynomials over GF(2) modulo P, reflected: bit 31 is x^0.  a * b mod P.
EXPO_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; --i) {
    p ^= ((a >> i) & 1u) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
  }
  return p;
}
// x^n mod P
EXPO_HD uint32_t crc_xpow(uint64_t n) {
  uint32_t r = 0x80000000u, base = 0x40000000u;
  for (; n; n >>= 1) {
    if (n & 1) r = crc_mul(r, base);
    base = crc_mul(base, base);
  }
  return r;
}
EXPO_HD uint32_t crc_table_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1u) ? kCrcPoly : 0u);
  return i;
}
// the register after one more byte (no table: the few bytes of the small chunks)
EXPO_HD uint32_t crc_byte(uint32_t reg, uint32_t byte) { return (reg >> 8) ^ crc_table_entry((reg ^ byte) & 255u); }
// The register of a message cut in two: reg_ab = reg_a * x^(8 len_b) + reg_b, with reg_b started from 0.
EXPO_HD uint32_t crc_combine_raw(uint32_t reg_a, uint32_t reg_b, uint64_t len_b) {
  return crc_mul(reg_a, crc_xpow(8 * len_b)) ^ reg_b;
}

}  // namespace png
}  // namespace expo
