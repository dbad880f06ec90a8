// jpeg_codec.h -- the serial integer routines of csrc/jpeg_encode.hip, written so that they also
// compile for the host: tools/jpeg_rehearse.cpp runs them under -fsanitize=address,undefined and writes whole files
// with them.  No float, no state: the tables of T.81 Annex K, the 13-bit cosine table, the canonical codes (T.81
// Annex C), the colour conversion, the two 8-point passes, the quantiser, one block's symbol stream, the sizes of the
// file and of the workspace, and the 629-byte header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EXPO_HD __host__ __device__ inline
#else
#define EXPO_HD inline
#endif

namespace expo {
namespace jpeg {

constexpr int kRestart444 = 16;   // MCUs (8 x 8 pixels, 3 blocks) per restart interval: 48 blocks, as in 4:2:0
constexpr int kRestart420 = 8;    // MCUs (16 x 16 pixels, 6 blocks) per restart interval
constexpr int kHeaderBytes = 629; // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
constexpr int kMaxDim = 65535;
constexpr int kBlockBits = 22 + 63 * 26;  // a block's worst case: DC code 11 + 11 bits, 63 x (AC code 16 + 10 bits)
constexpr int kMaxBlocks = 6 * (kRestart420 > kRestart444 / 2 ? kRestart420 : kRestart444 / 2);  // blocks per interval
static_assert(3 * kRestart444 <= kMaxBlocks && 6 * kRestart420 <= kMaxBlocks, "blocks per interval");
static_assert(kRestart444 >= 1 && kRestart444 <= 65535 && kRestart420 >= 1 && kRestart420 <= 65535, "Ri");

// C[u][x] = rint(2^13 k_u cos((2x + 1) u pi / 16)), k_0 = sqrt(1/8), else 1/2 (tests/test_jpeg_host.py holds it to the formula)
constexpr int16_t kCos[64] = {
    2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,   //
    4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,  //
    3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,   //
    3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,  //
    2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,   //
    2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,  //
    1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,   //
    799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};

// T.81 Annex K.1 and K.2, in natural order
constexpr uint8_t kQuantBase[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// the natural index of zigzag position k
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.3 - K.6: BITS (codes of length 1..16) and HUFFVAL; index 0 luma, 1 chroma
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};  // both tables
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// The canonical codes of T.81 Annex C, derived at compile time: word[s] = (length << 16) | code of symbol s, 0 for a
// symbol the table does not hold.  [table][symbol]; DC symbols are the categories 0..11, AC symbols (run << 4) | size.
struct Codes {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};
constexpr Codes make_codes() {
  Codes c{};
  for (int id = 0; id < 2; ++id) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int e = 0; e < kDcBits[id][len - 1]; ++e) c.dc[id][kDcVals[k++]] = (uint32_t(len) << 16) | code++;
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int e = 0; e < kAcBits[id][len - 1]; ++e) c.ac[id][kAcVals[id][k++]] = (uint32_t(len) << 16) | code++;
      code <<= 1;
    }
  }
  return c;
}
constexpr Codes kCodes = make_codes();

EXPO_HD int restart_mcus(int subsampling) { return subsampling == 0 ? kRestart444 : subsampling == 2 ? kRestart420 : -1; }
EXPO_HD int mcu_side(int subsampling) { return subsampling == 0 ? 8 : 16; }
EXPO_HD int mcu_blocks(int subsampling) { return subsampling == 0 ? 3 : 6; }
EXPO_HD bool valid_picture(int h, int w) { return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim; }
EXPO_HD int64_t mcus_x(int w, int subsampling) { return (int64_t(w) + mcu_side(subsampling) - 1) / mcu_side(subsampling); }
EXPO_HD int64_t mcus(int h, int w, int subsampling) { return mcus_x(h, subsampling) * mcus_x(w, subsampling); }
EXPO_HD int64_t intervals(int h, int w, int subsampling) {
  const int ri = restart_mcus(subsampling);
  return (mcus(h, w, subsampling) + ri - 1) / ri;
}
// An interval's largest payload: every block at kBlockBits, padded to a byte, every byte stuffed.
EXPO_HD int64_t interval_bound(int nmcu, int subsampling) { return 2 * ((int64_t(nmcu) * mcu_blocks(subsampling) * kBlockBits + 7) / 8); }
// The largest file: header, every interval at its bound and followed by two bytes (RSTm, or EOI behind the last).
EXPO_HD int64_t file_bound(int h, int w, int subsampling) {
  const int ri = restart_mcus(subsampling);
  const int64_t m = mcus(h, w, subsampling), full = m / ri, rest = m % ri;
  return kHeaderBytes + full * (interval_bound(ri, subsampling) + 2) + (rest ? interval_bound(int(rest), subsampling) + 2 : 0);
}

// One picture's part of the workspace, 16-byte aligned pieces: a record (the file's length), the intervals' stuffed
// payload bytes (uint32 each) and their offsets in the file (int64 each): 16 + 12 bytes per interval, rounded.
struct Layout {
  int64_t rec, counts, offs, end;
};
EXPO_HD int64_t align16(int64_t x) { return (x + 15) & ~int64_t(15); }
EXPO_HD Layout layout(int64_t base, int64_t nint) {
  Layout l;
  l.rec = base;
  l.counts = base + 16;
  l.offs = l.counts + align16(nint * 4);
  l.end = l.offs + align16(nint * 8);
  return l;
}

// Q of table `id` (0 luma, 1 chroma) at natural index k for quality 1..100
EXPO_HD int quant_value(int id, int k, int quality) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int q = (int(kQuantBase[id][k]) * scale + 50) / 100;
  return q < 1 ? 1 : q > 255 ? 255 : q;
}

// sign(f) ((|f| + (Q << 14)) / (Q << 15)) for |f| < 2^27, Q in 1..255.  floor(floor(x / 2^14) / 2Q) = floor(x / 2^15 Q)
// and the low 14 bits of Q << 14 are zero, so the quotient is ((|f| >> 14) + Q) / 2Q: a division of numbers below 2^14.
EXPO_HD int quantise(int32_t f, int q) {
  const uint32_t a = f < 0 ? uint32_t(-f) : uint32_t(f);
  const int v = int(((a >> 14) + uint32_t(q)) / (2u * uint32_t(q)));
  return f < 0 ? -v : v;
}

EXPO_HD void ycc(int r, int g, int b, int* y, int* cb, int* cr) {
  *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// the row pass on eight level-shifted samples: t[u] = (sum_x C[u][x] s[x] + 1024) >> 11, |t| <= 1449
template <typename T>
EXPO_HD void dct_row(const T* s, int stride, T* out) {
  int32_t v[8];
  for (int x = 0; x < 8; ++x) v[x] = s[x * stride];
  for (int u = 0; u < 8; ++u) {
    int32_t acc = 0;
    for (int x = 0; x < 8; ++x) acc += int32_t(kCos[u * 8 + x]) * v[x];
    out[u * stride] = T((acc + 1024) >> 11);
  }
}
// the column pass: f[v] = sum_y C[v][y] t[y], the coefficient times 2^15, |f| < 2^26
template <typename T>
EXPO_HD void dct_col(const T* t, int stride, int32_t* f) {
  int32_t v[8];
  for (int y = 0; y < 8; ++y) v[y] = t[y * stride];
  for (int u = 0; u < 8; ++u) {
    int32_t acc = 0;
    for (int y = 0; y < 8; ++y) acc += int32_t(kCos[u * 8 + y]) * v[y];
    f[u] = acc;
  }
}

// the category of T.81 table F.1: the bits of |v|
EXPO_HD int category(int v) {
  uint32_t a = v < 0 ? uint32_t(-v) : uint32_t(v);
  int n = 0;
  while (a) {
    ++n;
    a >>= 1;
  }
  return n;
}
// the n appended bits of v: v, or v + 2^n - 1 when negative
EXPO_HD uint32_t value_bits(int v, int n) { return uint32_t(v < 0 ? v + (1 << n) - 1 : v) & ((1u << n) - 1u); }

// One block's symbols (T.81 §F.1.2) into `sink.put(bits, n)`, n <= 27, most significant bit first: coef the quantised
// block in natural order (stride between neighbours), pred the DC predictor, dc / ac the tables' words as in Codes.
template <typename T, typename Sink>
EXPO_HD void block_symbols(const T* coef, int stride, int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink) {
  const int diff = int(coef[0]) - pred;
  int n = category(diff);
  uint32_t w = dc[n];
  sink.put(((w & 0xFFFFu) << n) | (n ? value_bits(diff, n) : 0u), int(w >> 16) + n);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = int(coef[int(kZigzag[k]) * stride]);
    if (v == 0) {
      ++run;
      continue;
    }
    while (run >= 16) {
      w = ac[0xF0];
      sink.put(w & 0xFFFFu, int(w >> 16));
      run -= 16;
    }
    n = category(v);
    w = ac[(run << 4) | n];
    sink.put(((w & 0xFFFFu) << n) | value_bits(v, n), int(w >> 16) + n);
    run = 0;
  }
  if (run) {
    w = ac[0x00];
    sink.put(w & 0xFFFFu, int(w >> 16));
  }
}

// The index of the block that holds block b's DC predictor inside an interval (blocks in scan order), -1 for none.
EXPO_HD int dc_pred_block(int b, int subsampling) {
  if (subsampling == 0) return b >= 3 ? b - 3 : -1;
  const int j = b % 6;
  if (j >= 1 && j <= 3) return b - 1;            // Y01, Y10, Y11 after the Y before
  if (j == 0) return b >= 6 ? b - 3 : -1;        // Y00 after the MCU before's Y11
  return b >= 6 ? b - 6 : -1;                    // Cb, Cr
}
// the table (0 luma, 1 chroma) of block b of an interval
EXPO_HD int block_table(int b, int subsampling) { return subsampling == 0 ? (b % 3 != 0) : (b % 6 >= 4); }

// the 629 header bytes of an h x w picture
EXPO_HD void write_header(uint8_t* p, int h, int w, int quality, int subsampling) {
  auto put = [&p](int v) { *p++ = uint8_t(v); };
  auto put16 = [&p](int v) {
    *p++ = uint8_t(v >> 8);
    *p++ = uint8_t(v);
  };
  put16(0xFFD8);
  put16(0xFFE0);
  put16(16);
  put('J'), put('F'), put('I'), put('F'), put(0);
  put16(0x0101);
  put(0);
  put16(1), put16(1);
  put(0), put(0);
  for (int id = 0; id < 2; ++id) {
    put16(0xFFDB);
    put16(67);
    put(id);
    for (int k = 0; k < 64; ++k) put(quant_value(id, kZigzag[k], quality));
  }
  put16(0xFFC0);
  put16(17);
  put(8);
  put16(h), put16(w);
  put(3);
  put(1), put(subsampling == 0 ? 0x11 : 0x22), put(0);
  put(2), put(0x11), put(1);
  put(3), put(0x11), put(1);
  for (int id = 0; id < 2; ++id) {
    put16(0xFFC4);
    put16(31);
    put(id);
    for (int e = 0; e < 16; ++e) put(kDcBits[id][e]);
    for (int e = 0; e < 12; ++e) put(kDcVals[e]);
    put16(0xFFC4);
    put16(181);
    put(0x10 | id);
    for (int e = 0; e < 16; ++e) put(kAcBits[id][e]);
    for (int e = 0; e < 162; ++e) put(kAcVals[id][e]);
  }
  put16(0xFFDD);
  put16(4);
  put16(restart_mcus(subsampling));
  put16(0xFFDA);
  put16(12);
  put(3);
  put(1), put(0x00), put(2), put(0x11), put(3), put(0x11);
  put(0), put(63), put(0);
}

}  // namespace jpeg
}  // namespace expo
