// png_rehearse.cpp -- the integer routines of exposure_amd/csrc/png_deflate.h on the host, without a GPU: a serial
// walk through csrc/png_encode.hip's launches (row types; per segment the filtered bytes, the code, dynamic against
// stored, the packed bits, the sliced CRC-32, the Adler pair; the scan; the gather), every "thread" of a phase in a loop.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/png_rehearse.cpp -o png_rehearse
//   png_rehearse selftest                      the routines against their definitions
//   png_rehearse encode H W FILTER in.rgb out.png   H*W*3 bytes in, the file out (tests/test_png_host.py decodes it)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../exposure_amd/csrc/png_deflate.h"

using namespace expo::png;

namespace {

constexpr int kThreads = 256;

void put_bits(std::vector<uint32_t>& words, uint32_t pos, uint32_t v, int n) {
  if (n <= 0) return;
  const uint64_t x = uint64_t(v) << (pos & 31);
  words.at(pos >> 5) |= uint32_t(x);
  if (uint32_t(x >> 32)) words.at((pos >> 5) + 1) |= uint32_t(x >> 32);
}

uint32_t crc_serial(const uint8_t* p, size_t n) {
  uint32_t reg = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) reg = crc_byte(reg, p[i]);
  return reg ^ 0xFFFFFFFFu;
}

void put_be32(std::vector<uint8_t>& f, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) f.push_back(uint8_t(v >> s));
}
void put_chunk(std::vector<uint8_t>& f, const char* type, const uint8_t* data, int n) {
  put_be32(f, uint32_t(n));
  const size_t at = f.size();
  f.insert(f.end(), type, type + 4);
  f.insert(f.end(), data, data + n);
  put_be32(f, crc_serial(f.data() + at, f.size() - at));
}

struct SegmentOut {
  std::vector<uint8_t> chunk;  // length, type, data, CRC
  uint32_t a, b, len;
  int depth;  // the longest code
};

// one workgroup of png_segment_kernel
SegmentOut encode_segment(const uint8_t* stream, int len, bool final) {
  SegmentOut out;
  uint32_t hist[kSyms] = {0};
  hist[256] = 1;
  uint64_t sum_d = 0, sum_w = 0;
  for (int j = 0; j < len; ++j) {
    ++hist[stream[j]];
    sum_d += stream[j];
    sum_w += uint64_t(len - j) * stream[j];
  }
  out.a = uint32_t((1 + sum_d) % kAdlerMod);
  out.b = uint32_t((len + sum_w) % kAdlerMod);
  out.len = uint32_t(len);
  int sorted_f[kSyms], sorted_len[kSyms], rank_of[kSyms], nsym = 0;
  for (int s = 0; s < kSyms; ++s) {
    if (!hist[s]) continue;
    const uint32_t key = (hist[s] << 9) | uint32_t(s);
    int rank = 0;
    for (int o = 0; o < kSyms; ++o) rank += (hist[o] && ((hist[o] << 9) | uint32_t(o)) < key) ? 1 : 0;
    rank_of[s] = rank;
    sorted_f[rank] = int(hist[s]);
    ++nsym;
  }
  huffman_lengths_limited(sorted_f, sorted_len, nsym);
  int lens[kSyms], count[16] = {0}, first[16];
  for (int s = 0; s < kSyms; ++s) {
    lens[s] = hist[s] ? sorted_len[rank_of[s]] : 0;
    if (lens[s]) ++count[lens[s]];
  }
  out.depth = sorted_len[0];
  // complete: the Kraft sum is exactly 1
  uint64_t kraft = 0;
  for (int s = 0; s < kSyms; ++s)
    if (lens[s]) kraft += uint64_t(1) << (kMaxBits - lens[s]);
  if (kraft != (uint64_t(1) << kMaxBits) || out.depth > kMaxBits) {
    fprintf(stderr, "incomplete or too deep a code: kraft %llu depth %d\n", (unsigned long long)kraft, out.depth);
    exit(1);
  }
  canonical_first_codes(count, first);
  uint32_t codes[kSyms];
  for (int s = 0; s < kSyms; ++s) {
    int code = 0;
    if (lens[s]) {
      code = first[lens[s]];
      for (int o = 0; o < s; ++o) code += lens[o] == lens[s] ? 1 : 0;
    }
    codes[s] = reverse_bits(uint32_t(code), lens[s]);
  }
  uint64_t data_bits = 0;
  for (int j = 0; j < len; ++j) data_bits += lens[stream[j]];
  const int64_t bits = kHeaderBits + int64_t(data_bits) + lens[256];
  const int dyn = dynamic_bytes(bits, final), sto = stored_bytes(len);
  const bool stored = dyn >= sto;
  const int P = stored ? sto : dyn;
  std::vector<uint32_t> obuf(kSlot / 4, 0);
  std::vector<uint8_t> ob8(kSlot, 0);
  if (stored) {
    ob8[8] = final ? 1 : 0;
    ob8[9] = uint8_t(len);
    ob8[10] = uint8_t(len >> 8);
    ob8[11] = uint8_t(~len);
    ob8[12] = uint8_t(~len >> 8);
    memcpy(&ob8[13], stream, size_t(len));
  } else {
    const uint32_t at = 64;
    put_bits(obuf, at, (final ? 1u : 0u) | (2u << 1) | (15u << 13), 17);
    for (int c = 3; c < 19; ++c) put_bits(obuf, at + 17 + 3 * c, 4u, 3);
    put_bits(obuf, at + 74 + 4 * 257, reverse_bits(1u, 4), 4);
    put_bits(obuf, at + kHeaderBits + uint32_t(data_bits), codes[256], lens[256]);
    if (!final) put_bits(obuf, at + 8u * uint32_t(((bits + 3 + 7) >> 3) + 2), 0xFFFFu, 16);
    for (int s = 0; s < kSyms; ++s) put_bits(obuf, at + 74 + 4 * s, reverse_bits(uint32_t(lens[s]), 4), 4);
    // every thread packs its run of kSeg / 256 bytes from its own first bit
    const int run = kSeg / kThreads;
    uint32_t my_first = 0;
    for (int t = 0; t < kThreads; ++t) {
      uint32_t pos = at + kHeaderBits + my_first, wi = pos >> 5;
      int nb = int(pos & 31);
      uint64_t acc = 0;
      for (int j = t * run; j < (t + 1) * run && j < len; ++j) {
        acc |= uint64_t(codes[stream[j]]) << nb;
        nb += lens[stream[j]];
        my_first += uint32_t(lens[stream[j]]);
        if (nb >= 32) {
          obuf.at(wi++) |= uint32_t(acc);
          acc >>= 32;
          nb -= 32;
        }
      }
      if (nb > 0 && uint32_t(acc)) obuf.at(wi) |= uint32_t(acc);
    }
    for (size_t e = 0; e < obuf.size(); ++e)
      for (int k = 0; k < 4; ++k) ob8[4 * e + k] = uint8_t(obuf[e] >> (8 * k));  // little-endian, as the device
  }
  ob8[0] = uint8_t(uint32_t(P) >> 24);
  ob8[1] = uint8_t(uint32_t(P) >> 16);
  ob8[2] = uint8_t(uint32_t(P) >> 8);
  ob8[3] = uint8_t(P);
  memcpy(&ob8[4], "IDAT", 4);
  // the sliced CRC
  const int N = 4 + P, K = (N + kThreads - 1) / kThreads;
  uint32_t pw[8], total = 0;
  for (int b = 0; b < 8; ++b) pw[b] = crc_xpow((8ull * uint64_t(K)) << b);
  for (int t = 0; t < kThreads; ++t) {
    const int start = N - (kThreads - t) * K, end = start + K;
    if (end <= 0) continue;
    uint32_t reg = start <= 0 ? 0xFFFFFFFFu : 0u;
    for (int j = start < 0 ? 0 : start; j < end; ++j) reg = crc_byte(reg, ob8.at(size_t(4 + j)));
    uint32_t m = 0x80000000u;
    for (int bit = 0; bit < 8; ++bit)
      if (((kThreads - 1 - t) >> bit) & 1) m = crc_mul(m, pw[bit]);
    total ^= crc_mul(reg, m);
  }
  const uint32_t crc = total ^ 0xFFFFFFFFu;
  if (crc != crc_serial(&ob8[4], size_t(N))) {
    fprintf(stderr, "sliced CRC differs from the serial one\n");
    exit(1);
  }
  for (int k = 0; k < 4; ++k) ob8[size_t(8 + P + k)] = uint8_t(crc >> (24 - 8 * k));
  out.chunk.assign(ob8.begin(), ob8.begin() + 12 + P);
  return out;
}

std::vector<uint8_t> encode(const uint8_t* pic, int h, int w, int filter, int* depth) {
  const int64_t S = stream_bytes(h, w);
  if (S < 0 || filter < 0 || filter > 5) {
    fprintf(stderr, "bad arguments\n");
    exit(1);
  }
  const int w3 = 3 * w;
  std::vector<uint8_t> stream;
  stream.reserve(size_t(S));
  for (int r = 0; r < h; ++r) {
    const uint8_t* cur = pic + size_t(r) * size_t(w3);
    auto at = [&](int t, int x) {
      const int a = x >= 3 ? cur[x - 3] : 0, up = r ? cur[x - w3] : 0, c = (r && x >= 3) ? cur[x - 3 - w3] : 0;
      return filter_byte(t, cur[x], a, up, c);
    };
    int ty = filter;
    if (filter == 5) {
      uint64_t least = 0;
      for (int t = 0; t < 5; ++t) {
        uint64_t s = 0;
        for (int x = 0; x < w3; ++x) s += uint64_t(filter_cost(at(t, x)));
        if (t == 0 || s < least) {
          least = s;
          ty = t;
        }
      }
    }
    stream.push_back(uint8_t(ty));
    for (int x = 0; x < w3; ++x) stream.push_back(uint8_t(at(ty, x)));
  }
  const int64_t nseg = segments(S);
  std::vector<uint8_t> f = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  uint8_t ihdr[13] = {uint8_t(w >> 24), uint8_t(w >> 16), uint8_t(w >> 8), uint8_t(w), uint8_t(h >> 24), uint8_t(h >> 16),
                      uint8_t(h >> 8), uint8_t(h), 8, 2, 0, 0, 0};
  put_chunk(f, "IHDR", ihdr, 13);
  const uint8_t zhdr[2] = {0x78, 0x01};
  put_chunk(f, "IDAT", zhdr, 2);
  if (int64_t(f.size()) != kFirstIdat) exit(1);
  uint32_t a = 1, b = 0;
  *depth = 0;
  for (int64_t k = 0; k < nseg; ++k) {
    const int len = int(S - k * kSeg < kSeg ? S - k * kSeg : kSeg);
    const SegmentOut seg = encode_segment(stream.data() + k * kSeg, len, k == nseg - 1);
    f.insert(f.end(), seg.chunk.begin(), seg.chunk.end());
    adler_combine(&a, &b, seg.a, seg.b, seg.len);
    *depth = seg.depth > *depth ? seg.depth : *depth;
  }
  // the combined pair against the definition
  uint32_t ra = 1, rb = 0;
  for (uint8_t v : stream) {
    ra = (ra + v) % kAdlerMod;
    rb = (rb + ra) % kAdlerMod;
  }
  if (ra != a || rb != b) {
    fprintf(stderr, "combined Adler-32 differs from the serial one\n");
    exit(1);
  }
  const uint32_t adler = (b << 16) | a;
  const uint8_t ad[4] = {uint8_t(adler >> 24), uint8_t(adler >> 16), uint8_t(adler >> 8), uint8_t(adler)};
  put_chunk(f, "IDAT", ad, 4);
  put_chunk(f, "IEND", ad, 0);
  if (int64_t(f.size()) > file_bound(S)) {
    fprintf(stderr, "file above the bound\n");
    exit(1);
  }
  return f;
}

int selftest() {
  // CRC-32 of "123456789", whole and cut in two at every place
  const uint8_t* m = reinterpret_cast<const uint8_t*>("123456789");
  if (crc_serial(m, 9) != 0xCBF43926u) return 1;
  for (size_t cut = 0; cut <= 9; ++cut) {
    uint32_t ra = 0xFFFFFFFFu, rb = 0;
    for (size_t i = 0; i < cut; ++i) ra = crc_byte(ra, m[i]);
    for (size_t i = cut; i < 9; ++i) rb = crc_byte(rb, m[i]);
    if ((crc_combine_raw(ra, rb, 9 - cut) ^ 0xFFFFFFFFu) != 0xCBF43926u) return 2;
  }
  if (crc_xpow(0) != 0x80000000u || crc_xpow(1) != 0x40000000u || crc_mul(crc_xpow(700), crc_xpow(5)) != crc_xpow(705)) return 3;
  // the bound and the slots
  if (file_bound(stream_bytes(1, 1)) != 75 + 17 + 4 || stream_bytes(0, 1) != -1 || stream_bytes(1, 0) != -1) return 4;
  if (stream_bytes(46341, 15447) != -1 || stream_bytes(3, 21845) != 3 * 65536) return 5;  // 46341 * 46342 >= 2^31
  if (segments(kSeg) != 1 || segments(kSeg + 1) != 2 || kSlot < kSeg + kSegOverhead + 8) return 6;
  const Layout l = layout(16, 5, 3);
  if (l.types != 16 || l.slots != 32 || l.recs != 32 + 3 * kSlot || l.offs != l.recs + 48 || l.end != l.offs + 32) return 7;
  // code lengths: two symbols; Fibonacci counts that go 17 deep without the limit and are held at 15 with it
  int two[2] = {1, 5};
  huffman_lengths_sorted(two, 2);
  if (two[0] != 1 || two[1] != 1) return 8;
  int fib[18] = {1, 1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2207}, deep[18], lim[18];
  for (int i = 0; i < 18; ++i) deep[i] = fib[i];
  huffman_lengths_sorted(deep, 18);
  if (deep[0] != 17) return 9;
  huffman_lengths_limited(fib, lim, 18);
  uint64_t kraft = 0;
  for (int i = 0; i < 18; ++i) kraft += uint64_t(1) << (15 - lim[i]);
  if (lim[0] > 15 || kraft != (uint64_t(1) << 15)) return 10;
  // canonical codes of RFC 1951's example: lengths 3 3 3 3 3 2 4 4 -> 010 011 100 101 110 00 1110 1111
  int count[16] = {0}, first[16];
  count[2] = 1;
  count[3] = 5;
  count[4] = 2;
  canonical_first_codes(count, first);
  if (first[2] != 0 || first[3] != 2 || first[4] != 14 || reverse_bits(6u, 3) != 3u) return 11;
  // Adler-32 of "Wikipedia" = 0x11E60398, cut in two
  const uint8_t* wk = reinterpret_cast<const uint8_t*>("Wikipedia");
  for (int cut = 0; cut <= 9; ++cut) {
    uint32_t a1 = 1, b1 = 0, a2 = 1, b2 = 0;
    for (int i = 0; i < cut; ++i) b1 = (b1 + (a1 = (a1 + wk[i]) % kAdlerMod)) % kAdlerMod;
    for (int i = cut; i < 9; ++i) b2 = (b2 + (a2 = (a2 + wk[i]) % kAdlerMod)) % kAdlerMod;
    adler_combine(&a1, &b1, a2, b2, uint32_t(9 - cut));
    if (((b1 << 16) | a1) != 0x11E60398u) return 12;
  }
  // whole files of noise, of one value and of the deep counts: the checks inside encode()
  int depth = 0;
  std::vector<uint8_t> pic(size_t(33) * 341 * 3);
  uint32_t x = 12345;
  for (auto& v : pic) v = uint8_t((x = x * 1664525u + 1013904223u) >> 24);
  for (int filter = 0; filter <= 5; ++filter) {
    const std::vector<uint8_t> f = encode(pic.data(), 33, 341, filter, &depth);
    if (filter == 0 && int64_t(f.size()) != file_bound(stream_bytes(33, 341))) return 13;  // noise: every segment stored
  }
  std::vector<uint8_t> zeros(size_t(64) * 64 * 3, 0);
  encode(zeros.data(), 64, 64, 5, &depth);
  if (depth != 1) return 14;
  std::vector<uint8_t> deepest;
  const int counts[17] = {1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2206};
  for (int v = 16; v >= 0; --v) deepest.insert(deepest.end(), size_t(counts[16 - v]), uint8_t(v));
  if (deepest.size() != 1925 * 3) return 15;
  encode(deepest.data(), 1, 1925, 0, &depth);
  if (depth > 15) return 16;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) {
    const int rc = selftest();
    printf(rc ? "selftest FAILED at %d\n" : "selftest OK\n", rc);
    return rc;
  }
  if (argc == 7 && !strcmp(argv[1], "encode")) {
    const int h = atoi(argv[2]), w = atoi(argv[3]), filter = atoi(argv[4]);
    if (stream_bytes(h, w) < 0) return 2;
    std::vector<uint8_t> pic(size_t(h) * size_t(w) * 3);
    FILE* in = fopen(argv[5], "rb");
    if (!in || fread(pic.data(), 1, pic.size(), in) != pic.size()) return 2;
    fclose(in);
    int depth = 0;
    const std::vector<uint8_t> f = encode(pic.data(), h, w, filter, &depth);
    FILE* out = fopen(argv[6], "wb");
    if (!out || fwrite(f.data(), 1, f.size(), out) != f.size()) return 2;
    fclose(out);
    printf("%zu bytes, longest code %d\n", f.size(), depth);
    return 0;
  }
  fprintf(stderr, "usage: png_rehearse selftest | encode H W FILTER in.rgb out.png\n");
  return 2;
}
