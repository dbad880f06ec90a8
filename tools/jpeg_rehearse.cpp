// jpeg_rehearse.cpp -- the integer routines of exposure_amd/csrc/jpeg_codec.h on the host, without a GPU: a serial
// walk through the phases of csrc/jpeg_encode.hip's kernels, "thread" by "thread", into whole files.  Its own main; build
// it with the sanitizers and run it directly:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/jpeg_rehearse.cpp -o jpeg_rehearse
//   jpeg_rehearse selftest                              the routines against their definitions
//   jpeg_rehearse encode H W QUALITY SUB in.rgb out.jpg   H*W*3 bytes in, the file out (tests/test_jpeg_host.py decodes
//                                                       it and compares it with the NumPy restatement byte for byte)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../exposure_amd/csrc/jpeg_codec.h"

using namespace expo::jpeg;

namespace {

constexpr int kLanes = 64;  // the interval kernel's workgroup: one wave

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

struct CountSink {
  uint32_t bits = 0;
  void put(uint32_t, int n) { bits += uint32_t(n); }
};
// the kernel's PackSink: OR into zeroed words, most significant bit first
struct PackSink {
  std::vector<uint32_t>* words;
  uint32_t pos;
  void put(uint32_t v, int n) {
    CHECK(n >= 1 && n <= 27 && (n == 32 || (v >> n) == 0));
    const uint64_t x = uint64_t(v) << (64 - n - int(pos & 31));
    words->at(pos >> 5) |= uint32_t(x >> 32);
    if (uint32_t(x)) words->at((pos >> 5) + 1) |= uint32_t(x);
    pos += uint32_t(n);
  }
};
uint32_t packed_byte(const std::vector<uint32_t>& words, int j) { return (words.at(j >> 2) >> (24 - 8 * (j & 3))) & 255u; }

// one interval as jpeg_interval_kernel computes it: the stuffed payload
std::vector<uint8_t> encode_interval(const uint8_t* pic, int h, int w, int quality, int sub, int k) {
  const int ri = restart_mcus(sub), bpm = mcu_blocks(sub);
  const int mx = int(mcus_x(w, sub)), nmcu_all = mx * int(mcus_x(h, sub));
  const int m_first = k * ri, nm = nmcu_all - m_first < ri ? nmcu_all - m_first : ri, nblk = nm * bpm;
  std::vector<int16_t> blk(size_t(ri) * bpm * 64, 0x7FFF);
  uint8_t qtab[2][64];
  for (int s = 0; s < 128; ++s) qtab[s >> 6][s & 63] = uint8_t(quant_value(s >> 6, s & 63, quality));
  for (int p = 0; p < nm * 64; ++p) {  // "thread" p % 64, pass p / 64
    const int m = p >> 6, yy = (p >> 3) & 7, xx = p & 7;
    const int g = m_first + m, my = g / mx, mxi = g - my * mx;
    if (sub == 0) {
      const int gy = my * 8 + yy < h - 1 ? my * 8 + yy : h - 1, gx = mxi * 8 + xx < w - 1 ? mxi * 8 + xx : w - 1;
      const uint8_t* px = pic + (size_t(gy) * size_t(w) + size_t(gx)) * 3;
      int y, cb, cr;
      ycc(px[0], px[1], px[2], &y, &cb, &cr);
      blk.at((m * 3 + 0) * 64 + yy * 8 + xx) = int16_t(y - 128);
      blk.at((m * 3 + 1) * 64 + yy * 8 + xx) = int16_t(cb - 128);
      blk.at((m * 3 + 2) * 64 + yy * 8 + xx) = int16_t(cr - 128);
    } else {
      int sb = 0, sr = 0;
      for (int d = 0; d < 4; ++d) {
        const int py = 2 * yy + (d >> 1), qx = 2 * xx + (d & 1);
        const int gy = my * 16 + py < h - 1 ? my * 16 + py : h - 1, gx = mxi * 16 + qx < w - 1 ? mxi * 16 + qx : w - 1;
        const uint8_t* px = pic + (size_t(gy) * size_t(w) + size_t(gx)) * 3;
        int y, cb, cr;
        ycc(px[0], px[1], px[2], &y, &cb, &cr);
        CHECK(y >= 0 && y <= 255 && cb >= 0 && cb <= 255 && cr >= 0 && cr <= 255);
        blk.at((m * 6 + (py >> 3) * 2 + (qx >> 3)) * 64 + (py & 7) * 8 + (qx & 7)) = int16_t(y - 128);
        sb += cb;
        sr += cr;
      }
      blk.at((m * 6 + 4) * 64 + yy * 8 + xx) = int16_t(((sb + 2) >> 2) - 128);
      blk.at((m * 6 + 5) * 64 + yy * 8 + xx) = int16_t(((sr + 2) >> 2) - 128);
    }
  }
  for (int r = 0; r < nblk * 8; ++r) {
    dct_row(&blk.at(r * 8), 1, &blk.at(r * 8));
    for (int u = 0; u < 8; ++u) CHECK(abs(blk[r * 8 + u]) <= 1449);
  }
  for (int c = 0; c < nblk * 8; ++c) {
    const int bl = c >> 3, u = c & 7;
    int32_t f[8];
    dct_col(&blk.at(bl * 64 + u), 8, f);
    const uint8_t* q = qtab[block_table(bl, sub)];
    for (int v = 0; v < 8; ++v) {
      CHECK(abs(f[v]) < (1 << 27));
      const int c16 = quantise(f[v], q[v * 8 + u]);
      CHECK(abs(c16) <= ((u | v) ? 1023 : 2047));
      blk.at(bl * 64 + v * 8 + u) = int16_t(c16);
    }
  }
  std::vector<uint32_t> my_bits(kLanes, 0), upto(kLanes, 0);
  std::vector<int> pred(kLanes, 0), id(kLanes, 0);
  CHECK(nblk <= kLanes);
  for (int t = 0; t < nblk; ++t) {
    const int pb = dc_pred_block(t, sub);
    pred[t] = pb >= 0 ? int(blk.at(pb * 64)) : 0;
    id[t] = block_table(t, sub);
    CountSink cs;
    block_symbols(&blk.at(t * 64), 1, pred[t], kCodes.dc[id[t]], kCodes.ac[id[t]], cs);
    CHECK(cs.bits <= uint32_t(kBlockBits));
    my_bits[t] = cs.bits;
  }
  uint32_t all_bits = 0;
  for (int t = 0; t < kLanes; ++t) upto[t] = all_bits += my_bits[t];
  const int nbytes = int((all_bits + 7) >> 3);
  const int bit_words = (ri * bpm * kBlockBits + 31) / 32 + 2;  // the kernel's LDS array
  CHECK((nbytes + 3) / 4 + 1 <= bit_words);
  std::vector<uint32_t> bits(size_t((nbytes + 3) / 4 + 1), 0);
  for (int t = 0; t < nblk; ++t) {
    PackSink ps = {&bits, upto[t] - my_bits[t]};
    block_symbols(&blk.at(t * 64), 1, pred[t], kCodes.dc[id[t]], kCodes.ac[id[t]], ps);
    CHECK(ps.pos == upto[t]);
  }
  if (all_bits & 7) {
    PackSink ps = {&bits, all_bits};
    const int npad = 8 - int(all_bits & 7);
    ps.put((1u << npad) - 1u, npad);
  }
  const int per = (nbytes + kLanes - 1) / kLanes;
  std::vector<uint32_t> ff(kLanes, 0), ff_upto(kLanes, 0);
  uint32_t all_ff = 0;
  for (int t = 0; t < kLanes; ++t) {
    const int j0 = t * per < nbytes ? t * per : nbytes, j1 = j0 + per < nbytes ? j0 + per : nbytes;
    for (int j = j0; j < j1; ++j) ff[t] += packed_byte(bits, j) == 255u;
    ff_upto[t] = all_ff += ff[t];
  }
  std::vector<uint8_t> out(size_t(nbytes) + all_ff, 0xA5);
  CHECK(int64_t(out.size()) <= interval_bound(nm, sub));
  for (int t = 0; t < kLanes; ++t) {
    const int j0 = t * per < nbytes ? t * per : nbytes, j1 = j0 + per < nbytes ? j0 + per : nbytes;
    size_t o = size_t(j0) + (ff_upto[t] - ff[t]);
    for (int j = j0; j < j1; ++j) {
      const uint32_t v = packed_byte(bits, j);
      out.at(o++) = uint8_t(v);
      if (v == 255u) out.at(o++) = 0;
    }
  }
  return out;
}

// the three launches: counts, the scan, the writes
std::vector<uint8_t> encode_file(const uint8_t* pic, int h, int w, int quality, int sub) {
  const int nint = int(intervals(h, w, sub));
  std::vector<int64_t> offs(nint);
  int64_t at = kHeaderBytes;
  for (int k = 0; k < nint; ++k) {
    offs[k] = at;
    at += int64_t(encode_interval(pic, h, w, quality, sub, k).size()) + 2;
  }
  CHECK(at <= file_bound(h, w, sub));
  std::vector<uint8_t> file(size_t(at), 0xA5);
  std::vector<uint8_t> written(size_t(at), 0);
  for (int k = 0; k < nint; ++k) {
    const std::vector<uint8_t> data = encode_interval(pic, h, w, quality, sub, k);
    for (size_t e = 0; e < data.size(); ++e) file.at(offs[k] + e) = data[e], ++written.at(offs[k] + e);
    file.at(offs[k] + data.size()) = 0xFF, ++written.at(offs[k] + data.size());
    file.at(offs[k] + data.size() + 1) = k == nint - 1 ? 0xD9 : uint8_t(0xD0 + (k & 7)), ++written.at(offs[k] + data.size() + 1);
  }
  uint8_t header[640];
  memset(header, 0xA5, sizeof(header));
  write_header(header, h, w, quality, sub);
  CHECK(header[kHeaderBytes - 1] == 0 && header[kHeaderBytes] == 0xA5);
  for (int e = 0; e < kHeaderBytes; ++e) file.at(e) = header[e], ++written.at(e);
  for (size_t e = 0; e < written.size(); ++e) CHECK(written[e] == 1);  // every byte once
  return file;
}

int selftest() {
  // the cosine table against its formula
  const double pi = acos(-1.0);
  int most = 0;
  for (int u = 0; u < 8; ++u) {
    int row = 0;
    for (int x = 0; x < 8; ++x) {
      const double k = u == 0 ? sqrt(1.0 / 8.0) : 0.5;
      CHECK(kCos[u * 8 + x] == int(rint(8192.0 * k * cos((2 * x + 1) * u * pi / 16.0))));
      row += abs(kCos[u * 8 + x]);
    }
    most = row > most ? row : most;
  }
  // int32: |sum| <= 128 * 23168 < 2^22, |t| <= 1449, |f| <= 1449 * 23168 < 2^26
  CHECK(most == 23168 && ((128 * most + 1024) >> 11) <= 1449 && int64_t(1449) * most < (int64_t(1) << 26));
  // zigzag: a permutation that walks the anti-diagonals
  int seen[64] = {0};
  for (int k = 0; k < 64; ++k) ++seen[kZigzag[k]];
  for (int k = 0; k < 64; ++k) CHECK(seen[k] == 1);
  for (int k = 1; k < 64; ++k) {
    const int a = kZigzag[k - 1], b = kZigzag[k];
    CHECK((b / 8 + b % 8) - (a / 8 + a % 8) == 0 || (b / 8 + b % 8) - (a / 8 + a % 8) == 1);
  }
  // the canonical codes: every listed symbol once, prefix-free (Kraft sum below 1: the all-ones code stays free)
  for (int id = 0; id < 2; ++id) {
    int ndc = 0, nac = 0;
    uint64_t kraft_dc = 0, kraft_ac = 0;
    for (int s = 0; s < 12; ++s)
      if (kCodes.dc[id][s]) ++ndc, kraft_dc += uint64_t(1) << (16 - (kCodes.dc[id][s] >> 16));
    for (int s = 0; s < 256; ++s)
      if (kCodes.ac[id][s]) {
        ++nac, kraft_ac += uint64_t(1) << (16 - (kCodes.ac[id][s] >> 16));
        CHECK((s & 15) <= 10 && ((s & 15) != 0 || s == 0x00 || s == 0xF0));
      }
    CHECK(ndc == 12 && nac == 162 && kraft_dc < 65536 && kraft_ac < 65536);
    for (int a = 0; a < 256; ++a)
      for (int b = 0; b < 256; ++b) {
        const uint32_t wa = kCodes.ac[id][a], wb = kCodes.ac[id][b];
        if (!wa || !wb || a == b) continue;
        const int la = int(wa >> 16), lb = int(wb >> 16);
        if (la <= lb) CHECK(((wb & 0xFFFF) >> (lb - la)) != (wa & 0xFFFF));
      }
    CHECK((kCodes.dc[id][11] >> 16) + 11 <= 22 && (kCodes.ac[id][0xFA] >> 16) == 16);
  }
  CHECK(kCodes.dc[0][0] == ((2u << 16) | 0u) && kCodes.ac[0][0x00] == ((4u << 16) | 0xAu) && kCodes.ac[0][0xF0] == ((11u << 16) | 0x7F9u));
  // the quantiser against its definition: per Q a strided set of |f| < 2^27 and every quotient boundary
  for (int q = 1; q <= 255; ++q) {
    const int64_t d = int64_t(q) << 15, half = int64_t(q) << 14;
    for (int64_t f = 0; f < (int64_t(1) << 27); f += 4093) {
      CHECK(quantise(int32_t(f), q) == int((f + half) / d));
      CHECK(quantise(int32_t(-f), q) == -int((f + half) / d));
    }
    for (int64_t n = 0; n * d + half - 1 < (int64_t(1) << 27); ++n)
      for (int64_t f = n * d + half - 1; f <= n * d + half + 1; ++f)
        if (f >= 0 && f < (int64_t(1) << 27)) {
          CHECK(quantise(int32_t(f), q) == int((f + half) / d));
          CHECK(quantise(int32_t(-f), q) == -int((f + half) / d));
        }
  }
  // quality scaling, categories and appended bits
  CHECK(quant_value(0, 0, 50) == 16 && quant_value(0, 0, 100) == 1 && quant_value(1, 63, 1) == 255 && quant_value(0, 0, 75) == 8);
  for (int v = -2047; v <= 2047; ++v) {
    const int n = category(v);
    CHECK(n <= 11 && (v == 0 ? n == 0 : (abs(v) >> (n - 1)) == 1));
    if (n) CHECK(value_bits(v, n) == uint32_t(v < 0 ? v + (1 << n) - 1 : v) && (value_bits(v, n) >> (n - 1)) == uint32_t(v > 0));
  }
  // sizes: the bound grows with the picture and covers a file of worst-case intervals; the workspace layout
  CHECK(file_bound(1, 1, 0) == kHeaderBytes + 2 * ((3 * kBlockBits + 7) / 8) + 2);
  CHECK(file_bound(16, 16, 2) == kHeaderBytes + 2 * ((6 * kBlockBits + 7) / 8) + 2);
  CHECK(file_bound(65535, 65535, 0) > int64_t(65535) * 65535 * 3 && file_bound(65535, 65535, 2) > 0);
  CHECK(intervals(16, 16 * (9 * kRestart420 + 1), 2) == 10 && intervals(8, 8, 0) == 1 && intervals(65535, 65535, 0) == 8192 * 8192 / kRestart444);
  const Layout l = layout(32, 5);
  CHECK(l.rec == 32 && l.counts == 48 && l.offs == 48 + 32 && l.end == 48 + 32 + 48);
  // DC predictors inside an interval
  CHECK(dc_pred_block(0, 0) == -1 && dc_pred_block(4, 0) == 1 && dc_pred_block(0, 2) == -1 && dc_pred_block(6, 2) == 3 &&
        dc_pred_block(7, 2) == 6 && dc_pred_block(10, 2) == 4 && dc_pred_block(5, 2) == -1 && dc_pred_block(11, 2) == 5);
  // whole files of the test shapes: every byte written once, within the bound (encode_file checks)
  const int shapes[][2] = {{1, 1}, {7, 9}, {8, 8}, {16, 16}, {17, 33}, {64, 64}, {16, 16 * (9 * 8 + 1)}};
  uint32_t rnd = 12345;
  for (const auto& s : shapes)
    for (int content = 0; content < 3; ++content)
      for (int sub = 0; sub <= 2; sub += 2) {
        std::vector<uint8_t> pic(size_t(s[0]) * s[1] * 3);
        for (size_t e = 0; e < pic.size(); ++e) {
          rnd = rnd * 1664525u + 1013904223u;
          const int x = int(e / 3) % s[1], y = int(e / 3) / s[1];
          pic[e] = content == 0 ? uint8_t(rnd >> 24) : content == 1 ? uint8_t(((x + y) & 1) == int(e % 3 == 1) ? 0 : 255) : uint8_t(x + 2 * y);
        }
        for (int quality : {1, 50, 100}) {
          const std::vector<uint8_t> file = encode_file(pic.data(), s[0], s[1], quality, sub);
          CHECK(file.size() > size_t(kHeaderBytes) && file[0] == 0xFF && file[1] == 0xD8 && file[file.size() - 1] == 0xD9);
        }
      }
  printf("jpeg_rehearse selftest: ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc == 8 && !strcmp(argv[1], "encode")) {
    const int h = atoi(argv[2]), w = atoi(argv[3]), quality = atoi(argv[4]), sub = atoi(argv[5]);
    if (!valid_picture(h, w) || quality < 1 || quality > 100 || restart_mcus(sub) < 0) {
      fprintf(stderr, "h, w in 1..65535, quality in 1..100 and sub 0 or 2 required\n");
      return 2;
    }
    std::vector<uint8_t> pic(size_t(h) * w * 3);
    FILE* in = fopen(argv[6], "rb");
    if (!in || fread(pic.data(), 1, pic.size(), in) != pic.size()) {
      fprintf(stderr, "cannot read %zu bytes from %s\n", pic.size(), argv[6]);
      return 2;
    }
    fclose(in);
    const std::vector<uint8_t> file = encode_file(pic.data(), h, w, quality, sub);
    FILE* out = fopen(argv[7], "wb");
    if (!out || fwrite(file.data(), 1, file.size(), out) != file.size()) {
      fprintf(stderr, "cannot write %s\n", argv[7]);
      return 2;
    }
    fclose(out);
    printf("%zu\n", file.size());
    return 0;
  }
  fprintf(stderr, "usage: jpeg_rehearse selftest | encode H W QUALITY SUB in.rgb out.jpg\n");
  return 2;
}
