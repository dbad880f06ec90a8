// jpeg_decode.h -- the serial integer routines of csrc/jpeg_decode.hip, written so that they also
// compile for the host: tools/jpeg_decode_rehearse.cpp runs them under -fsanitize=address,undefined over whole files.
// No float, no state: the geometry of a picture and of its workspace, the layout of the plan, the bit reader with
// FF 00 unstuffing, one block's symbol walk (T.81 §F.2.2), libjpeg's "islow" 8-point pass with 13-bit constants, the
// taps of the triangle-filter chroma upsampling and the colour expressions.
//
// The plan of a picture (a device blob the host parser builds; expo_jpeg_decode_plan_bytes(nsegs) bytes, little endian):
//   0     int32 ri            MCUs per restart interval, 0 for a file without DRI
//   4     uint8 tq[4]         per component (Y, Cb, Cr, -) its quantiser table 0..3
//   8     uint8 td[4]         per component its DC Huffman table 0..1
//   12    uint8 ta[4]         per component its AC Huffman table 0..1
//   16    uint8 q[4][64]      the quantiser tables in natural (row-major) order
//   272   Huff huff[4]        DC 0, DC 1, AC 0, AC 1; per table
//           uint32 limit[16]    limit[l - 1] = (MAXCODE(l) + 1) << (16 - l), T.81 Annex C's codes of length l left-aligned
//                               in 16 bits; for a length without codes the limit of the length before (0 before the
//                               first), so a 16-bit window w has the first length l with w < limit[l - 1]
//           int32  offs[16]     offs[l - 1] = VALPTR(l) - MINCODE(l)
//           uint8  vals[256]    HUFFVAL
//   1808  int32 seg[nsegs][2] the byte range [begin, end) of every restart interval's stuffed bytes in the file
// The kernels trust none of it for addressing: table numbers are masked, the symbol index is masked to 0..255, byte
// ranges are clamped to the file, ri to the picture's MCUs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_codec.h"  // EXPO_HD, kZigzag, align16

namespace expo {
namespace jpegdec {

using jpeg::align16;
using jpeg::kZigzag;

constexpr int kMaxDim = 65535;
constexpr int kTruncated = 1;  // a segment consumed more bits than it has
constexpr int kBadCode = 2;    // 16 bits matched no code (or a DC category above 15)
constexpr int kBadRun = 4;     // a run stepped past coefficient 63

struct PlanHuff {
  uint32_t limit[16];
  int32_t offs[16];
  uint8_t vals[256];
};
struct PlanHead {
  int32_t ri;
  uint8_t tq[4], td[4], ta[4];
  uint8_t q[4][64];
  PlanHuff huff[4];
};
static_assert(sizeof(PlanHuff) == 384 && sizeof(PlanHead) == 1808 && sizeof(PlanHead) % 16 == 0, "the plan's layout");

EXPO_HD int64_t plan_bytes(int64_t nsegs) { return int64_t(sizeof(PlanHead)) + align16(nsegs * 8); }

// ---------------------------------------------------------------------------------------------------- geometry
// sampling: PIL's numbers, 0 = 4:4:4 (Y 1 x 1), 1 = 4:2:2 (Y 2 x 1), 2 = 4:2:0 (Y 2 x 2); ncomp 1 (grey, 1 x 1) or 3
EXPO_HD bool valid_picture(int h, int w, int sampling, int ncomp) {
  return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim && sampling >= 0 && sampling <= 2 &&
         (ncomp == 3 || (ncomp == 1 && sampling == 0));
}
struct Geometry {
  int hs, vs;       // Y's sampling factors
  int bpm;          // blocks per MCU
  int mx, my;       // MCUs across and down
  int h, w, ncomp;
};
EXPO_HD Geometry geometry(int h, int w, int sampling, int ncomp) {
  Geometry g;
  g.hs = sampling == 0 ? 1 : 2;
  g.vs = sampling == 2 ? 2 : 1;
  g.bpm = ncomp == 1 ? 1 : g.hs * g.vs + 2;
  g.mx = (w + 8 * g.hs - 1) / (8 * g.hs);
  g.my = (h + 8 * g.vs - 1) / (8 * g.vs);
  g.h = h, g.w = w, g.ncomp = ncomp;
  return g;
}
EXPO_HD int64_t mcus(const Geometry& g) { return int64_t(g.mx) * g.my; }
EXPO_HD int64_t blocks(const Geometry& g) { return mcus(g) * g.bpm; }
// the real samples of component c and the stride of its plane (whole blocks across, so a block's row is 8-byte aligned)
EXPO_HD int plane_h(const Geometry& g, int c) { return c == 0 ? g.h : (g.h + g.vs - 1) / g.vs; }
EXPO_HD int plane_w(const Geometry& g, int c) { return c == 0 ? g.w : (g.w + g.hs - 1) / g.hs; }
EXPO_HD int plane_stride(const Geometry& g, int c) { return (plane_w(g, c) + 7) / 8 * 8; }
// nsegs of a file with restart interval ri (0: none)
EXPO_HD int64_t segments(const Geometry& g, int ri) { return ri > 0 ? (mcus(g) + ri - 1) / ri : 1; }
// is nsegs = ceil(mcus / Ri) for some Ri >= 1?
EXPO_HD bool valid_segments(const Geometry& g, int64_t nsegs) {
  const int64_t m = mcus(g);
  if (nsegs < 1 || nsegs > m) return false;
  const int64_t ri = (m + nsegs - 1) / nsegs;
  return (m + ri - 1) / ri == nsegs;
}

// One picture's part of the workspace, 16-byte aligned pieces: the coefficients (int16, 64 per block in natural order,
// the blocks in scan order) and the component planes (uint8, plane_h rows of plane_stride bytes).
struct Layout {
  int64_t coef, plane[3], end;
};
EXPO_HD Layout layout(int64_t base, const Geometry& g) {
  Layout l;
  l.coef = base;
  int64_t at = base + blocks(g) * 128;
  for (int c = 0; c < 3; ++c) {
    l.plane[c] = at;
    if (c < g.ncomp) at += align16(int64_t(plane_h(g, c)) * plane_stride(g, c));
  }
  l.end = at;
  return l;
}
// block j of an MCU: its component, and where block (m, j) lies in its component's plane, in blocks
EXPO_HD int block_component(const Geometry& g, int j) { return g.ncomp == 1 || j < g.hs * g.vs ? 0 : j - g.hs * g.vs + 1; }
EXPO_HD void block_place(const Geometry& g, int64_t m, int j, int* brow, int* bcol) {
  const int my = int(m / g.mx), mx = int(m - int64_t(my) * g.mx);
  if (block_component(g, j) == 0 && g.ncomp == 3) {
    *brow = my * g.vs + j / g.hs;
    *bcol = mx * g.hs + j % g.hs;
  } else {
    *brow = my;
    *bcol = mx;
  }
}

// ------------------------------------------------------------------------------------------------ entropy decoding
// The bits of one segment: the file's bytes [pos, end) with the byte behind every FF dropped (FF 00 -> FF), most
// significant bit first.  acc holds nbits real bits left-aligned, zeros below them; past the end the window reads zeros.
struct BitReader {
  const uint8_t* file;
  int64_t pos, end;
  uint64_t acc;
  int nbits;
};
EXPO_HD BitReader open_bits(const uint8_t* file, int64_t file_bytes, int64_t begin, int64_t end) {
  BitReader r;
  r.file = file;
  r.pos = begin < 0 ? 0 : begin > file_bytes ? file_bytes : begin;  // whatever the plan says: inside the file
  r.end = end < r.pos ? r.pos : end > file_bytes ? file_bytes : end;
  r.acc = 0;
  r.nbits = 0;
  return r;
}
// at least 57 bits, or every bit that is left (at most 8 bytes a call)
EXPO_HD void fill(BitReader& r) {
  for (int e = 0; e < 8 && r.nbits <= 56 && r.pos < r.end; ++e) {
    const uint32_t b = r.file[r.pos++];
    if (b == 0xFFu) ++r.pos;  // the stuffed 00
    r.acc |= uint64_t(b) << (56 - r.nbits);
    r.nbits += 8;
  }
}
EXPO_HD void skip(BitReader& r, int n) {
  r.acc <<= n;
  r.nbits -= n;
}
// One Huffman symbol, or -1 with a flag in *status: no code in the 16-bit window is kBadCode when 16 real bits were
// there and kTruncated otherwise; a code longer than the bits left is kTruncated.
EXPO_HD int symbol(BitReader& r, const PlanHuff& t, int* status) {
  fill(r);
  const uint32_t window = uint32_t(r.acc >> 48);
  int len = 1;  // the limits never decrease: the first length whose limit is above the window is 1 + the limits at or
  for (int l = 0; l < 16; ++l) len += window >= t.limit[l] ? 1 : 0;  // below it (sixteen independent loads, no branch)
  if (len > 16) {
    *status |= r.nbits < 16 ? kTruncated : kBadCode;
    return -1;
  }
  if (len > r.nbits) {
    *status |= kTruncated;
    return -1;
  }
  const uint32_t code = window >> (16 - len);
  skip(r, len);
  return t.vals[(code + uint32_t(t.offs[len - 1])) & 255u];
}
// the n appended bits (1 <= n <= 15, behind a symbol: the reader holds them) as T.81's EXTEND; false: truncated
EXPO_HD bool value(BitReader& r, int n, int* v, int* status) {
  if (n > r.nbits) {
    *status |= kTruncated;
    return false;
  }
  const int x = int(r.acc >> (64 - n));
  skip(r, n);
  *v = x >> (n - 1) ? x : x - (1 << n) + 1;
  return true;
}
// One block: its 64 coefficients into the zeroed `slot` in natural order (int16; a value that does not fit wraps), the
// DC predictor updated.  Returns false with a flag in *status on an error; the slot then holds a part of the block.
// At most 1 + 63 symbols whatever the data.
EXPO_HD bool decode_block(BitReader& r, const PlanHuff& dc, const PlanHuff& ac, int* pred, int16_t* slot, int* status) {
  int s = symbol(r, dc, status);
  if (s < 0) return false;
  if (s > 15) {
    *status |= kBadCode;
    return false;
  }
  int v = 0;
  if (s && !value(r, s, &v, status)) return false;
  *pred = int(uint32_t(*pred) + uint32_t(v));
  slot[0] = int16_t(*pred);
  int k = 1;
  for (int e = 0; e < 63 && k < 64; ++e) {
    s = symbol(r, ac, status);
    if (s < 0) return false;
    const int run = s >> 4, size = s & 15;
    if (size == 0) {
      if (run != 15) break;  // EOB
      k += 16;               // ZRL
      if (k > 64) {
        *status |= kBadRun;
        return false;
      }
      continue;
    }
    k += run;
    if (k > 63) {
      *status |= kBadRun;
      return false;
    }
    if (!value(r, size, &v, status)) return false;
    slot[kZigzag[k]] = int16_t(v);
    ++k;
  }
  return true;
}

// One segment (lane k of a picture): its MCUs' blocks into the picture's coefficients `coef` (16-byte vectors V, eight
// per block), each staged in the lane's own 128-byte `slot`.  Returns the status flags.  Whatever the plan says, the
// bytes read lie inside the file and the blocks written are those of MCUs [k ri, k ri + ri) inside the picture; on an
// error the lane stops reading and the rest of its blocks, the one it stopped in included, are all-zero.
template <typename V>
EXPO_HD int decode_segment(const uint8_t* file, int64_t file_bytes, const uint8_t* planp, const Geometry& g, int k,
                           V* slot, V* coef, const V zero) {
  static_assert(sizeof(V) == 16, "16-byte vectors");
  const PlanHead* plan = reinterpret_cast<const PlanHead*>(planp);
  const int64_t all = mcus(g);
  int64_t ri = plan->ri;
  if (ri < 1 || ri > all) ri = all;
  const int64_t m0 = int64_t(k) * ri < all ? int64_t(k) * ri : all, m1 = m0 + ri < all ? m0 + ri : all;
  const int32_t* range = reinterpret_cast<const int32_t*>(planp + sizeof(PlanHead)) + 2 * int64_t(k);
  BitReader r = open_bits(file, file_bytes, range[0], range[1]);
  V* out = coef + m0 * g.bpm * 8;
  int pred0 = 0, pred1 = 0, pred2 = 0, st = 0;
  bool dead = false;
  for (int64_t m = m0; m < m1; ++m)
    for (int j = 0; j < g.bpm; ++j) {
      for (int e = 0; e < 8; ++e) slot[e] = zero;
      if (!dead) {
        const int c = block_component(g, j);
        int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
        const PlanHuff& dc = plan->huff[plan->td[c] & 1];
        const PlanHuff& ac = plan->huff[2 + (plan->ta[c] & 1)];
        if (!decode_block(r, dc, ac, &pred, reinterpret_cast<int16_t*>(slot), &st)) {
          dead = true;
          for (int e = 0; e < 8; ++e) slot[e] = zero;
        }
        pred0 = c == 0 ? pred : pred0, pred1 = c == 1 ? pred : pred1, pred2 = c == 2 ? pred : pred2;
      }
      for (int e = 0; e < 8; ++e) out[e] = slot[e];
      out += 8;
    }
  return st;
}

// ------------------------------------------------------------------------------------------------ reconstruction
// libjpeg's "islow" 8-point pass, constants at 13 bits, descale shift s (11 for the columns, 18 for the rows), in
// wrapping 32-bit arithmetic: for |dequantised coefficient| < 2^15 nothing wraps.
EXPO_HD void idct_pass(const int32_t* in, int s, int32_t* out) {
  constexpr uint32_t C0_298 = 2446, C0_390 = 3196, C0_541 = 4433, C0_765 = 6270, C0_899 = 7373, C1_175 = 9633,
                     C1_501 = 12299, C1_847 = 15137, C1_961 = 16069, C2_053 = 16819, C2_562 = 20995, C3_072 = 25172;
  const uint32_t i0 = uint32_t(in[0]), i1 = uint32_t(in[1]), i2 = uint32_t(in[2]), i3 = uint32_t(in[3]),
                 i4 = uint32_t(in[4]), i5 = uint32_t(in[5]), i6 = uint32_t(in[6]), i7 = uint32_t(in[7]);
  uint32_t z1 = (i2 + i6) * C0_541;
  const uint32_t t2 = z1 - i6 * C1_847, t3 = z1 + i2 * C0_765;
  const uint32_t t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a = i7, b = i5, c = i3, e = i1;
  z1 = a + e;
  uint32_t z2 = b + c, z3 = a + c, z4 = b + e;
  const uint32_t z5 = (z3 + z4) * C1_175;
  a *= C0_298, b *= C2_053, c *= C3_072, e *= C1_501;
  z1 *= 0u - C0_899, z2 *= 0u - C2_562;
  z3 = z3 * (0u - C1_961) + z5;
  z4 = z4 * (0u - C0_390) + z5;
  a += z1 + z3, b += z2 + z4, c += z2 + z3, e += z1 + z4;
  const uint32_t round = 1u << (s - 1);
  out[0] = int32_t(t10 + e + round) >> s;
  out[7] = int32_t(t10 - e + round) >> s;
  out[1] = int32_t(t11 + c + round) >> s;
  out[6] = int32_t(t11 - c + round) >> s;
  out[2] = int32_t(t12 + b + round) >> s;
  out[5] = int32_t(t12 - b + round) >> s;
  out[3] = int32_t(t13 + a + round) >> s;
  out[4] = int32_t(t13 - a + round) >> s;
}
EXPO_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
EXPO_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// libjpeg's "fancy" upsampling across: the two outputs of chroma sample `mid` with its neighbours (clamped by the caller)
EXPO_HD int up2x1_even(int left, int mid) { return (3 * mid + left + 1) >> 2; }
EXPO_HD int up2x1_odd(int mid, int right) { return (3 * mid + right + 2) >> 2; }
// 2 x 2: first down (r = 3 near + far), then across on r
EXPO_HD int up2x2_row(int near, int far) { return 3 * near + far; }
EXPO_HD int up2x2_even(int rleft, int rmid) { return (3 * rmid + rleft + 8) >> 4; }
EXPO_HD int up2x2_odd(int rmid, int rright) { return (3 * rmid + rright + 7) >> 4; }

EXPO_HD void rgb(int y, int cb, int cr, uint8_t* out) {
  cb -= 128;
  cr -= 128;
  out[0] = uint8_t(clamp255(y + ((91881 * cr + 32768) >> 16)));
  out[1] = uint8_t(clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16)));
  out[2] = uint8_t(clamp255(y + ((116130 * cb + 32768) >> 16)));
}

// The output pixels of chroma sample (uy, ux) -- one, 2 x 1 or 2 x 2, cropped to the picture -- from the planes in `ws`
// into the (h, w, 3) bytes at `out`: upsampling with indices clamped to the real plane, then the colour conversion.
EXPO_HD void rgb_unit(const Geometry& g, const Layout& lay, const uint8_t* ws, uint8_t* out, int uy, int ux) {
  const int dh = plane_h(g, g.ncomp - 1), dw = plane_w(g, g.ncomp - 1);
  const uint8_t* py = ws + lay.plane[0];
  const int sy = plane_stride(g, 0);
  const int64_t row = int64_t(g.w) * 3;
  if (g.ncomp == 1) {
    const uint8_t v = py[int64_t(uy) * sy + ux];
    uint8_t* o = out + uy * row + ux * 3;
    o[0] = v, o[1] = v, o[2] = v;
    return;
  }
  const uint8_t* pb = ws + lay.plane[1];
  const uint8_t* pr = ws + lay.plane[2];
  const int sc = plane_stride(g, 1);
  if (g.hs == 1) {
    rgb(py[int64_t(uy) * sy + ux], pb[int64_t(uy) * sc + ux], pr[int64_t(uy) * sc + ux], out + uy * row + ux * 3);
    return;
  }
  const int xl = ux > 0 ? ux - 1 : 0, xr = ux < dw - 1 ? ux + 1 : dw - 1;
  if (g.vs == 1) {
    const uint8_t* b = pb + int64_t(uy) * sc;
    const uint8_t* c = pr + int64_t(uy) * sc;
    const int x = 2 * ux;
    uint8_t* o = out + uy * row + x * 3;
    rgb(py[int64_t(uy) * sy + x], up2x1_even(b[xl], b[ux]), up2x1_even(c[xl], c[ux]), o);
    if (x + 1 < g.w) rgb(py[int64_t(uy) * sy + x + 1], up2x1_odd(b[ux], b[xr]), up2x1_odd(c[ux], c[xr]), o + 3);
    return;
  }
  const int yu = uy > 0 ? uy - 1 : 0, yd = uy < dh - 1 ? uy + 1 : dh - 1;
  // r of the upper (u) and the lower (d) output row at xl, ux, xr
  const int nb0 = pb[int64_t(uy) * sc + xl], nb1 = pb[int64_t(uy) * sc + ux], nb2 = pb[int64_t(uy) * sc + xr];
  const int nc0 = pr[int64_t(uy) * sc + xl], nc1 = pr[int64_t(uy) * sc + ux], nc2 = pr[int64_t(uy) * sc + xr];
  for (int d = 0; d < 2; ++d) {
    const int y = 2 * uy + d, x = 2 * ux, yf = d == 0 ? yu : yd;
    if (y >= g.h) break;
    const int rb0 = up2x2_row(nb0, pb[int64_t(yf) * sc + xl]), rb1 = up2x2_row(nb1, pb[int64_t(yf) * sc + ux]),
              rb2 = up2x2_row(nb2, pb[int64_t(yf) * sc + xr]);
    const int rc0 = up2x2_row(nc0, pr[int64_t(yf) * sc + xl]), rc1 = up2x2_row(nc1, pr[int64_t(yf) * sc + ux]),
              rc2 = up2x2_row(nc2, pr[int64_t(yf) * sc + xr]);
    uint8_t* o = out + y * row + x * 3;
    rgb(py[int64_t(y) * sy + x], up2x2_even(rb0, rb1), up2x2_even(rc0, rc1), o);
    if (x + 1 < g.w) rgb(py[int64_t(y) * sy + x + 1], up2x2_odd(rb1, rb2), up2x2_odd(rc1, rc2), o + 3);
  }
}

}  // namespace jpegdec
}  // namespace expo
