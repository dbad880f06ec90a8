// jpeg_encode.hip -- baseline JPEG files made on the device (expo_jpeg_encode_ragged): colour
// conversion, the 8 x 8 transform, quantisation and the fixed Huffman code of T.81 Annex K, cut by restart markers into
// intervals of Ri MCUs that are coded on their own and end on a byte boundary, so that no workgroup waits for another.
// Default flags (csrc/build.sh).  Integer code only: no float, no global atomic, no zero-filled state; the bytes depend
// on the picture, the quality and the sampling alone.  Three launches per group of up to 64 pictures, in stream order:
//   jpeg_interval_kernel<S, false>  a wave per interval: loads its MCUs with the edge clamp, converts, downsamples and
//                                   level-shifts into LDS, runs the two 8-point passes and the quantiser in place, a
//                                   lane per block counts and then packs its symbols into LDS words, the 1-padding,
//                                   and the count of the stuffed bytes, which is all it stores (4 bytes)
//   jpeg_scan_kernel                a workgroup per picture: the intervals' offsets in the file, the file's length
//   jpeg_interval_kernel<S, true>   the same interval once more, for the pictures whose file fits their capacity: the
//                                   stuffed bytes go straight to their place in the file with the marker behind them;
//                                   an interval's first wave also writes the 629 header bytes
// The interval is computed twice rather than kept: its worst case is 2 x 48 x 1660 bits = 19 920 bytes for 2048 pixels
// of 4:2:0, 3.2 times raw, and the coefficients would be 1 to 2 times raw; length and offset are 12 bytes per interval.
// The serial routines are jpeg_codec.h's, which tools/jpeg_rehearse.cpp runs on the host.
#include <limits.h>

#include "host_common.h"
#include "jpeg_codec.h"

namespace expo {

namespace {

using namespace jpeg;

constexpr int kJpegMaxImages = 64;
constexpr int kJpegThreads = 64;                              // one wave per interval

// up to 64 pictures by value in the kernel arguments (3.1 KB)
struct JpegTable {
  const uint8_t* pic[kJpegMaxImages];
  uint8_t* out[kJpegMaxImages];
  int64_t base[kJpegMaxImages];  // the picture's part of the workspace (jpeg::layout)
  int64_t cap[kJpegMaxImages];
  int h[kJpegMaxImages];
  int w[kJpegMaxImages];
  int first_int[kJpegMaxImages + 1];  // first interval
  int n;
  int quality;
};
static_assert(sizeof(JpegTable) + 32 <= 4096, "the table must fit the 4 KB kernarg block");

// the last image whose first block is <= b
__device__ __forceinline__ int find_image(const int* first, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

struct CountSink {
  uint32_t bits;
  __device__ __forceinline__ void put(uint32_t, int n) { bits += uint32_t(n); }
};
// `n` bits (at most 32) of `v` into the zeroed LDS words at bit `pos`, most significant bit first
struct PackSink {
  uint32_t* words;
  uint32_t pos;
  __device__ __forceinline__ void put(uint32_t v, int n) {
    const uint64_t x = uint64_t(v) << (64 - n - int(pos & 31));
    atomicOr(&words[pos >> 5], uint32_t(x >> 32));
    if (uint32_t(x)) atomicOr(&words[(pos >> 5) + 1], uint32_t(x));
    pos += uint32_t(n);
  }
};

// byte j of the packed bits
__device__ __forceinline__ uint32_t packed_byte(const uint32_t* words, int j) { return (words[j >> 2] >> (24 - 8 * (j & 3))) & 255u; }

// inclusive sums over the workgroup's one wave, through LDS
__device__ __forceinline__ uint32_t wave_scan(uint32_t* scan, int t, uint32_t mine) {
  scan[t] = mine;
  __syncthreads();
  for (int d = 1; d < kJpegThreads; d <<= 1) {
    const uint32_t add = t >= d ? scan[t - d] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  return scan[t];
}

template <int kSub, bool kWrite>
__global__ __launch_bounds__(kJpegThreads) void jpeg_interval_kernel(const JpegTable tab, uint8_t* __restrict__ ws) {
  constexpr int kRi = kSub == 0 ? kRestart444 : kRestart420;
  constexpr int kBpm = kSub == 0 ? 3 : 6;
  constexpr int kBitWords = (kRi * kBpm * kBlockBits + 31) / 32 + 2;  // an interval's unstuffed bits, and the padding
  __shared__ int16_t blk[kRi * kBpm * 64];
  __shared__ uint32_t bits[kBitWords];
  __shared__ uint32_t code_ac[2][256];
  __shared__ uint32_t code_dc[2][12];
  __shared__ uint8_t qtab[2][64];
  __shared__ uint32_t scan[kJpegThreads];
  __shared__ uint8_t header[kWrite ? 640 : 4];

  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int i = find_image(tab.first_int, tab.n, b);
  const int k = b - tab.first_int[i];
  const int h = tab.h[i], w = tab.w[i];
  const int mx = int(mcus_x(w, kSub));
  const int nmcu_all = mx * int(mcus_x(h, kSub));  // at most 8192^2
  const int nint = (nmcu_all + kRi - 1) / kRi;
  const Layout lay = layout(tab.base[i], nint);
  if (kWrite && *reinterpret_cast<const int64_t*>(ws + lay.rec) > tab.cap[i]) return;  // block-uniform: the file does not fit
  const int m_first = k * kRi;
  const int nm = nmcu_all - m_first < kRi ? nmcu_all - m_first : kRi;
  const int nblk = nm * kBpm;
  const uint8_t* pic = tab.pic[i];

  for (int s = t; s < 512; s += kJpegThreads) code_ac[s >> 8][s & 255] = kCodes.ac[s >> 8][s & 255];
  if (t < 24) code_dc[t / 12][t % 12] = kCodes.dc[t / 12][t % 12];
  for (int s = t; s < 128; s += kJpegThreads) qtab[s >> 6][s & 63] = uint8_t(quant_value(s >> 6, s & 63, tab.quality));

  // the MCUs' samples, level-shifted, block after block in the order of the scan
  for (int p = t; p < nm * 64; p += kJpegThreads) {
    const int m = p >> 6, yy = (p >> 3) & 7, xx = p & 7;
    const int g = m_first + m, my = g / mx, mxi = g - my * mx;
    if (kSub == 0) {
      const int gy = min(my * 8 + yy, h - 1), gx = min(mxi * 8 + xx, w - 1);
      const uint8_t* px = pic + (size_t(gy) * size_t(w) + size_t(gx)) * 3;
      int y, cb, cr;
      ycc(px[0], px[1], px[2], &y, &cb, &cr);
      blk[(m * 3 + 0) * 64 + yy * 8 + xx] = int16_t(y - 128);
      blk[(m * 3 + 1) * 64 + yy * 8 + xx] = int16_t(cb - 128);
      blk[(m * 3 + 2) * 64 + yy * 8 + xx] = int16_t(cr - 128);
    } else {
      int sb = 0, sr = 0;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int py = 2 * yy + (d >> 1), qx = 2 * xx + (d & 1);
        const int gy = min(my * 16 + py, h - 1), gx = min(mxi * 16 + qx, w - 1);
        const uint8_t* px = pic + (size_t(gy) * size_t(w) + size_t(gx)) * 3;
        int y, cb, cr;
        ycc(px[0], px[1], px[2], &y, &cb, &cr);
        blk[(m * 6 + (py >> 3) * 2 + (qx >> 3)) * 64 + (py & 7) * 8 + (qx & 7)] = int16_t(y - 128);
        sb += cb;
        sr += cr;
      }
      blk[(m * 6 + 4) * 64 + yy * 8 + xx] = int16_t(((sb + 2) >> 2) - 128);
      blk[(m * 6 + 5) * 64 + yy * 8 + xx] = int16_t(((sr + 2) >> 2) - 128);
    }
  }
  __syncthreads();
  for (int r = t; r < nblk * 8; r += kJpegThreads) dct_row(&blk[r * 8], 1, &blk[r * 8]);
  __syncthreads();
  for (int c = t; c < nblk * 8; c += kJpegThreads) {
    const int bl = c >> 3, u = c & 7;
    int32_t f[8];
    dct_col(&blk[bl * 64 + u], 8, f);
    const uint8_t* q = qtab[block_table(bl, kSub)];
#pragma unroll
    for (int v = 0; v < 8; ++v) blk[bl * 64 + v * 8 + u] = int16_t(quantise(f[v], q[v * 8 + u]));
  }
  __syncthreads();

  // a lane per block: its bits, where they start, then the bits themselves
  int pred = 0, id = 0;
  uint32_t my_bits = 0;
  if (t < nblk) {
    const int pb = dc_pred_block(t, kSub);
    pred = pb >= 0 ? int(blk[pb * 64]) : 0;
    id = block_table(t, kSub);
    CountSink cs = {0};
    block_symbols(&blk[t * 64], 1, pred, code_dc[id], code_ac[id], cs);
    my_bits = cs.bits;
  }
  const uint32_t upto = wave_scan(scan, t, my_bits);
  const uint32_t all_bits = scan[kJpegThreads - 1];
  const int nbytes = int((all_bits + 7) >> 3);
  for (int e = t; e < (nbytes + 3) / 4 + 1; e += kJpegThreads) bits[e] = 0;
  __syncthreads();
  if (t < nblk) {
    PackSink ps = {bits, upto - my_bits};
    block_symbols(&blk[t * 64], 1, pred, code_dc[id], code_ac[id], ps);
  }
  if (t == kJpegThreads - 1 && (all_bits & 7)) {  // the padding: 1-bits to the byte
    PackSink ps = {bits, all_bits};
    const int npad = 8 - int(all_bits & 7);
    ps.put((1u << npad) - 1u, npad);
  }
  __syncthreads();

  // every 0xFF is followed by a zero byte: a lane counts those of its run of bytes
  const int per = (nbytes + kJpegThreads - 1) / kJpegThreads;
  const int j0 = min(t * per, nbytes), j1 = min(j0 + per, nbytes);
  uint32_t ff = 0;
  for (int j = j0; j < j1; ++j) ff += packed_byte(bits, j) == 255u ? 1u : 0u;
  __syncthreads();  // scan[] is read above
  const uint32_t ff_upto = wave_scan(scan, t, ff);
  const uint32_t stuffed = uint32_t(nbytes) + scan[kJpegThreads - 1];
  if (!kWrite) {
    if (t == 0) reinterpret_cast<uint32_t*>(ws + lay.counts)[k] = stuffed;
    return;
  }
  uint8_t* dst = tab.out[i] + reinterpret_cast<const int64_t*>(ws + lay.offs)[k];
  uint8_t* o = dst + j0 + (ff_upto - ff);
  for (int j = j0; j < j1; ++j) {
    const uint32_t v = packed_byte(bits, j);
    *o++ = uint8_t(v);
    if (v == 255u) *o++ = 0;
  }
  if (t == 0) {
    dst[stuffed] = 0xFF;
    dst[stuffed + 1] = k == nint - 1 ? 0xD9 : uint8_t(0xD0 + (k & 7));
  }
  if (k == 0) {  // block-uniform
    if (t == 0) write_header(header, h, w, tab.quality, kSub);
    __syncthreads();
    for (int e = t; e < kHeaderBytes; e += kJpegThreads) tab.out[i][e] = header[e];
  }
}

// a workgroup per picture: every thread walks a run of consecutive intervals, lane 0 joins the 256 runs
__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(const JpegTable tab, uint8_t* __restrict__ ws,
                                                             int64_t* __restrict__ sizes, int sub) {
  __shared__ int64_t run_bytes[kThreads];
  const int t = threadIdx.x, i = blockIdx.x;
  const int64_t nint = intervals(tab.h[i], tab.w[i], sub);
  const Layout lay = layout(tab.base[i], nint);
  const uint32_t* counts = reinterpret_cast<const uint32_t*>(ws + lay.counts);
  int64_t* offs = reinterpret_cast<int64_t*>(ws + lay.offs);
  const int64_t per = (nint + kThreads - 1) / kThreads;
  const int64_t k0 = t * per < nint ? t * per : nint, k1 = k0 + per < nint ? k0 + per : nint;
  int64_t bytes = 0;
  for (int64_t k = k0; k < k1; ++k) bytes += int64_t(counts[k]) + 2;  // the payload and its marker
  run_bytes[t] = bytes;
  __syncthreads();
  if (t == 0) {
    int64_t at = kHeaderBytes;
    for (int o = 0; o < kThreads; ++o) {
      const int64_t nb = run_bytes[o];
      run_bytes[o] = at;
      at += nb;
    }
    *reinterpret_cast<int64_t*>(ws + lay.rec) = at;
    sizes[i] = at;
  }
  __syncthreads();
  int64_t at = run_bytes[t];
  for (int64_t k = k0; k < k1; ++k) {
    offs[k] = at;
    at += int64_t(counts[k]) + 2;
  }
}

}  // namespace

}  // namespace expo

using namespace expo;

namespace {

// bytes of workspace of images [base, base + m): the pictures' parts behind one another
int64_t group_workspace(const int* hs, const int* ws, int base, int m, int sub, int64_t* bases) {
  int64_t at = 0;
  for (int j = 0; j < m; ++j) {
    if (bases) bases[j] = at;
    at = jpeg::layout(at, jpeg::intervals(hs[base + j], ws[base + j], sub)).end;
  }
  return at;
}

template <int kSub>
int launch_group(const JpegTable& tab, int ints, int m, uint8_t* wsp, int64_t* sizes, hipStream_t s) {
  const dim3 wave(kJpegThreads);
  hipLaunchKernelGGL((jpeg_interval_kernel<kSub, false>), dim3(unsigned(ints)), wave, 0, s, tab, wsp);
  HIP_TRY(hipGetLastError(), "jpeg_interval (count) launch");
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(unsigned(m)), dim3(kThreads), 0, s, tab, wsp, sizes, kSub);
  HIP_TRY(hipGetLastError(), "jpeg_scan launch");
  hipLaunchKernelGGL((jpeg_interval_kernel<kSub, true>), dim3(unsigned(ints)), wave, 0, s, tab, wsp);
  HIP_TRY(hipGetLastError(), "jpeg_interval (write) launch");
  return EXPO_OK;
}

}  // namespace

extern "C" {

int expo_jpeg_restart_mcus(int subsampling) {
  const int ri = jpeg::restart_mcus(subsampling);
  if (ri < 0) fail(EXPO_E_BADARG, "subsampling must be 0 (4:4:4) or 2 (4:2:0)");
  return ri;
}

int64_t expo_jpeg_encode_bound(int h, int w, int subsampling) {
  if (jpeg::restart_mcus(subsampling) < 0) {
    fail(EXPO_E_BADARG, "subsampling must be 0 (4:4:4) or 2 (4:2:0)");
    return -1;
  }
  if (!jpeg::valid_picture(h, w)) {
    fail(EXPO_E_BADARG, "h and w in 1..65535 required");
    return -1;
  }
  return jpeg::file_bound(h, w, subsampling);
}

size_t expo_jpeg_encode_workspace_bytes(const int* hs, const int* ws, int n, int subsampling) {
  if (n < 1 || !hs || !ws || jpeg::restart_mcus(subsampling) < 0) return 0;
  for (int i = 0; i < n; ++i)
    if (!jpeg::valid_picture(hs[i], ws[i])) return 0;
  int64_t most = 0;  // a launch group at a time uses it
  for (int base = 0; base < n; base += kJpegMaxImages) {
    const int64_t need = group_workspace(hs, ws, base, n - base < kJpegMaxImages ? n - base : kJpegMaxImages, subsampling, nullptr);
    most = need > most ? need : most;
  }
  return size_t(most);
}

int expo_jpeg_encode_ragged(const void* const* pics, const int* hs, const int* ws, int n, int quality, int subsampling,
                            void* const* outs, const int64_t* out_capacity, int64_t* sizes, void* workspace,
                            size_t workspace_bytes, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (quality < 1 || quality > 100) return fail(EXPO_E_BADARG, "quality must be 1..100");
  if (jpeg::restart_mcus(subsampling) < 0) return fail(EXPO_E_BADARG, "subsampling must be 0 (4:4:4) or 2 (4:2:0)");
  if (n == 0) return EXPO_OK;
  if (!hs || !ws) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i)
    if (!jpeg::valid_picture(hs[i], ws[i])) return fail(EXPO_E_BADARG, "h and w in 1..65535 required");
  if (!pics || !outs || !out_capacity || !sizes) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (!pics[i] || !outs[i]) return fail(EXPO_E_BADARG, "null picture pointer");
    if (out_capacity[i] < 0) return fail(EXPO_E_BADARG, "out_capacity >= 0 required");
  }
  if (workspace_bytes < expo_jpeg_encode_workspace_bytes(hs, ws, n, subsampling)) return fail(EXPO_E_BADARG, "workspace too small");
  if (!workspace) return fail(EXPO_E_BADARG, "null workspace");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(EXPO_E_BADARG, "the workspace must be 16-byte aligned");
  for (int base = 0; base < n; base += kJpegMaxImages) {  // the grids of every group, before the first launch
    long ints = 0;
    for (int i = base; i < n && i < base + kJpegMaxImages; ++i) ints += long(jpeg::intervals(hs[i], ws[i], subsampling));
    if (ints > INT_MAX - kJpegMaxImages) return fail(EXPO_E_BADARG, "too many blocks in one launch");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* wsp = static_cast<uint8_t*>(workspace);
  for (int base = 0; base < n; base += kJpegMaxImages) {
    const int m = n - base < kJpegMaxImages ? n - base : kJpegMaxImages;
    JpegTable tab = {};
    tab.n = m;
    tab.quality = quality;
    group_workspace(hs, ws, base, m, subsampling, tab.base);
    long ints = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j;
      tab.pic[j] = static_cast<const uint8_t*>(pics[i]);
      tab.out[j] = static_cast<uint8_t*>(outs[i]);
      tab.cap[j] = out_capacity[i];
      tab.h[j] = hs[i];
      tab.w[j] = ws[i];
      tab.first_int[j] = int(ints);
      ints += long(jpeg::intervals(hs[i], ws[i], subsampling));
    }
    tab.first_int[m] = int(ints);
    const int rc = subsampling == 0 ? launch_group<0>(tab, int(ints), m, wsp, sizes + base, s)
                                    : launch_group<2>(tab, int(ints), m, wsp, sizes + base, s);
    if (rc != EXPO_OK) return rc;
  }
  return EXPO_OK;
}

}  // extern "C"
