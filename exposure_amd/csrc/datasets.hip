// datasets.hip -- the training sets on the device: the master pack of a folder of photos and its per-epoch re-cut.
// expo_area_resize_ragged / expo_pack_recut; DESIGN.md §3.18.
//
//   area_resize_kernel  one block per (window, output row): INTER_AREA (OpenCV's computeResizeAreaTab weights, in
//                       double) of a square window of a linear NHWC image to S x S.  The block walks the source rows of
//                       its output row's cell with coalesced loads and keeps one weighted column sum per source column
//                       and channel in LDS (float, 12 bytes per column; output columns are tiled when a window's columns
//                       exceed kTileCols); then one lane per output value sums its cell's columns.  Every sum runs in a
//                       fixed order in double: no atomics, and a window's result does not depend on what else the
//                       launch holds.
//   pack_recut_kernel   one block per output row: a C x C crop of one master image, optionally flipped left-right (a
//                       copy, exact in either dtype).
#include "host_common.h"

namespace expo {

namespace {

constexpr int kResizeMaxWindows = 64;  // windows per launch, by value in the kernel arguments
constexpr int kTileCols = 4096;        // source columns of one LDS tile (48 KiB of float column sums)
constexpr int kChunk = 16;             // column-pass elements per thread held in registers (16 loads in flight)

struct ResizeTable {
  const void* x[kResizeMaxWindows];  // the first element of the window (row y0, column x0) in its image
  void* out[kResizeMaxWindows];      // [S][S][3] of the window
  long stride[kResizeMaxWindows];    // elements per image row (3 W)
  int side[kResizeMaxWindows];
  int S;
};
static_assert(sizeof(ResizeTable) <= 4096, "the resize table must fit the 4 KB kernarg block");

// computeResizeAreaTab along one axis for output index d: the source range [first, last] and its weights.  The
// arithmetic is the reference's double expressions, un-contracted, so the host restatement reproduces every decision.
struct Axis {
  double f1, f2, cell;
  int s1, s2, first, last;
};

#pragma clang fp contract(off)
__host__ __device__ inline Axis area_axis(int d, double scale, int side) {
  Axis a;
  a.f1 = d * scale;
  a.f2 = a.f1 + scale;
  a.cell = scale < side - a.f1 ? scale : side - a.f1;
  a.s1 = int(ceil(a.f1));
  a.s2 = int(floor(a.f2));
  a.s2 = a.s2 < side - 1 ? a.s2 : side - 1;
  a.s1 = a.s1 < a.s2 ? a.s1 : a.s2;
  a.first = a.s1 - a.f1 > 1e-3 ? a.s1 - 1 : a.s1;
  a.last = a.f2 - a.s2 > 1e-3 ? a.s2 : a.s2 - 1;
  return a;
}

__host__ __device__ inline double area_weight(const Axis& a, int s) {
  if (s < a.s1) return (a.s1 - a.f1) / a.cell;
  if (s < a.s2) return 1.0 / a.cell;
  const double t = a.f2 - a.s2 < 1.0 ? a.f2 - a.s2 : 1.0;
  return (t < a.cell ? t : a.cell) / a.cell;
}
#pragma clang fp contract(on)

// output columns of one tile: the span of their source columns is at most per * scale + 2 <= kTileCols
__host__ __device__ inline int tile_out_cols(double scale) { return int((kTileCols - 2) / scale); }

template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void area_resize_kernel(const ResizeTable tab) {
  __shared__ float colsum[kTileCols * 3];
  const int j = blockIdx.y, oy = blockIdx.x, S = tab.S;
  const int side = tab.side[j];
  const double scale = double(side) / S;
  const Axis ya = area_axis(oy, scale, side);
  const long stride = tab.stride[j];
  const TI* win = static_cast<const TI*>(tab.x[j]);
  TO* out = static_cast<TO*>(tab.out[j]) + long(oy) * S * 3;
  const int per = tile_out_cols(scale);
  for (int ox0 = 0; ox0 < S; ox0 += per) {
    const int ox1 = ox0 + per < S ? ox0 + per : S;
    const int c0 = area_axis(ox0, scale, side).first;
    const int c1 = area_axis(ox1 - 1, scale, side).last + 1;
    const int ne = min(c1 - c0, kTileCols) * 3;
    const TI* src0 = win + long(c0) * 3 + threadIdx.x;
    // column pass: colsum[e] = sum over the cell's rows of w_r x[r][c0 * 3 + e], rows in order
    for (int e0 = 0; e0 < ne; e0 += kThreads * kChunk) {
      double acc[kChunk];
#pragma unroll
      for (int k = 0; k < kChunk; ++k) acc[k] = 0.0;
      for (int r = ya.first; r <= ya.last; ++r) {
        const double wr = area_weight(ya, r);
        const TI* src = src0 + long(r) * stride + e0;
        float v[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) v[k] = e0 + k * kThreads + int(threadIdx.x) < ne ? float(src[k * kThreads]) : 0.0f;
#pragma unroll
        for (int k = 0; k < kChunk; ++k) acc[k] += wr * double(v[k]);
      }
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        const int e = e0 + k * kThreads + threadIdx.x;
        if (e < ne) colsum[e] = float(acc[k]);
      }
    }
    __syncthreads();
    // row pass: one lane per output value, its cell's columns in order
    for (int t = threadIdx.x; t < (ox1 - ox0) * 3; t += kThreads) {
      const int ox = ox0 + t / 3, ch = t - (t / 3) * 3;
      const Axis xa = area_axis(ox, scale, side);
      double s = 0.0;
      for (int c = xa.first; c <= xa.last; ++c) s += area_weight(xa, c) * double(colsum[(c - c0) * 3 + ch]);
      out[ox * 3 + ch] = TO(float(s));
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pack_recut_kernel(const T* __restrict__ master, int m, int S,
                                                              const int32_t* __restrict__ records, int C,
                                                              T* __restrict__ out) {
  const int r = blockIdx.x;
  // (a record out of range is the caller's error; it is clamped so that no read leaves the master)
  const int src = min(max(records[4 * r], 0), m - 1);
  const int oy = min(max(records[4 * r + 1], 0), S - C);
  const int ox = min(max(records[4 * r + 2], 0), S - C);
  const bool flip = records[4 * r + 3] != 0;
  const T* in = master + (long(src) * S + oy) * long(S) * 3 + long(ox) * 3;
  T* o = out + long(r) * C * C * 3;
  const int rowlen = C * 3, total = C * rowlen;
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int y = e / rowlen, rem = e - y * rowlen;
    const int x = rem / 3, ch = rem - x * 3;
    o[e] = in[long(y) * S * 3 + (flip ? C - 1 - x : x) * 3 + ch];
  }
}

inline long elem_bytes(int dtype) { return dtype == EXPO_F16 ? 2 : 4; }

template <typename TI, typename TO>
int area_resize_t(const void* const* xs, const int* ws, const int32_t* windows, int q, int S, void* out,
                  hipStream_t s) {
  for (int base = 0; base < q; base += kResizeMaxWindows) {
    const int m = q - base < kResizeMaxWindows ? q - base : kResizeMaxWindows;
    ResizeTable tab = {};
    tab.S = S;
    for (int j = 0; j < m; ++j) {
      const int32_t* w = windows + 4 * (base + j);
      const long stride = long(ws[w[0]]) * 3;
      tab.x[j] = static_cast<const TI*>(xs[w[0]]) + long(w[1]) * stride + long(w[2]) * 3;
      tab.out[j] = static_cast<TO*>(out) + long(base + j) * S * S * 3;
      tab.stride[j] = stride;
      tab.side[j] = w[3];
    }
    hipLaunchKernelGGL((area_resize_kernel<TI, TO>), dim3(unsigned(S), unsigned(m)), dim3(kThreads), 0, s, tab);
    HIP_TRY(hipGetLastError(), "area_resize launch");
  }
  return EXPO_OK;
}

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

int expo_area_resize_ragged(const void* const* xs, const int* hs, const int* ws, int n, int in_dtype,
                            const int32_t* windows, int q, int S, void* out, int out_dtype, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0 || q < 0) return fail(EXPO_E_BADARG, "n >= 0 and q >= 0 required");
  if ((in_dtype != EXPO_F16 && in_dtype != EXPO_F32) || (out_dtype != EXPO_F16 && out_dtype != EXPO_F32))
    return fail(EXPO_E_BADDTYPE, "in_dtype and out_dtype must be EXPO_F16 or EXPO_F32");
  if (q == 0) return EXPO_OK;
  if (S < 1 || S > 65535) return fail(EXPO_E_BADARG, "1 <= S <= 65535 required");
  if (n == 0) return fail(EXPO_E_BADARG, "windows need images (n == 0)");
  if (!xs || !hs || !ws || !windows || !out) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (int rc = check_common(1, hs[i], ws[i], in_dtype)) return rc;
    if (!xs[i]) return fail(EXPO_E_BADARG, "null image pointer");
  }
  if (long(q) * S * S * 3 * elem_bytes(out_dtype) > (1L << 40)) return fail(EXPO_E_BADARG, "output too large");
  for (int k = 0; k < q; ++k) {
    const int32_t* w = windows + 4 * k;
    if (w[0] < 0 || w[0] >= n) return fail(EXPO_E_BADARG, "window image index out of range");
    if (w[3] < S) return fail(EXPO_E_BADARG, "window side < S: upscaling is not an area resize");
    if (w[1] < 0 || w[2] < 0 || long(w[1]) + w[3] > hs[w[0]] || long(w[2]) + w[3] > ws[w[0]])
      return fail(EXPO_E_BADARG, "window outside its image");
    if (tile_out_cols(double(w[3]) / S) < 1) return fail(EXPO_E_BADARG, "window side / S too large for one LDS tile");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (in_dtype == EXPO_F32)
    return out_dtype == EXPO_F32 ? area_resize_t<float, float>(xs, ws, windows, q, S, out, s)
                                 : area_resize_t<float, half_t>(xs, ws, windows, q, S, out, s);
  return out_dtype == EXPO_F32 ? area_resize_t<half_t, float>(xs, ws, windows, q, S, out, s)
                               : area_resize_t<half_t, half_t>(xs, ws, windows, q, S, out, s);
}

int expo_pack_recut(const void* master, int m, int S, const int32_t* records, int count, int C, void* out, int dtype,
                    void* stream) {
  if (count < 0) return fail(EXPO_E_BADARG, "count >= 0 required");
  if (dtype != EXPO_F16 && dtype != EXPO_F32) return fail(EXPO_E_BADDTYPE, "dtype must be EXPO_F16 or EXPO_F32");
  if (S < 1 || C < 1 || C > S) return fail(EXPO_E_BADARG, "1 <= C <= S required");
  if (long(S) * S * 3 * elem_bytes(dtype) > (1L << 31)) return fail(EXPO_E_BADARG, "one master image must be <= 2 GiB");
  if (count == 0) return EXPO_OK;
  if (m < 1) return fail(EXPO_E_BADARG, "m >= 1 required");
  if (!master || !records || !out) return fail(EXPO_E_BADARG, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == EXPO_F32)
    hipLaunchKernelGGL(pack_recut_kernel<float>, dim3(unsigned(count)), dim3(kThreads), 0, s,
                       static_cast<const float*>(master), m, S, records, C, static_cast<float*>(out));
  else
    hipLaunchKernelGGL(pack_recut_kernel<half_t>, dim3(unsigned(count)), dim3(kThreads), 0, s,
                       static_cast<const half_t*>(master), m, S, records, C, static_cast<half_t*>(out));
  HIP_TRY(hipGetLastError(), "pack_recut launch");
  return EXPO_OK;
}

}  // extern "C"
