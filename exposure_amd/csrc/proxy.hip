// proxy.hip -- the agent's low-resolution proxies on the device: plain bilinear resampling (half-pixel centres, no
// antialiasing) of square windows of linear NHWC images to S x S.  expo_bilinear_resize_ragged; DESIGN.md §3.20.
//
//   bilinear_resize_kernel  one thread per output pixel of one window: two source coordinates, four taps of three
//                           channels.  The kernel reads 4 S^2 pixels of a window whatever its side, so it is bound by
//                           the latency of its gathers, not by bytes: a thread issues its twelve element loads (any
//                           alignment, any stride) before it uses one of them, and a launch of 64 windows at S = 64 is
//                           1024 blocks (four per CU).  No LDS, no atomics, no workspace; an output value depends on
//                           its own window alone.
//
// The arithmetic is torch's upsample_bilinear2d(align_corners=False, antialias=False) spelled out in individually
// rounded float32 operations: this unit is compiled with -ffp-contract=off (csrc/build.sh), so the host restatement
// (tests/_bilinear_ref.py) reproduces every bit.  The scale side / S is divided on the host (IEEE) and travels in the
// table.
#include "host_common.h"

namespace expo {

namespace {

constexpr int kProxyMaxWindows = 64;  // windows per launch, by value in the kernel arguments
constexpr int kProxyMaxS = 4096;      // S^2 output pixels of a window are indexed by one int

struct ProxyTable {
  const void* x[kProxyMaxWindows];  // the first element of the window (row y0, column x0) in its image
  long stride[kProxyMaxWindows];    // elements per image row (3 W)
  int side[kProxyMaxWindows];
  float scale[kProxyMaxWindows];    // fl32(float(side) / float(S))
  void* out;                        // [windows of this launch][S][S][3]
  int S;
};
static_assert(sizeof(ProxyTable) <= 4096, "the proxy table must fit the 4 KB kernarg block");

#pragma clang fp contract(off)
// source coordinate of output index d along one axis: the lower tap i0 (i1 = i0 + step) and the weight l1 of i1
__device__ __forceinline__ void bilinear_axis(int d, float scale, int side, int& i0, int& step, float& l0, float& l1) {
  const float t = scale * (float(d) + 0.5f);  // the product is rounded, then the subtraction
  const float src = fmaxf(t - 0.5f, 0.0f);
  i0 = int(src);
  i0 = i0 < side - 1 ? i0 : side - 1;  // (src < side always; the clamp only keeps a read inside whatever happens)
  step = i0 < side - 1 ? 1 : 0;
  l1 = src - float(i0);
  l0 = 1.0f - l1;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void bilinear_resize_kernel(const ProxyTable tab) {
  const int j = blockIdx.y, S = tab.S;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= S * S) return;
  const int oy = p / S, ox = p - oy * S;
  const int side = tab.side[j];
  const float scale = tab.scale[j];
  int y0, ys, x0, xs;
  float hl0, hl1, wl0, wl1;
  bilinear_axis(oy, scale, side, y0, ys, hl0, hl1);
  bilinear_axis(ox, scale, side, x0, xs, wl0, wl1);
  const long stride = tab.stride[j];
  const TI* r0 = static_cast<const TI*>(tab.x[j]) + long(y0) * stride + long(x0) * 3;
  const TI* r1 = r0 + (ys ? stride : 0);
  const int dx = xs * 3;
  // all twelve loads are issued before the first use
  TI a[3], b[3], c[3], d[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    a[ch] = r0[ch];
    b[ch] = r0[dx + ch];
    c[ch] = r1[ch];
    d[ch] = r1[dx + ch];
  }
  TO* out = static_cast<TO*>(tab.out) + (long(j) * S * S + p) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float top = wl0 * float(a[ch]) + wl1 * float(b[ch]);
    const float bot = wl0 * float(c[ch]) + wl1 * float(d[ch]);
    out[ch] = TO(hl0 * top + hl1 * bot);
  }
}
#pragma clang fp contract(on)

inline long elem_bytes(int dtype) { return dtype == EXPO_F16 ? 2 : 4; }

// arguments validated by the caller
template <typename TI, typename TO>
int bilinear_resize_t(const void* const* xs, const int* ws, const int32_t* windows, int q, int S, void* out,
                      hipStream_t s) {
  const unsigned blocks_x = unsigned((S * S + kThreads - 1) / kThreads);
  for (int base = 0; base < q; base += kProxyMaxWindows) {
    const int m = q - base < kProxyMaxWindows ? q - base : kProxyMaxWindows;
    ProxyTable tab = {};
    tab.S = S;
    tab.out = static_cast<TO*>(out) + long(base) * S * S * 3;
    for (int j = 0; j < m; ++j) {
      const int32_t* w = windows + 4 * (base + j);
      const long stride = long(ws[w[0]]) * 3;
      tab.x[j] = static_cast<const TI*>(xs[w[0]]) + long(w[1]) * stride + long(w[2]) * 3;
      tab.stride[j] = stride;
      tab.side[j] = w[3];
      tab.scale[j] = float(w[3]) / float(S);
    }
    hipLaunchKernelGGL((bilinear_resize_kernel<TI, TO>), dim3(blocks_x, unsigned(m)), dim3(kThreads), 0, s, tab);
    HIP_TRY(hipGetLastError(), "bilinear_resize launch");
  }
  return EXPO_OK;
}

}  // namespace

}  // namespace expo

// (proxy_codes.hip includes this file for the arithmetic above and defines this: the export below, and with it the
// kernels above, belong to this unit alone)
#ifndef EXPO_PROXY_TEMPLATES_ONLY
using namespace expo;

extern "C" {

int expo_bilinear_resize_ragged(const void* const* xs, const int* hs, const int* ws, int n, int in_dtype,
                                const int32_t* windows, int q, int S, void* out, int out_dtype, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0 || q < 0) return fail(EXPO_E_BADARG, "n >= 0 and q >= 0 required");
  if ((in_dtype != EXPO_F16 && in_dtype != EXPO_F32) || (out_dtype != EXPO_F16 && out_dtype != EXPO_F32))
    return fail(EXPO_E_BADDTYPE, "in_dtype and out_dtype must be EXPO_F16 or EXPO_F32");
  if (q == 0) return EXPO_OK;
  if (S < 1 || S > kProxyMaxS) return fail(EXPO_E_BADARG, "1 <= S <= 4096 required");
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
    if (w[3] < 1) return fail(EXPO_E_BADARG, "window side >= 1 required");
    if (w[1] < 0 || w[2] < 0 || long(w[1]) + w[3] > hs[w[0]] || long(w[2]) + w[3] > ws[w[0]])
      return fail(EXPO_E_BADARG, "window outside its image");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (in_dtype == EXPO_F32)
    return out_dtype == EXPO_F32 ? bilinear_resize_t<float, float>(xs, ws, windows, q, S, out, s)
                                 : bilinear_resize_t<float, half_t>(xs, ws, windows, q, S, out, s);
  return out_dtype == EXPO_F32 ? bilinear_resize_t<half_t, float>(xs, ws, windows, q, S, out, s)
                               : bilinear_resize_t<half_t, half_t>(xs, ws, windows, q, S, out, s);
}

}  // extern "C"
#endif  // EXPO_PROXY_TEMPLATES_ONLY
