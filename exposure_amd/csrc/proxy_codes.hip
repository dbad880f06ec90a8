// proxy_codes.hip -- the agent's proxies read from the files' integer codes (expo_bilinear_resize_ragged_codes;
// DESIGN.md §3.23): bilinear_resize_kernel's thread with another loader.  A tap is float(table[code]), the value the
// decoded tensor would hold, with the image's table in the storage dtype (expo_decode_tables), so the float image need
// not exist.  Codes of 1 (the grey channel is replicated), 3 or 4 (alpha is dropped) channels, 8 or 16 bits, at any
// byte / element.
//
// A unit of its own with exactly proxy.hip's flags (-ffp-contract=off, csrc/build.sh): it includes that file for
// bilinear_axis and the launch constants and instantiates none of its kernels (EXPO_PROXY_TEMPLATES_ONLY), so proxy.hip
// compiles to what it was.  The arithmetic is bilinear_resize_kernel's, operation for operation.
#define EXPO_PROXY_TEMPLATES_ONLY
#include "proxy.hip"

namespace expo {

namespace {

#pragma clang fp contract(off)
// the windows of a codes launch: as ProxyTable, plus each window's table (its image's)
struct ProxyCodesTable {
  const void* x[kProxyMaxWindows];    // the first code of the window (row y0, column x0, channel 0) in its image
  const void* tab[kProxyMaxWindows];  // the table of the window's image, 2^bits entries in the storage dtype
  long stride[kProxyMaxWindows];      // codes per image row (C W)
  int side[kProxyMaxWindows];
  float scale[kProxyMaxWindows];
  void* out;
  int S;
};
static_assert(sizeof(ProxyCodesTable) <= 4096, "the proxy table must fit the 4 KB kernarg block");

// CT the code type, C the channels of the file (1: the grey channel is replicated; 4: alpha is dropped), TT the tables'
// dtype.  The twelve code loads are issued first, then the twelve table gathers, then the arithmetic of
// bilinear_resize_kernel on the widened values.
template <typename CT, int C, typename TT, typename TO>
__global__ __launch_bounds__(kThreads) void bilinear_resize_codes_kernel(const ProxyCodesTable tab) {
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
  const CT* r0 = static_cast<const CT*>(tab.x[j]) + long(y0) * stride + long(x0) * C;
  const CT* r1 = r0 + (ys ? stride : 0);
  const int dx = xs * C;
  const TT* lut = static_cast<const TT*>(tab.tab[j]);
  CT ka[3], kb[3], kc[3], kd[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int o = C == 1 ? 0 : ch;
    ka[ch] = r0[o];
    kb[ch] = r0[dx + o];
    kc[ch] = r1[o];
    kd[ch] = r1[dx + o];
  }
  TT a[3], b[3], c[3], d[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    a[ch] = lut[ka[ch]];
    b[ch] = lut[kb[ch]];
    c[ch] = lut[kc[ch]];
    d[ch] = lut[kd[ch]];
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

// arguments validated by the caller; table_stride in entries (0: one shared table)
template <typename CT, int C, typename TT, typename TO>
int bilinear_resize_codes_t(const void* const* codes, const int* ws, const void* tables, int table_stride,
                            const int32_t* windows, int q, int S, void* out, hipStream_t s) {
  const unsigned blocks_x = unsigned((S * S + kThreads - 1) / kThreads);
  for (int base = 0; base < q; base += kProxyMaxWindows) {
    const int m = q - base < kProxyMaxWindows ? q - base : kProxyMaxWindows;
    ProxyCodesTable tab = {};
    tab.S = S;
    tab.out = static_cast<TO*>(out) + long(base) * S * S * 3;
    for (int j = 0; j < m; ++j) {
      const int32_t* w = windows + 4 * (base + j);
      const long stride = long(ws[w[0]]) * C;
      tab.x[j] = static_cast<const CT*>(codes[w[0]]) + long(w[1]) * stride + long(w[2]) * C;
      tab.tab[j] = static_cast<const TT*>(tables) + size_t(w[0]) * size_t(table_stride);
      tab.stride[j] = stride;
      tab.side[j] = w[3];
      tab.scale[j] = float(w[3]) / float(S);
    }
    hipLaunchKernelGGL((bilinear_resize_codes_kernel<CT, C, TT, TO>), dim3(blocks_x, unsigned(m)), dim3(kThreads), 0, s,
                       tab);
    HIP_TRY(hipGetLastError(), "bilinear_resize_codes launch");
  }
  return EXPO_OK;
}

template <typename CT, int C>
int bilinear_resize_codes_c(int table_dtype, int out_dtype, const void* const* codes, const int* ws, const void* tables,
                            int table_stride, const int32_t* windows, int q, int S, void* out, hipStream_t s) {
  if (table_dtype == EXPO_F32)
    return out_dtype == EXPO_F32
               ? bilinear_resize_codes_t<CT, C, float, float>(codes, ws, tables, table_stride, windows, q, S, out, s)
               : bilinear_resize_codes_t<CT, C, float, half_t>(codes, ws, tables, table_stride, windows, q, S, out, s);
  return out_dtype == EXPO_F32
             ? bilinear_resize_codes_t<CT, C, half_t, float>(codes, ws, tables, table_stride, windows, q, S, out, s)
             : bilinear_resize_codes_t<CT, C, half_t, half_t>(codes, ws, tables, table_stride, windows, q, S, out, s);
}

template <typename CT>
int bilinear_resize_codes_ct(int channels, int table_dtype, int out_dtype, const void* const* codes, const int* ws,
                             const void* tables, int table_stride, const int32_t* windows, int q, int S, void* out,
                             hipStream_t s) {
  if (channels == 1)
    return bilinear_resize_codes_c<CT, 1>(table_dtype, out_dtype, codes, ws, tables, table_stride, windows, q, S, out, s);
  if (channels == 3)
    return bilinear_resize_codes_c<CT, 3>(table_dtype, out_dtype, codes, ws, tables, table_stride, windows, q, S, out, s);
  return bilinear_resize_codes_c<CT, 4>(table_dtype, out_dtype, codes, ws, tables, table_stride, windows, q, S, out, s);
}

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

int expo_bilinear_resize_ragged_codes(const void* const* codes, const int* hs, const int* ws, int n, int channels,
                                      int code_bits, const void* tables, int table_stride, int table_dtype,
                                      const int32_t* windows, int q, int S, void* out, int out_dtype, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0 || q < 0) return fail(EXPO_E_BADARG, "n >= 0 and q >= 0 required");
  if (channels != 1 && channels != 3 && channels != 4) return fail(EXPO_E_BADARG, "channels must be 1, 3 or 4");
  if (code_bits != 8 && code_bits != 16) return fail(EXPO_E_BADARG, "code_bits must be 8 or 16");
  if ((table_dtype != EXPO_F16 && table_dtype != EXPO_F32) || (out_dtype != EXPO_F16 && out_dtype != EXPO_F32))
    return fail(EXPO_E_BADDTYPE, "table_dtype and out_dtype must be EXPO_F16 or EXPO_F32");
  if (table_stride != 0 && table_stride < (1 << code_bits))
    return fail(EXPO_E_BADARG, "table_stride must be 0 (one shared table) or at least 2^code_bits entries");
  if (q == 0) return EXPO_OK;
  if (S < 1 || S > kProxyMaxS) return fail(EXPO_E_BADARG, "1 <= S <= 4096 required");
  if (n == 0) return fail(EXPO_E_BADARG, "windows need images (n == 0)");
  if (!codes || !hs || !ws || !tables || !windows || !out) return fail(EXPO_E_BADARG, "null pointer");
  if ((reinterpret_cast<uintptr_t>(tables) & 3) != 0) return fail(EXPO_E_BADARG, "tables must be 4-byte aligned");
  for (int i = 0; i < n; ++i) {
    if (hs[i] < 1 || ws[i] < 1) return fail(EXPO_E_BADARG, "h >= 1, w >= 1 required");
    if (long(hs[i]) * ws[i] * channels * (code_bits / 8) > (1L << 31) - 8192)
      return fail(EXPO_E_BADARG, "the codes of one image must be smaller than 2 GiB");
    if (!codes[i]) return fail(EXPO_E_BADARG, "null image pointer");
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
  if (code_bits == 8)
    return bilinear_resize_codes_ct<uint8_t>(channels, table_dtype, out_dtype, codes, ws, tables, table_stride, windows, q,
                                             S, out, s);
  return bilinear_resize_codes_ct<uint16_t>(channels, table_dtype, out_dtype, codes, ws, tables, table_stride, windows, q,
                                            S, out, s);
}

}  // extern "C"
