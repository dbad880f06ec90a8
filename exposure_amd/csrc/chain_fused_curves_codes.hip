// chain_fused_curves_codes.hip -- the fused ragged inference pass for ANY cfg.curve_steps L in [1, 16] straight from the
// integer codes of the image files (expo_chain_fused_curves_fwd_ragged_codes).  It is
// expo_chain_fused_fwd_ragged_codes (chain_fused_codes.hip, §3.23) with the step loop of
// expo_chain_fused_curves_fwd_ragged (chain_fused_curves.hip, §3.25): the input of image i is its codes plus its table
// in the storage dtype T, a pixel value enters the step loop as float(T table[code]), and Tone / Color evaluate L
// segments from parameter rows of EXPO_MAX_PARAMS_CURVES.  The outputs are bit-identical to decode + the pass from
// tensors, and the float input never exists.
//
// A unit of its own, compiled with exactly chain_fused.hip's flags (csrc/build.sh).  Nothing of the device code is its
// own but the kernel that joins the parts: chain_fused.hip (EXPO_CHAIN_FUSED_TEMPLATES_ONLY) gives chain_step, TapSink
// and the stores, curves_run.h the step loop and the per-wave curve table, codes_image.h the table of a launch and the
// loader with its vector and element-wise paths; the host side of a call is ragged_launch.h's.
//   tables      an 8-bit table is staged in LDS once per block; a 16-bit table is read through the caches as ttab[k],
//               a plain global load -- no pointer or value is pinned into a register by hand anywhere in this unit.
//   parameters  three scalars and the id per step in SGPRs, the knots through the lane-mirrored vector load
//               (curves_run.h), so the kernel holds fewer SGPRs than chain_fused_codes.hip's.
#define EXPO_CHAIN_FUSED_TEMPLATES_ONLY
#include "chain_fused.hip"
#include "curves_run.h"
#include "codes_image.h"

namespace expo {

namespace {

// kernel arguments: ids, params, steps, L, tap_mask, tables, table_stride, the table
static_assert(sizeof(CodesTable<half_t>) + 48 + sizeof(int) <= 4096,
              "the codes table must fit the 4 KB kernarg block alongside the curve steps");

// chain_fused_curves_image with the codes loader (codes_image_loop); Sink = NoSink: no taps
template <typename CT, int C, typename T, bool VEC, class IO, class Sink, class Look>
__device__ __forceinline__ void chain_fused_curves_codes_image(const int32_t* idn, const float* prn, int steps, int L,
                                                               const CT* codes, T* yi, int hw, int groups, int first_gw,
                                                               int stride, float2_lut* tab, const Sink& sink,
                                                               const Look& look) {
  constexpr bool kTaps = !std::is_same<Sink, NoSink>::value;
  const int lane = threadIdx.x & 63;
  const int plane = lane < EXPO_MAX_PARAMS_CURVES ? lane : EXPO_MAX_PARAMS_CURVES - 1;
  auto run = [&](float* v, int gw) {
    if constexpr (kTaps)
      chain_fused_curves_run<T>(idn, prn, steps, L, tab, plane, v, [&](int k, const float* o) { sink(k, gw, lane, o); });
    else
      chain_fused_curves_run<T>(idn, prn, steps, L, tab, plane, v);
  };
  codes_image_loop<CT, C, T, VEC, IO>(codes, yi, hw, groups, first_gw, stride, look, run);
}

// FMT: an EXPO_TAP_* format, or kTapNone (tap_mask == 0).  Both paths in every kernel: the choice is block-uniform.
template <typename CT, int C, typename T, class IO, int FMT>
__global__ __launch_bounds__(kThreads) void chain_fused_fwd_ragged_codes_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, int steps, int L, uint64_t tap_mask,
    const T* __restrict__ tables, int table_stride, const CodesTable<T> tab) {
  constexpr bool LDS = sizeof(CT) == 1;
  static_assert(!LDS || kThreads == 256, "one thread per entry of an 8-bit table");
  __shared__ float2_lut curve_tab[kWaves][kCurvesTabEntries];
  __shared__ __attribute__((aligned(4))) uint8_t tap_stage[kWaves][TapStage<T, FMT>::kBytes];
  __shared__ T lut[LDS ? 256 : 1];
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;  // the last image whose first block is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int i = __builtin_amdgcn_readfirstlane(lo);
  constexpr int PPL = PixTraits<T>::PPL;
  const T* ttab = tables + size_t(i) * size_t(table_stride);
  if constexpr (LDS) {  // before any wave leaves: every thread stages one entry
    lut[threadIdx.x] = ttab[threadIdx.x];
    __syncthreads();
  }
  auto look = [&](uint32_t k) -> T {
    if constexpr (LDS) return lut[k];
    else return ttab[k];
  };
  const int hw = tab.hw[i];
  const int groups = (hw + PPL - 1) / PPL;
  const int first_gw = (b - tab.first[i]) * kThreads + (threadIdx.x & ~63);
  const int stride = (tab.first[i + 1] - tab.first[i]) * kThreads;
  const int32_t* idn = ids + size_t(i) * steps;
  const float* prn = params + size_t(i) * steps * EXPO_MAX_PARAMS_CURVES;
  float2_lut* const curve = curve_tab[threadIdx.x >> 6];
  const CT* codes = static_cast<const CT*>(tab.codes[i]);
  auto image = [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    if constexpr (FMT == kTapNone) {
      chain_fused_curves_codes_image<CT, C, T, VEC, IO>(idn, prn, steps, L, codes, tab.y[i], hw, groups, first_gw, stride,
                                                        curve, NoSink(), look);
    } else {
      using Sink = TapSink<T, VEC, IO, FMT>;
      const Sink sink{tab.taps[i], size_t(hw) * 3 * Sink::ES, tap_mask, hw, tap_stage[threadIdx.x >> 6]};
      chain_fused_curves_codes_image<CT, C, T, VEC, IO>(idn, prn, steps, L, codes, tab.y[i], hw, groups, first_gw, stride,
                                                        curve, sink, look);
    }
  };
  if ((tab.vec >> i) & 1) image(std::true_type());
  else image(std::false_type());
}

// arguments validated by the caller; ys NULL = no image output.  The codes kernels hold both paths, so a launch does not
// look at any_slow.
template <typename CT, int C>
int chain_fused_curves_codes_t(int dtype, int tap_format, const int32_t* ids, const float* params, int steps, int L,
                               const void* const* codes, const void* tables, int table_stride, void* const* ys,
                               const int* hs, const int* ws, int n, uint64_t tap_mask, void* const* taps, hipStream_t s) {
  return dispatch_dtype_tap(dtype, tap_mask, tap_format, [&](auto t, auto fmt) {
    using T = decltype(t);
    constexpr int FMT = decltype(fmt)::value;
    return ragged_launches<T, CodesTable<T>>(
        hs, ws, n, codes_fill<T, FMT>(codes, ys, hs, ws, taps),
        [&](auto io, auto, dim3 grid, int base, const CodesTable<T>& tab) {
          hipLaunchKernelGGL((chain_fused_fwd_ragged_codes_kernel<CT, C, T, decltype(io), FMT>), grid, dim3(kThreads),
                             0, s, ids + size_t(base) * steps, params + size_t(base) * steps * EXPO_MAX_PARAMS_CURVES,
                             steps, L, tap_mask,
                             static_cast<const T*>(tables) + size_t(base) * size_t(table_stride), table_stride, tab);
          HIP_TRY(hipGetLastError(), "chain_fused_curves_fwd_ragged_codes launch");
          return EXPO_OK;
        });
  });
}

template <typename CT, typename... A>
int chain_fused_curves_codes_channels(int channels, A... a) {
  if (channels == 1) return chain_fused_curves_codes_t<CT, 1>(a...);
  if (channels == 3) return chain_fused_curves_codes_t<CT, 3>(a...);
  return chain_fused_curves_codes_t<CT, 4>(a...);
}

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

int expo_chain_fused_curves_fwd_ragged_codes(const int32_t* filter_ids, const float* params, int steps, int curve_steps,
                                             const void* const* codes, int channels, int code_bits, const void* tables,
                                             int table_stride, void* const* ys, const int* hs, const int* ws, int n,
                                             int dtype, uint64_t tap_mask, int tap_format, void* const* taps,
                                             void* stream) {
  if (curve_steps < 1 || curve_steps > kCurvesMaxL)
    return fail(EXPO_E_BADARG, "curve_steps must be in [1, EXPO_CURVE_MAX_STEPS]");
  if (int rc = codes_check_scalars(channels, code_bits, table_stride)) return rc;
  bool go;
  if (int rc = ragged_check_args(steps, codes, ys, true, hs, ws, n, dtype, tap_mask, tap_format, taps, tables != nullptr,
                                 filter_ids && params, &go, codes_check_extra(tables, hs, ws, channels, code_bits)))
    return rc;
  if (!go) return EXPO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (code_bits == 8)
    return chain_fused_curves_codes_channels<uint8_t>(channels, dtype, tap_format, filter_ids, params, steps, curve_steps,
                                                      codes, tables, table_stride, ys, hs, ws, n, tap_mask, taps, s);
  return chain_fused_curves_codes_channels<uint16_t>(channels, dtype, tap_format, filter_ids, params, steps, curve_steps,
                                                     codes, tables, table_stride, ys, hs, ws, n, tap_mask, taps, s);
}

}  // extern "C"
