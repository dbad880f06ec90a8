// chain_fused_curves.hip -- the fused ragged inference pass for ANY cfg.curve_steps L in [1, 16]
// (expo_chain_fused_curves_fwd_ragged).  expo_chain_fused_fwd_ragged_taps with two other curve steps:
// Tone (id 4) and Color (id 7) evaluate
//   y = (L/S) sum_i clip(x - i/L, 0, 1/L) k_i,  S = sum_i k_i + 1e-30
// for a runtime, wave-uniform L instead of the compile-time 8 of filter_math.h, so a parameter row is
// EXPO_MAX_PARAMS_CURVES = 3 * 16 floats wide (Tone: k_0..k_{L-1}; Color: channel * L + knot).  Every other step is
// chain_step's body of chain_fused.hip.
//
// A unit of its own, compiled with exactly chain_fused.hip's flags (csrc/build.sh): it includes that file for
// chain_step, TapSink, the ragged tables and the stores, which it uses untouched, and instantiates none of its kernels
// (EXPO_CHAIN_FUSED_TEMPLATES_ONLY), so the kernels of chain_fused.hip keep their code and registers.  The host side
// of a call is ragged_launch.h's, with chain_fused.hip's fills.
//   parameters  chain_fused_run keeps two sets of 24 parameters in SGPRs; two sets of 48 do not fit.  The filters that
//               are no curve read at most three scalars, so only a row's first three entries (and the id) are fetched
//               one step ahead through scalar loads; a curve step's knots arrive in a lane-mirrored vector load
//               (lane l <-> entry l, requested one step ahead as well) and never touch an SGPR.
//   table       per curve and segment j the line y = a x^ + b of curve_lut_build (kernel_common.h), with L + 1 entries
//               per curve (entry L repeats L - 1: x^ == 1 needs no index clamp): at most 3 * 17 float2 per wave in LDS,
//               built once per wave and curve step -- a segmented cross-lane scan (four shuffles) gives the prefix
//               sums -- for the 24 values a lane maps through it: clamp, mul, cvt, address, ds_read_b64, fma per value,
//               whatever L is.  The segment is j = min(int(L x^), L - 1), as curve_generic.hip's.
#define EXPO_CHAIN_FUSED_TEMPLATES_ONLY
#include "chain_fused.hip"
#include "curves_run.h"

namespace expo {

namespace {

// chain_fused_image (Sink = NoSink: stream_groups stores y) / chain_fused_image_taps (yi may be NULL) with the step
// loop above
template <typename T, bool VEC, class IO, class Sink>
__device__ __forceinline__ void chain_fused_curves_image(const int32_t* idn, const float* prn, int steps, int L,
                                                         const T* xi, T* yi, int hw, int groups, int first_gw,
                                                         int stride, float2_lut* tab, const Sink& sink) {
  constexpr int PPL = PixTraits<T>::PPL;
  constexpr bool kTaps = !std::is_same<Sink, NoSink>::value;
  const int lane = threadIdx.x & 63;
  const int plane = lane < EXPO_MAX_PARAMS_CURVES ? lane : EXPO_MAX_PARAMS_CURVES - 1;
  auto run = [&](float* v, int gw) {
    if constexpr (kTaps)
      chain_fused_curves_run<T>(idn, prn, steps, L, tab, plane, v, [&](int k, const float* o) { sink(k, gw, lane, o); });
    else
      chain_fused_curves_run<T>(idn, prn, steps, L, tab, plane, v);
  };
  if constexpr (VEC) {
    const T* const ins[1] = {xi};
    if constexpr (kTaps) {
#if EXPO_FP16_OVFL
      // the fp16 stores (y and storage taps) saturate as in stream_groups, which sets this only when it stores itself
      if constexpr (sizeof(T) == 2) __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
#endif
      const __amdgpu_buffer_rsrc_t ry = make_image_rsrc(yi, hw);
      stream_groups<T, 1, false, true, IO>(ins, nullptr, hw, first_gw, stride, [&](float (&v)[1][PPL * 3], int g) {
        const int gw = g - lane;
        run(v[0], gw);
        if (yi) store_raw<IO::kStore>(ry, chunk_byte_offset<T>(gw, lane), pack<T>(v[0]));
      });
    } else {
      stream_groups<T, 1, true, false, IO>(ins, yi, hw, first_gw, stride,
                                           [&](float (&v)[1][PPL * 3], int g) { run(v[0], g - lane); });
    }
  } else {
    for (int g0 = first_gw; g0 < groups; g0 += stride) {  // wave-uniform trip count: the table builds need every lane
      const int g = g0 + lane;
      float v[PPL * 3];
      load_slow<T>(xi, g, hw, v);
      run(v, g0);
      if (!kTaps || yi) store_slow<T>(yi, g, hw, v);
    }
  }
}

// FMT kTapNone: the table of chain_fused_fwd_ragged_kernel, otherwise the one with a tap buffer per image
template <typename T, int FMT>
using CurvesTable = typename std::conditional<FMT == kTapNone, RaggedTable<T>, RaggedTapTable<T>>::type;

template <typename T, class IO, bool ANY_SLOW, int FMT>
__global__ __launch_bounds__(kThreads) void chain_fused_curves_ragged_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, int steps, int L, uint64_t tap_mask,
    const CurvesTable<T, FMT> tt) {
  __shared__ float2_lut curve_tab[kWaves][kCurvesTabEntries];
  __shared__ __attribute__((aligned(4))) uint8_t tap_stage[kWaves][TapStage<T, FMT>::kBytes];
  const RaggedTable<T>& tab = [&]() -> const RaggedTable<T>& {
    if constexpr (FMT == kTapNone) return tt;
    else return tt.t;
  }();
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;  // the last image whose first block is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int i = __builtin_amdgcn_readfirstlane(lo);
  constexpr int PPL = PixTraits<T>::PPL;
  const int hw = tab.hw[i];
  const int groups = (hw + PPL - 1) / PPL;
  const int first_gw = (b - tab.first[i]) * kThreads + (threadIdx.x & ~63);
  const int stride = (tab.first[i + 1] - tab.first[i]) * kThreads;
  const int32_t* idn = ids + size_t(i) * steps;
  const float* prn = params + size_t(i) * steps * EXPO_MAX_PARAMS_CURVES;
  float2_lut* const lut = curve_tab[threadIdx.x >> 6];
  auto image = [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    if constexpr (FMT == kTapNone) {
      chain_fused_curves_image<T, VEC, IO>(idn, prn, steps, L, tab.x[i], tab.y[i], hw, groups, first_gw, stride, lut,
                                           NoSink());
    } else {
      using Sink = TapSink<T, VEC, IO, FMT>;
      const Sink sink{tt.taps[i], size_t(hw) * 3 * Sink::ES, tap_mask, hw, tap_stage[threadIdx.x >> 6]};
      chain_fused_curves_image<T, VEC, IO>(idn, prn, steps, L, tab.x[i], tab.y[i], hw, groups, first_gw, stride, lut,
                                           sink);
    }
  };
  if (!ANY_SLOW || ((tab.vec >> i) & 1)) image(std::true_type());
  else image(std::false_type());
}

// arguments validated by the caller; FMT kTapNone: tap_mask == 0 and taps unused; otherwise ys NULL = no image output
template <typename T, int FMT>
int chain_fused_curves_ragged_t(const int32_t* ids, const float* params, int steps, int L, const void* const* xs,
                                void* const* ys, const int* hs, const int* ws, int n, uint64_t tap_mask,
                                void* const* taps, hipStream_t s) {
  const auto fill = [&] {
    if constexpr (FMT == kTapNone) return ragged_fill<T>(xs, ys, hs, ws);
    else return ragged_taps_fill<T, FMT>(xs, ys, hs, ws, taps);
  }();
  return ragged_launches<T, CurvesTable<T, FMT>>(
      hs, ws, n, fill, [&](auto io, auto any_slow, dim3 grid, int base, const CurvesTable<T, FMT>& tt) {
        hipLaunchKernelGGL((chain_fused_curves_ragged_kernel<T, decltype(io), decltype(any_slow)::value, FMT>), grid,
                           dim3(kThreads), 0, s, ids + size_t(base) * steps,
                           params + size_t(base) * steps * EXPO_MAX_PARAMS_CURVES, steps, L, tap_mask, tt);
        HIP_TRY(hipGetLastError(), "chain_fused_curves_fwd_ragged launch");
        return EXPO_OK;
      });
}

// kernel arguments: ids, params, steps, L, tap_mask, the table
static_assert(sizeof(RaggedTapTable<half_t>) + 40 <= 4096, "the ragged tap table must fit the 4 KB kernarg block");

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

int expo_chain_fused_curves_fwd_ragged(const int32_t* filter_ids, const float* params, int steps, int curve_steps,
                                       const void* const* xs, void* const* ys, const int* hs, const int* ws, int n,
                                       int dtype, uint64_t tap_mask, int tap_format, void* const* taps, void* stream) {
  if (curve_steps < 1 || curve_steps > kCurvesMaxL)
    return fail(EXPO_E_BADARG, "curve_steps must be in [1, EXPO_CURVE_MAX_STEPS]");
  bool go;
  if (int rc = ragged_check_args(steps, xs, ys, true, hs, ws, n, dtype, tap_mask, tap_format, taps, true,
                                 filter_ids && params, &go))
    return rc;
  if (!go) return EXPO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dispatch_dtype_tap(dtype, tap_mask, tap_format, [&](auto t, auto fmt) {
    return chain_fused_curves_ragged_t<decltype(t), decltype(fmt)::value>(filter_ids, params, steps, curve_steps, xs, ys,
                                                                          hs, ws, n, tap_mask, taps, s);
  });
}

}  // extern "C"
