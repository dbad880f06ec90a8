// chain_fused_codes.hip -- the fused ragged inference pass straight from the integer codes of the image files
// (expo_chain_fused_fwd_ragged_codes).  expo_chain_fused_fwd_ragged_taps with another loader: the
// input of image i is its codes (8 or 16 bits, 1, 3 or 4 channels, as the file holds them) plus its table in the
// storage dtype T (expo_decode_tables), and a pixel value enters the step loop as float(T table[code]) -- the very value
// the decoded tensor would have held, so the outputs are bit-identical to decode + pass and the float input never exists.
//
// A unit of its own, compiled with exactly chain_fused.hip's flags (csrc/build.sh): it includes that file for
// chain_fused_run, TapSink and the stores, which it uses untouched, and instantiates none of its kernels
// (EXPO_CHAIN_FUSED_TEMPLATES_ONLY), so the kernels of chain_fused.hip keep their code and registers and the two units
// compile side by side.  The only device code of its own is the loader below (the row load is codes_loader.h's).
// The table of a launch and the codes' own argument checks are codes_image.h's, shared with
// chain_fused_curves_codes.hip; the host side of a call is ragged_launch.h's.  The loader below is stated here and, word for word, as codes_image_loop in that header
// for the other unit: calling the header's from here moves this unit's instruction schedule, and its listing is held
// fixed.
//   tables            an 8-bit table is staged in LDS once per block (a block belongs to one image; 512 B / 1 KiB); a
//                     16-bit table (128 / 256 KiB per image) is read through the caches.
#define EXPO_CHAIN_FUSED_TEMPLATES_ONLY
#include "chain_fused.hip"
#include "codes_image.h"

namespace expo {

namespace {

// kernel arguments: ids, params, steps, tap_mask, tables, table_stride, the table
static_assert(sizeof(CodesTable<half_t>) + 48 <= 4096, "the codes table must fit the 4 KB kernarg block");

// chain_fused_image_taps with the codes loader; Sink = NoSink: no taps.  look(code) is the table gather.  yi may be
// NULL with taps.  One chunk per wave and trip, the next trip `stride` groups on (the ragged grid covers an image's
// groups in one trip).
template <typename CT, int C, typename T, bool VEC, class IO, class Sink, class Look>
__device__ __forceinline__ void chain_fused_codes_image(const int32_t* idn, const float* prn, int steps, const CT* codes,
                                                        T* yi, int hw, int groups, int first_gw, int stride,
                                                        float2_lut* tab, const Sink& sink, const Look& look) {
  constexpr int PPL = PixTraits<T>::PPL, PPV = VecTraits<T>::PPV;
  constexpr bool kTaps = !std::is_same<Sink, NoSink>::value;
  const int lane = threadIdx.x & 63;
  const int plane = lane % EXPO_MAX_PARAMS;
  auto run = [&](float* v, int gw) {
    if constexpr (kTaps)
      chain_fused_run<T>(idn, prn, steps, tab, plane, v, [&](int k, const float* o) { sink(k, gw, lane, o); });
    else
      chain_fused_run<T>(idn, prn, steps, tab, plane, v);
  };
  if constexpr (VEC) {
#if EXPO_FP16_OVFL
    // the fp16 stores (y and storage taps) saturate as in stream_groups
    if constexpr (sizeof(T) == 2) __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
#endif
    constexpr int NB = PPV * C * int(sizeof(CT));  // code bytes per lane-row
    const __amdgpu_buffer_rsrc_t rin =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<CT*>(codes), 0, hw * C * int(sizeof(CT)), kBufferRsrcFlags);
    const __amdgpu_buffer_rsrc_t ry = make_image_rsrc(yi, hw);
    for (int gw = first_gw; gw * PPL < hw; gw += stride) {  // wave-uniform
      CT c[4][PPV * C];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        load_code_row<CT, NB, IO::kLoadX>(rin, (gw * PPL + r * 64 * PPV + lane * PPV) * C * int(sizeof(CT)), c[r]);
      float v[PPL * 3];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int p = 0; p < PPV; ++p) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) v[(r * PPV + p) * 3 + ch] = float(look(c[r][p * C + (C == 1 ? 0 : ch)]));
        }
      }
      run(v, gw);
      if (yi) store_raw<IO::kStore>(ry, chunk_byte_offset<T>(gw, lane), pack<T>(v));
    }
  } else {
    for (int g0 = first_gw; g0 < groups; g0 += stride) {  // wave-uniform trip count, as chain_fused_image
      const int g = g0 + lane;
      float v[PPL * 3];
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int px = g * PPL + k;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          v[k * 3 + ch] = px < hw ? float(look(codes[size_t(px) * C + (C == 1 ? 0 : ch)])) : 0.0f;
      }
      run(v, g0);
      if (yi) store_slow<T>(yi, g, hw, v);
    }
  }
}

// FMT: an EXPO_TAP_* format, or kTapNone (tap_mask == 0).  Both paths in every kernel: the choice is block-uniform.
template <typename CT, int C, typename T, class IO, int FMT>
__global__ __launch_bounds__(kThreads) void chain_fused_fwd_ragged_codes_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, int steps, uint64_t tap_mask,
    const T* __restrict__ tables, int table_stride, const CodesTable<T> tab) {
  constexpr bool LDS = sizeof(CT) == 1;
  static_assert(!LDS || kThreads == 256, "one thread per entry of an 8-bit table");
  __shared__ float2_lut curve_tab[kWaves][32];
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
  const float* prn = params + size_t(i) * steps * EXPO_MAX_PARAMS;
  float2_lut* const curve = curve_tab[threadIdx.x >> 6];
  const CT* codes = static_cast<const CT*>(tab.codes[i]);
  auto image = [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    if constexpr (FMT == kTapNone) {
      chain_fused_codes_image<CT, C, T, VEC, IO>(idn, prn, steps, codes, tab.y[i], hw, groups, first_gw, stride, curve,
                                                 NoSink(), look);
    } else {
      using Sink = TapSink<T, VEC, IO, FMT>;
      const Sink sink{tab.taps[i], size_t(hw) * 3 * Sink::ES, tap_mask, hw, tap_stage[threadIdx.x >> 6]};
      chain_fused_codes_image<CT, C, T, VEC, IO>(idn, prn, steps, codes, tab.y[i], hw, groups, first_gw, stride, curve,
                                                 sink, look);
    }
  };
  if ((tab.vec >> i) & 1) image(std::true_type());
  else image(std::false_type());
}

// arguments validated by the caller; ys NULL = no image output.  The codes kernels hold both paths, so a launch does not
// look at any_slow.
template <typename CT, int C>
int chain_fused_codes_t(int dtype, int tap_format, const int32_t* ids, const float* params, int steps,
                        const void* const* codes, const void* tables, int table_stride, void* const* ys, const int* hs,
                        const int* ws, int n, uint64_t tap_mask, void* const* taps, hipStream_t s) {
  return dispatch_dtype_tap(dtype, tap_mask, tap_format, [&](auto t, auto fmt) {
    using T = decltype(t);
    constexpr int FMT = decltype(fmt)::value;
    return ragged_launches<T, CodesTable<T>>(
        hs, ws, n, codes_fill<T, FMT>(codes, ys, hs, ws, taps),
        [&](auto io, auto, dim3 grid, int base, const CodesTable<T>& tab) {
          hipLaunchKernelGGL((chain_fused_fwd_ragged_codes_kernel<CT, C, T, decltype(io), FMT>), grid, dim3(kThreads),
                             0, s, ids + size_t(base) * steps, params + size_t(base) * steps * EXPO_MAX_PARAMS, steps, tap_mask,
                             static_cast<const T*>(tables) + size_t(base) * size_t(table_stride), table_stride, tab);
          HIP_TRY(hipGetLastError(), "chain_fused_fwd_ragged_codes launch");
          return EXPO_OK;
        });
  });
}

template <typename CT, typename... A>
int chain_fused_codes_channels(int channels, A... a) {
  if (channels == 1) return chain_fused_codes_t<CT, 1>(a...);
  if (channels == 3) return chain_fused_codes_t<CT, 3>(a...);
  return chain_fused_codes_t<CT, 4>(a...);
}

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

int expo_chain_fused_fwd_ragged_codes(const int32_t* filter_ids, const float* params, int steps,
                                      const void* const* codes, int channels, int code_bits, const void* tables,
                                      int table_stride, void* const* ys, const int* hs, const int* ws, int n, int dtype,
                                      uint64_t tap_mask, int tap_format, void* const* taps, void* stream) {
  if (int rc = codes_check_scalars(channels, code_bits, table_stride)) return rc;
  bool go;
  if (int rc = ragged_check_args(steps, codes, ys, true, hs, ws, n, dtype, tap_mask, tap_format, taps, tables != nullptr,
                                 filter_ids && params, &go, codes_check_extra(tables, hs, ws, channels, code_bits)))
    return rc;
  if (!go) return EXPO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (code_bits == 8)
    return chain_fused_codes_channels<uint8_t>(channels, dtype, tap_format, filter_ids, params, steps, codes, tables,
                                               table_stride, ys, hs, ws, n, tap_mask, taps, s);
  return chain_fused_codes_channels<uint16_t>(channels, dtype, tap_format, filter_ids, params, steps, codes, tables,
                                              table_stride, ys, hs, ws, n, tap_mask, taps, s);
}

}  // extern "C"
