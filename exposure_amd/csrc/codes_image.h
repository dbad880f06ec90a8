// codes_image.h -- what the fused ragged passes that read the files' integer codes share (chain_fused_codes.hip,
// chain_fused_curves_codes.hip): the by-value table of a launch, the loader of one image and the
// split of a call into launches.  Include it after chain_fused.hip (EXPO_CHAIN_FUSED_TEMPLATES_ONLY), whose PixTraits,
// stores and ragged constants it uses; the step loop is the including unit's (`run`).
//   vector path       a lane's group keeps pixel_io.h's pixel positions: row r of a wave's chunk is the 12-byte vector
//                     of PPV pixels (fp16 2, fp32 1) at pixel gw * PPL + r * 64 * PPV + lane * PPV; its PPV * C codes
//                     come in with the widest buffer load their size allows, as decode_kernel's.  Rows past the end of
//                     the image read code 0 and their stores are dropped by the bounds checks.
//   element-wise path per image, block-uniform: codes not 4-byte aligned, hw % PPV != 0, or y / a vector-stored tap
//                     plane misaligned (the rule of chain_fused.hip with the codes' base added).
#pragma once
#include "codes_loader.h"

namespace expo {

namespace {

// up to 64 images by value in the kernel arguments (2 KB): codes, output (NULL: none), tap buffer, pixel count, first
// block of each image (first[n] = the grid's size) and a bit per image for the vector path
template <typename T>
struct CodesTable {
  const void* codes[kRaggedMaxImages];
  T* y[kRaggedMaxImages];
  char* taps[kRaggedMaxImages];
  int hw[kRaggedMaxImages];
  int first[kRaggedMaxImages + 1];
  int n;
  uint64_t vec;
};

// One image of a codes pass: look(code) is the table gather, run(v, gw) the step loop on a lane's PPL pixels (it feeds
// the taps, if any).  yi may be NULL with taps.  One chunk per wave and trip, the next trip `stride` groups on (the
// ragged grid covers an image's groups in one trip).
template <typename CT, int C, typename T, bool VEC, class IO, class Look, class Run>
__device__ __forceinline__ void codes_image_loop(const CT* codes, T* yi, int hw, int groups, int first_gw, int stride,
                                                 const Look& look, const Run& run) {
  constexpr int PPL = PixTraits<T>::PPL, PPV = VecTraits<T>::PPV;
  const int lane = threadIdx.x & 63;
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

// The launches of one call (arguments validated by the caller): at most kRaggedMaxImages images each, the cache policy
// from the bytes of the whole call, as the pass from tensors.  `width` is the floats of a parameter row;
// launch(stream, grid, ids, params, tables, tab) enqueues one.  FMT kTapNone: taps unused; ys NULL = no image output.
template <typename T, int FMT, class Launch>
int codes_launches(const int32_t* ids, const float* params, int steps, int width, const void* const* codes,
                   const void* tables, int table_stride, void* const* ys, const int* hs, const int* ws, int n,
                   void* const* taps, const char* what, const Launch& launch) {
  constexpr int PPL = PixTraits<T>::PPL;
  long bytes = 0;
  for (int i = 0; i < n; ++i) bytes += long(hs[i]) * ws[i] * 3L * long(sizeof(T));
  const bool stream = bytes >= stream_min_bytes();
  for (int base = 0; base < n; base += kRaggedMaxImages) {
    const int m = n - base < kRaggedMaxImages ? n - base : kRaggedMaxImages;
    CodesTable<T> tab = {};
    tab.n = m;
    long blocks = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j, hw = hs[i] * ws[i];
      tab.codes[j] = codes[i];
      tab.y[j] = ys ? static_cast<T*>(ys[i]) : nullptr;
      tab.taps[j] = FMT == kTapNone ? nullptr : static_cast<char*>(taps[i]);
      tab.hw[j] = hw;
      tab.first[j] = int(blocks);
      blocks += ((hw + PPL - 1) / PPL + kThreads - 1) / kThreads;
      const uintptr_t a = reinterpret_cast<uintptr_t>(codes[i]) | reinterpret_cast<uintptr_t>(tab.y[j]) |
                          (tap_vector_store<T, FMT>() ? reinterpret_cast<uintptr_t>(tab.taps[j]) : 0);
      if (hw % VecTraits<T>::PPV == 0 && (a & 3) == 0) tab.vec |= uint64_t(1) << j;
    }
    if (blocks > 0x7fffffffL) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    tab.first[m] = int(blocks);
    launch(stream, dim3(static_cast<unsigned>(blocks)), ids + size_t(base) * steps,
           params + size_t(base) * steps * width, static_cast<const T*>(tables) + size_t(base) * size_t(table_stride),
           tab);
    HIP_TRY(hipGetLastError(), what);
  }
  return EXPO_OK;
}

// the checks of a codes pass that do not depend on its step loop, all before the first launch; EXPO_OK with *go = false:
// nothing to do (n == 0)
inline int codes_check_args(const int32_t* filter_ids, const float* params, int steps, const void* const* codes,
                            int channels, int code_bits, const void* tables, int table_stride, void* const* ys,
                            const int* hs, const int* ws, int n, int dtype, uint64_t tap_mask, int tap_format,
                            void* const* taps, bool* go) {
  *go = false;
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (dtype != EXPO_F16 && dtype != EXPO_F32) return fail(EXPO_E_BADDTYPE, "dtype must be EXPO_F16 or EXPO_F32");
  if (channels != 1 && channels != 3 && channels != 4) return fail(EXPO_E_BADARG, "channels must be 1, 3 or 4");
  if (code_bits != 8 && code_bits != 16) return fail(EXPO_E_BADARG, "code_bits must be 8 or 16");
  if (table_stride != 0 && table_stride < (1 << code_bits))
    return fail(EXPO_E_BADARG, "table_stride must be 0 (one shared table) or at least 2^code_bits entries");
  if (steps < 0 || steps > 64) return fail(EXPO_E_BADARG, "steps must be in [0, 64]");
  if (int rc = check_taps(steps, tap_mask, tap_format)) return rc;
  if (!ys && !tap_mask) return fail(EXPO_E_BADARG, "nothing to write (ys NULL and tap_mask 0)");
  if (n == 0) return EXPO_OK;
  if (!codes || !tables || !hs || !ws || (tap_mask && !taps) || (steps > 0 && (!filter_ids || !params)))
    return fail(EXPO_E_BADARG, "null pointer");
  if ((reinterpret_cast<uintptr_t>(tables) & 3) != 0) return fail(EXPO_E_BADARG, "tables must be 4-byte aligned");
  for (int i = 0; i < n; ++i) {
    if (int rc = check_common(1, hs[i], ws[i], dtype)) return rc;
    if (long(hs[i]) * ws[i] * channels * (code_bits / 8) > (1L << 31) - 8192)
      return fail(EXPO_E_BADARG, "the codes of one image must be smaller than 2 GiB");
    if (!codes[i] || (ys && !ys[i])) return fail(EXPO_E_BADARG, "null image pointer");
    if (tap_mask && !taps[i]) return fail(EXPO_E_BADARG, "null tap pointer");
  }
  *go = true;
  return EXPO_OK;
}

}  // namespace

}  // namespace expo
