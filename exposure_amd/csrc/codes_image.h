// codes_image.h -- what the fused ragged passes that read the files' integer codes share (chain_fused_codes.hip,
// chain_fused_curves_codes.hip): the by-value table of a launch with its `fill`, the loader of
// one image and the codes' own argument checks; the launches are ragged_launch.h's.  Include it after
// chain_fused.hip (EXPO_CHAIN_FUSED_TEMPLATES_ONLY), whose PixTraits and stores it uses; the step loop is the including
// unit's (`run`).
//   vector path       a lane's group keeps pixel_io.h's pixel positions: row r of a wave's chunk is the 12-byte vector
//                     of PPV pixels (fp16 2, fp32 1) at pixel gw * PPL + r * 64 * PPV + lane * PPV; its PPV * C codes
//                     come in with the widest buffer load their size allows, as decode_kernel's.  Rows past the end of
//                     the image read code 0 and their stores are dropped by the bounds checks.
//   element-wise path per image, block-uniform: the vec bit of §3.31 with the codes' base among the addresses.
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

// ragged_launches' `fill` (ragged_launch.h) for a codes pass: the codes' base joins the alignment test.  FMT kTapNone:
// taps unused; ys NULL = no image output.
template <typename T, int FMT>
auto codes_fill(const void* const* codes, void* const* ys, const int* hs, const int* ws, void* const* taps) {
  return [=](CodesTable<T>& tab, int j, int i) {
    tab.codes[j] = codes[i];
    tab.y[j] = ys ? static_cast<T*>(ys[i]) : nullptr;
    tab.taps[j] = FMT == kTapNone ? nullptr : static_cast<char*>(taps[i]);
    tab.hw[j] = hs[i] * ws[i];
    return ragged_addr(codes[i]) | ragged_addr(tab.y[j]) | (tap_vector_store<T, FMT>() ? ragged_addr(tab.taps[j]) : 0);
  };
}

// the scalar checks of a codes pass, in front of ragged_check_args
inline int codes_check_scalars(int channels, int code_bits, int table_stride) {
  if (channels != 1 && channels != 3 && channels != 4) return fail(EXPO_E_BADARG, "channels must be 1, 3 or 4");
  if (code_bits != 8 && code_bits != 16) return fail(EXPO_E_BADARG, "code_bits must be 8 or 16");
  if (table_stride != 0 && table_stride < (1 << code_bits))
    return fail(EXPO_E_BADARG, "table_stride must be 0 (one shared table) or at least 2^code_bits entries");
  return EXPO_OK;
}

// the pointer-stage checks of a codes pass, ragged_check_args' `extra`: the tables' alignment (i < 0), the bytes of
// image i's codes
inline auto codes_check_extra(const void* tables, const int* hs, const int* ws, int channels, int code_bits) {
  return [=](int i) {
    if (i < 0)
      return (ragged_addr(tables) & 3) != 0 ? fail(EXPO_E_BADARG, "tables must be 4-byte aligned") : int(EXPO_OK);
    return long(hs[i]) * ws[i] * channels * (code_bits / 8) > (1L << 31) - 8192
               ? fail(EXPO_E_BADARG, "the codes of one image must be smaller than 2 GiB")
               : int(EXPO_OK);
  };
}

}  // namespace

}  // namespace expo
