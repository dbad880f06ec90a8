// stream_bodies.h -- the per-image bodies of the streaming kernels (forward, backward, zero fill), shared by the
// translation units that put them behind a kernel of their own: exposure_hip.hip (per-filter and per-image dispatch
// kernels) and dispatch_curves.hip (the dispatch for any cfg.curve_steps).  Both compile them with the same flags, so a
// body gives the same bits wherever it is launched from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "filter_math.h"
#include "pixel_io.h"
#include "kernel_common.h"

// Compile-time structure of the streaming kernels (each alternative was measured and rejected, see
// profiles/r02_experiments.md): forward waves own exactly one chunk and do not prefetch; backward waves walk
// block-strided chunks with a one-deep software prefetch; the forward's per-image constants are fetched after
// the first chunk's loads have been issued.
#ifndef EXPO_BWD_MIN_WAVES
#define EXPO_BWD_MIN_WAVES  // e.g. -DEXPO_BWD_MIN_WAVES=,5 : a register budget for 5 waves per SIMD (probe builds)
#endif
#ifndef EXPO_CURVE_BWD_PREFETCH
#define EXPO_CURVE_BWD_PREFETCH 1  // (probe builds: the curve backward without its one-deep software prefetch)
#endif
constexpr bool kFwdPrefetch = false;
constexpr bool kBwdPrefetch = true;
constexpr int kAccParts = 4;  // partial sums per thread in the element-wise backward (1 / 2 / 4 measured, r02p27)

namespace expo {

// --------------------------------------------------------------------------- forward
template <class F, typename T, bool VEC, bool PEN, class IO = IoCached>
__device__ __forceinline__ void fwd_body(const T* __restrict__ xi, T* __restrict__ yi,
                                         const float* __restrict__ prm, float* __restrict__ rec,
                                         int hw, int groups) {
  constexpr int PPL = PixTraits<T>::PPL;
  // On the vector path the per-image constants are fetched AFTER the first chunk's loads have been issued
  // (stream_groups' prologue): the dependent scalar loads (kernel argument -> parameter -> exp2) otherwise sit
  // in front of the image loads of every wave, and a forward wave lives for exactly one chunk.
  typename F::Prm q;
  if constexpr (!VEC) q = F::load(prm);
  float pen = 0.f;
  const int stride = gridDim.x * kThreads;
  // Tone / Color on the vector path (all lanes of a wave alive): segment table instead of the
  // telescoped min/fma chain; built once per wave behind the first loads (stream_groups' prologue)
  constexpr bool kCurveTab = VEC && F::kLutFloats > 0;
  constexpr int kNC = kCurveTab ? F::NP / kCurveSteps : 1;
  __shared__ float2_lut ftab[kCurveTab ? kWaves : 1][32];
  float2_lut* const tab = ftab[kCurveTab ? (threadIdx.x >> 6) : 0];
  // per-group work, shared by the prefetching (VEC) and the element-wise loop
  auto compute = [&](float* v, int g) {
    if constexpr (kCurveTab) {
      curve_lut_apply<kNC, PPL>(v, tab);
      if constexpr (PEN) {
#pragma unroll
        for (int j = 0; j < PPL * 3; ++j) {
          const float o = fmaxf(v[j] - 1.0f, 0.0f);
          pen = fmaf(o, o, pen);
        }
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      float y[3];
      F::fwd(q, v + 3 * k, y);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[3 * k + c] = y[c];
        if constexpr (PEN) {
          // padding pixels are x = 0, and f(0) <= 1 for every filter, so they add nothing
          const float o = fmaxf(y[c] - 1.0f, 0.0f);
          pen = fmaf(o, o, pen);
        }
      }
    }
  };
  if constexpr (VEC) {
    const T* const ins[1] = {xi};
    stream_groups<T, 1, true, kFwdPrefetch, IO>(
        ins, yi, hw, blockIdx.x * kThreads + (threadIdx.x & ~63), stride,
        [&](float (&v)[1][PPL * 3], int g) { compute(v[0], g); },
        [&]() {
          q = F::load(prm);
          if constexpr (kCurveTab) curve_lut_build<kNC>(prm[(threadIdx.x & 63) % F::NP], tab);
        });
  } else {
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
      float v[PPL * 3];
      load_slow<T>(xi, g, hw, v);
      compute(v, g);
      store_slow<T>(yi, g, hw, v);
    }
  }
  if constexpr (PEN) {
    float a[1] = {pen};
    block_reduce_record<1>(a, rec);  // finish_kernel: penalty[n] = sum * inv_count
  }
}

// -------------------------------------------------------------------------- backward
template <class F, typename T, bool VEC, bool HAS_DX, bool PEN, int MODE, class IO = IoCached>
__device__ __forceinline__ void bwd_body(const T* __restrict__ xi, const T* __restrict__ dyi,
                                         T* __restrict__ dxi, const float* __restrict__ prm,
                                         float* __restrict__ rec, int hw, int groups, float pen_scale) {
  constexpr int PPL = PixTraits<T>::PPL;
  const typename F::Prm q = F::load(prm);
  // per-image curve LUT (Tone / Color backward) staged in LDS once per block
  __shared__ __attribute__((aligned(16))) float lut[F::kLutFloats > 0 ? F::kLutFloats : 4];
  // fp16-exact fast path of the curve filters (bit-pattern LUT + packed accumulators).  With the fused penalty
  // dy stays an fp16 value and the penalty's addend travels beside it (CurveF::bwd_group<.., HAS_PEN>); the
  // masked path scales dy -> generic path there.
  constexpr bool kF16X = std::is_same<T, half_t>::value;
  // staged AFTER the first chunk's loads are in flight on the vector path (stream_groups' prologue)
  // fp16 vector path: the table is built from a per-lane copy of the parameters, fetched HERE -- before the first
  // image loads are issued -- so that nothing in the staging waits behind them (CurveF::stage16_lanes)
  constexpr bool kLaneStage = F::kLutFloats > 0 && kF16X && VEC;
  float klane = 0.f;
  if constexpr (kLaneStage) klane = prm[(threadIdx.x & 63) % F::NP];
  auto stage_lut = [&]() {
    if constexpr (F::kLutFloats > 0) {
      if constexpr (kLaneStage) F::stage16_lanes(klane, lut);
      else F::template stage_for<kF16X>(prm, lut);
      __syncthreads();
    }
  };
  if constexpr (!VEC) stage_lut();
  // fused penalty of the curve filters on the vector path: the forward is re-evaluated through the per-wave
  // segment table of the forward kernels (5 VALU + one LDS read per element instead of 16 VALU), and not at all
  // for an image whose curve cannot exceed 1 (curve_can_exceed_one -- every image under the reference's ranges)
  constexpr bool kPenTab = PEN && VEC && F::kLutFloats > 0;
  constexpr int kNC = kPenTab ? F::NP / kCurveSteps : 1;
  __shared__ float2_lut ptab[kPenTab ? kWaves : 1][32];
  float2_lut* const tab = ptab[kPenTab ? (threadIdx.x >> 6) : 0];
  bool pen_live = PEN;
  if constexpr (kPenTab) {
    pen_live = curve_can_exceed_one<kNC>(prm);
    if (pen_live) curve_lut_build<kNC>(prm[(threadIdx.x & 63) % F::NP], tab);
  }
  float acc[F::NACC];
#pragma unroll
  for (int j = 0; j < F::NACC; ++j) acc[j] = 0.f;
  // element-wise filters: the pixels of a group feed kAccParts independent partial sums, so a group's 24
  // accumulator updates are not one dependent chain (Exposure / Gamma / S+ / Contrast / WNB keep ONE accumulator)
  constexpr int kParts = F::kHasGroupBwd ? 1 : (kAccParts < PPL ? kAccParts : PPL);
  float part[kParts > 1 ? kParts - 1 : 1][F::NACC];
#pragma unroll
  for (int p = 0; p < (kParts > 1 ? kParts - 1 : 1); ++p)
#pragma unroll
    for (int j = 0; j < F::NACC; ++j) part[p][j] = 0.f;
  const int stride = gridDim.x * kThreads;
  auto compute = [&](float* v, float* d, int g) {
    if constexpr (kPenTab) {
      // plain group backward on dy, then the penalty's share as a fix-up (block-uniform: only for an image whose
      // curve can exceed 1; element-wise: only where y > 1)
      F::template bwd_group<PPL, kF16X, false>(q, lut, v, d, acc, nullptr);
      if (pen_live) F::template bwd_pen_fixup<PPL, kF16X>(lut, tab, v, d, acc, pen_scale);
      return;
    }
    float pen[PEN ? PPL * 3 : 1];
    if constexpr (PEN) {
      // fused over-exposure penalty: dy += 2 max(y-1,0) * dpen / (H W 3)
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        float y[3];
        F::fwd(q, v + 3 * k, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {  // padding pixels: y = f(0) <= 1 -> no contribution
          pen[3 * k + c] = fmaxf(y[c] - 1.0f, 0.0f) * pen_scale;
          if constexpr (!F::kHasGroupBwd) d[3 * k + c] += pen[3 * k + c];
        }
      }
    }
    if constexpr (F::kHasGroupBwd) {
      F::template bwd_group<PPL, kF16X, PEN>(q, lut, v, d, acc, pen);
    } else {
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        float dx[3];
        F::bwd(q, lut, v + 3 * k, d + 3 * k, dx, (k % kParts == 0) ? acc : part[(k % kParts + kParts - 1) % kParts], MODE);
#pragma unroll
        for (int c = 0; c < 3; ++c) d[3 * k + c] = dx[c];
      }
    }
  };
  if constexpr (VEC) {
    const T* const ins[2] = {xi, dyi};
    constexpr bool kPf = (F::kLutFloats > 0 && !PEN) ? bool(EXPO_CURVE_BWD_PREFETCH) : kBwdPrefetch;
    stream_groups<T, 2, HAS_DX, kPf, IO>(ins, dxi, hw, blockIdx.x * kThreads + (threadIdx.x & ~63), stride,
                                         [&](float (&v)[2][PPL * 3], int g) { compute(v[0], v[1], g); }, stage_lut);
  } else {
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
      float v[PPL * 3], d[PPL * 3];
      load_slow<T>(xi, g, hw, v);
      load_slow<T>(dyi, g, hw, d);
      compute(v, d, g);
      if constexpr (HAS_DX) store_slow<T>(dxi, g, hw, d);
    }
  }
  if constexpr (kParts > 1) {
#pragma unroll
    for (int p = 0; p < kParts - 1; ++p)
#pragma unroll
      for (int j = 0; j < F::NACC; ++j) acc[j] += part[p][j];
  }
  block_reduce_record<F::NACC>(acc, rec);  // finish_kernel applies F::finish_one to the image totals
}

// y = 0 for a whole image (filter id -1 in the per-image dispatch entry points)
template <typename T, bool VEC, class IO = IoCached>
__device__ __forceinline__ void zero_image(T* __restrict__ yi, int hw, int groups) {
  constexpr int PPL = PixTraits<T>::PPL;
  float z[PPL * 3];
#pragma unroll
  for (int j = 0; j < PPL * 3; ++j) z[j] = 0.f;
  const int stride = gridDim.x * kThreads;
  if constexpr (VEC) {
    const RawGroup rz = pack<T>(z);
    const __amdgpu_buffer_rsrc_t ry = make_image_rsrc(yi, hw);
    for (int gw = blockIdx.x * kThreads + (threadIdx.x & ~63); gw * PPL < hw; gw += stride)
      store_raw<IO::kStore>(ry, chunk_byte_offset<T>(gw, threadIdx.x & 63), rz);
  } else {
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) store_slow<T>(yi, g, hw, z);
  }
}

}  // namespace expo
