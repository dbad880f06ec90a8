// curve_segments.h -- the segment form of the Tone / Color curves for any cfg.curve_steps (see curve_generic.hip for
// the derivation): per-curve constants staged in LDS, the evaluation, and the block count of the kernels that keep
// private LDS accumulator columns.  Shared by curve_generic.hip and dispatch_curves.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exposure_hip.h"

namespace expo {

constexpr int kCgThreads = 256;
constexpr int kCgMaxSteps = EXPO_CURVE_MAX_STEPS;  // 16: 3 curves x (2 x 16 + 1) private slots x 257 floats = 99.7 KB of LDS
constexpr int kCgPad = kCgThreads + 1;

template <typename T> __device__ __forceinline__ float cg_load(const T* p, size_t i) { return float(p[i]); }
template <typename T> __device__ __forceinline__ void cg_store(T* p, size_t i, float v) { p[i] = T(v); }
template <> __device__ __forceinline__ void cg_store<_Float16>(_Float16* p, size_t i, float v) {
  p[i] = _Float16(fminf(fmaxf(v, -65504.0f), 65504.0f));  // fp16 stores saturate, like the tuned kernels'
}

struct CgCurve {  // per-curve constants in LDS
  float k[kCgMaxSteps], prefix[kCgMaxSteps], scale, inv_s;
};

__device__ __forceinline__ void cg_stage(const float* __restrict__ prm, int curves, int L, CgCurve* cv) {
  if (threadIdx.x < unsigned(curves)) {
    const float* k = prm + threadIdx.x * L;
    CgCurve& c = cv[threadIdx.x];
    float s = 0.f;
    for (int i = 0; i < L; ++i) {
      c.k[i] = k[i];
      c.prefix[i] = s;
      s += k[i];
    }
    s += 1e-30f;
    c.scale = float(L) / s;
    c.inv_s = 1.0f / s;
  }
  __syncthreads();
}

// T(x) * L / S through the segment form; also returns the segment and the offset inside it
__device__ __forceinline__ float cg_eval(const CgCurve& c, int L, float x, int* seg, float* off) {
  const float xc = fminf(fmaxf(x, 0.0f), 1.0f);
  int j = int(xc * float(L));
  j = j > L - 1 ? L - 1 : j;
  const float o = xc - float(j) / float(L);
  *seg = j;
  *off = o;
  return (c.prefix[j] / float(L) + o * c.k[j]) * c.scale;
}

inline int cg_blocks(int hw) {
  int b = (hw + kCgThreads * 8 - 1) / (kCgThreads * 8);  // ~8 pixels per thread
  return b < 1 ? 1 : (b > 256 ? 256 : b);
}

}  // namespace expo
