// chain_steps_bwd_body.h -- what the two run kernels of expo_chain_bwd share: chain_steps_bwd.hip (every step's x is
// loaded) and chain_steps_bwd_rc.hip (the interior x of a run are recomputed from the lowest one).  The kernel
// arguments, one backward step on one group, a step's epilogue and the static run table.  chain_steps_bwd.hip's header
// says why each piece looks the way it does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "filter_math.h"
#include "pixel_io.h"
#include "kernel_common.h"
#include "stream_bodies.h"  // kAccParts, EXPO_BWD_MIN_WAVES

namespace expo {

// everything a launch needs, by value in the kernel arguments; slot k is step (head - k) of the chain
template <int NS>
struct ChainStepsBwdArgs {
  const void* dy;        // grads[head + 1], at the chunk's first image
  const void* x[NS];     // acts[head - k]
  void* dx[NS];          // grads[head - k]
  const float* prm[NS];  // the step's parameters, at the chunk's first image
  float* rec[NS];        // the step's record slice, at the chunk's first image
  int id[NS];
  int acc_at[NS];        // where the step's kAccParts * NACC accumulators start among a thread's acc_floats
  int acc_floats, hw;
};

// one step on one group: the data flow of bwd_body between its loads and its store.  The step's accumulators
// (bwd_body's acc = a[0] and part[p] = a[p + 1]) live in this thread's LDS column between two groups.
template <class F, typename T, int MODE>
__device__ __forceinline__ void run_step(const float* prm, const RawGroup& x, RawGroup& g, float* lds) {
  constexpr int PPL = PixTraits<T>::PPL;
  constexpr int kParts = kAccParts < PPL ? kAccParts : PPL;
  static_assert(!F::kHasGroupBwd && F::kLutFloats == 0, "element-wise filters only");
  const typename F::Prm q = F::load(prm);
  float a[kParts][F::NACC];
#pragma unroll
  for (int p = 0; p < kParts; ++p)
#pragma unroll
    for (int j = 0; j < F::NACC; ++j) a[p][j] = lds[(p * F::NACC + j) * kThreads];
  float v[PPL * 3], d[PPL * 3];
  unpack<T>(x, v);
  unpack<T>(g, d);
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    float dx[3];
    F::bwd(q, nullptr, v + 3 * k, d + 3 * k, dx, a[k % kParts], MODE);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[3 * k + c] = dx[c];
  }
  g = pack<T>(d);
#pragma unroll
  for (int p = 0; p < kParts; ++p)
#pragma unroll
    for (int j = 0; j < F::NACC; ++j) lds[(p * F::NACC + j) * kThreads] = a[p][j];
}

// bwd_body's epilogue for one step
template <class F, typename T>
__device__ __forceinline__ void run_reduce(const float* lds, float* rec) {
  constexpr int PPL = PixTraits<T>::PPL;
  constexpr int kParts = kAccParts < PPL ? kAccParts : PPL;
  float acc[F::NACC];
#pragma unroll
  for (int j = 0; j < F::NACC; ++j) acc[j] = lds[j * kThreads];
#pragma unroll
  for (int p = 0; p < kParts - 1; ++p)
#pragma unroll
    for (int j = 0; j < F::NACC; ++j) acc[j] += lds[((p + 1) * F::NACC + j) * kThreads];
  block_reduce_record<F::NACC>(acc, rec);
}

// The filters a run may hold -- a static table, decided by the GPU comparison against the per-step kernels
// (tests/test_hip_chain_bwd_runs.py) and not by the source: Contrast (5) and WNB (6) are NOT in it.  Their backwards
// hold a * b + c * d sums (lum3, the dy . x dot product) that the compiler may contract either way round, and it
// contracts them one way in filter_bwd_kernel (whose accumulators are loop-carried registers that the SLP vectoriser
// pairs, taking the sums with them) and the other way here: WNB's dparams differ in the last bits in both storage
// types, Contrast's dparams in fp16 and dparams and dx in fp32.  Exposure, Gamma, White balance, S+ and Level give the
// per-step bits at every run length 2..8, for every ordered pair of neighbouring filters, in both storage types and
// cache policies and in both run kernels (tests/test_hip_chain_bwd_pairs.py holds them to that, clamp edges and
// saturating values included) -- except S+ with hsv_grad_mode 1 in fp32 (its dx differs in 0.4 % of the values),
// which chain_steps_bwd_fusable keeps out as well.
#define EXPO_RUN_FILTERS(X) X(0, ExposureF) X(1, GammaF) X(2, WhiteBalanceF) X(3, SatPlusF) X(8, LevelF)

}  // namespace expo
