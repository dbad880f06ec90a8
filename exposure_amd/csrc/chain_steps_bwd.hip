// chain_steps_bwd.hip -- consecutive element-wise steps of expo_chain_bwd in ONE launch, bit-identical to the per-step
// kernels.
//
// A chain's backward launches one filter_bwd_kernel per step: step i reads acts[i] and grads[i + 1] and writes
// grads[i], and step i - 1 reads back what step i has just written.  expo_chain_bwd knows every id and pointer before
// its first launch, so these re-reads are work the result does not need: for a RUN of consecutive element-wise steps
// (ids 0, 1, 2, 3, 8 -- element-wise steps, whose per-step kernels share the kGeomReduce geometry; Contrast and WNB
// are element-wise too but stay out, see EXPO_RUN_FILTERS below) this kernel loads a
// 48-byte group of the run head's dy once, applies the steps' backwards one after the other while the gradient sits in
// registers, and stores every intermediate grads[k] on the way (the ABI hands each one back).  A run of c steps moves
// c x + 1 dy + c dx passes instead of 3 c.  Tone / Color keep their own geometry and their per-step launches.
//
// Geometry: exactly filter_bwd_kernel's for kGeomReduce of the whole batch -- the same blocks_x, grid (blocks_x, np),
// block-strided wave walk and IoStream / IoCached choice.  A thread owns the groups it owns in a per-step launch, in
// stream_groups' order (also where a thread walks several: images above kMaxReduceBlocksX * kThreads groups, tensors
// of 256 MiB or more at four groups per thread), so every per-thread sum has the per-step kernel's addends in its order.
//
// Why the bits do not change, and how each trap of the surrounding code is handled:
//  * Rounding between steps.  The gradient travels PACKED (chain_steps.hip explains the v_fma_mix* against
//    v_fma_f32 + v_cvt_pk_f16_f32 mixture): every step is unpack<T> -> F::load + F::bwd with MODE, the calls bwd_body
//    makes -> pack<T>; those registers are stored and the next step continues from unpack<T> of them, the value a
//    reload would return.  MODE.FP16_OVFL is set as stream_groups sets it.  Compiled with exposure_hip.hip's flags.
//  * A body compiled without its dx store rounds its dparams differently (Contrast / WNB / Level): every step of a run
//    computes AND stores dx; the host keeps a step with grads[i] == NULL out of runs.  That was not enough for
//    Contrast and WNB: they are excluded by the static table at EXPO_RUN_FILTERS, which says why.
//  * Accumulators.  Each step keeps its own acc and kAccParts - 1 partial sums with bwd_body's k % kParts assignment,
//    folds them in bwd_body's order and ends in block_reduce_record<F::NACC> on its own record slice.
//  * block_reduce_record keeps its scratch in a function-static __shared__ array that two steps with the same NACC
//    share: consecutive reductions are separated by a __syncthreads(), and the epilogue is outside every
//    work-dependent branch, so all waves -- the ones without a group too -- reach every barrier.
//  * Gradient buffers may alias (two ping-pong buffers: the run's input is also the buffer of grads[head - 1]).  No
//    __restrict__ on them; a thread loads a group's dy (for the prefetched next group too) before it stores anything
//    to that group's offsets, and no other thread touches those bytes.
//  * The per-step kernels are not touched: this unit only includes the shared headers.
//
// Resources.  The kernel is instantiated per run length NS (2..8) and its step loop is ROLLED (a block-uniform switch
// on the id: one copy of each filter's body per kernel).  A first version unrolled the loop by template so that every
// slot's accumulators were registers of their own: 176..256 VGPRs plus up to 132 AGPRs, SGPR spills and 80 bytes of
// scratch in the S+ mode-1 kernels.  A rolled loop cannot index registers by the step, so
//  * the accumulators of all steps live in LDS between two groups, one column per thread (kAccParts * NACC floats per
//    step, accs[f][thread]: conflict-free, and exact -- an fp32 goes in and comes out).  The host cuts a run where
//    its accumulators would exceed kChainBwdAccFloatsMax per thread (48 KiB per block);
//  * the steps' x sit in a register queue: every x of the first group is issued before the first step computes, x[0]
//    is the step about to run, and after a step the queue moves up (12 v_mov per slot).  Where a thread walks more
//    than one group, the next group's dy is loaded before the steps start and the next group's x_k joins the tail of
//    the queue right after step k has freed its slot: a one-deep prefetch for 12 extra registers, not 12 (NS + 1).
// tests/test_isa_chain_steps_bwd.py holds every kernel to 0 bytes of scratch and no spills and records the registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exposure_hip.h"
#include "filter_math.h"
#include "pixel_io.h"
#include "kernel_common.h"
#include "host_common.h"
#include "stream_bodies.h"  // kAccParts, EXPO_BWD_MIN_WAVES
// ChainStepsBwdArgs, run_step, run_reduce and the run table EXPO_RUN_FILTERS (shared with chain_steps_bwd_rc.hip)
#include "chain_steps_bwd_body.h"

namespace expo {

// (declared in host_common.h)
bool chain_steps_bwd_fusable(int id, int dtype, int mode) {
  if (id == 3 && dtype == EXPO_F32 && mode == 1) return false;
  return chain_steps_bwd_acc_floats(id) > 0;
}

// (declared in host_common.h)
int chain_steps_bwd_acc_floats(int id) {
  switch (id) {
#define EXPO_CASE(ID, F) \
  case ID: return kAccParts * F::NACC;
    EXPO_RUN_FILTERS(EXPO_CASE)
#undef EXPO_CASE
  }
  return 0;
}

template <typename T, int MODE, class IO, int NS>
__global__ __launch_bounds__(kThreads EXPO_BWD_MIN_WAVES) void chain_steps_bwd_kernel(const ChainStepsBwdArgs<NS> a) {
  constexpr int PPL = PixTraits<T>::PPL;
  static_assert(PPL >= kAccParts, "kParts == kAccParts in both storage types");
  const int n = blockIdx.y;
  const int hw = a.hw;
  const size_t off = size_t(n) * hw * 3;
  const int lane = threadIdx.x & 63;
#if EXPO_FP16_OVFL
  // MODE.FP16_OVFL as in stream_groups: the conversions of pack<half_t> saturate at +-65504
  if constexpr (sizeof(T) == 2) __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
#endif
  const int stride = gridDim.x * kThreads;
  int gw = blockIdx.x * kThreads + (threadIdx.x & ~63);  // wave-uniform
  const bool work = gw * PPL < hw;
  const __amdgpu_buffer_rsrc_t rdy = make_image_rsrc(static_cast<const T*>(a.dy) + off, hw);
  int boff = chunk_byte_offset<T>(gw, lane);
  // every step's x is in flight before the first step computes; x[0] is always the step about to run
  RawGroup cur, x[NS];
  if (work) {
    cur = load_raw<IO::kLoadDy>(rdy, boff);
#pragma unroll
    for (int k = 0; k < NS; ++k)
      x[k] = load_raw<IO::kLoadX>(make_image_rsrc(static_cast<const T*>(a.x[k]) + off, hw), boff);
  }
  // accs[f][thread], zeroed behind the first loads by every wave (one without a group reduces zeros): only the
  // owning thread ever touches its column, so no barrier guards it
  extern __shared__ float accs[];
  float* const mine = accs + threadIdx.x;
  for (int f = 0; f < a.acc_floats; ++f) mine[f * kThreads] = 0.f;
  if (work) {
    while (true) {
      const int gn = gw + stride;
      const bool more = gn * PPL < hw;  // wave-uniform
      const int bnext = chunk_byte_offset<T>(gn, lane);
      // the next group's dy before anything is stored (the buffers may alias, see the header)
      RawGroup nxt = cur;
      if (more) nxt = load_raw<IO::kLoadDy>(rdy, bnext);
#pragma unroll 1
      for (int st = 0; st < NS; ++st) {
        const float* const prm = a.prm[st];
        float* const lds = mine + a.acc_at[st] * kThreads;
#define EXPO_CASE(ID, F) \
  case ID: run_step<F, T, MODE>(prm + n * F::NP, x[0], cur, lds); break;
        switch (a.id[st]) {  // block-uniform
          EXPO_RUN_FILTERS(EXPO_CASE)
          default: break;  // (the host puts no other id into a run)
        }
#undef EXPO_CASE
        // the rounded gradient is stored AND is the next step's dy: what the next launch would have loaded
        store_raw<IO::kStore>(make_image_rsrc(static_cast<T*>(a.dx[st]) + off, hw), boff, cur);
        // the registers of this step's x are free: the queue moves up, and the next group's x of this step joins it
#pragma unroll
        for (int k = 0; k + 1 < NS; ++k) x[k] = x[k + 1];
        if (more) x[NS - 1] = load_raw<IO::kLoadX>(make_image_rsrc(static_cast<const T*>(a.x[st]) + off, hw), bnext);
      }
      if (!more) break;
      gw = gn;
      boff = bnext;
      cur = nxt;
    }
  }
  // every wave arrives here, also one without a group: each step's block reduction, a barrier between two of them
#pragma unroll 1
  for (int st = 0; st < NS; ++st) {
    if (st > 0) __syncthreads();
    float* const rec = a.rec[st] + size_t(n) * gridDim.x * kWsSlots;
    const float* const lds = mine + a.acc_at[st] * kThreads;
#define EXPO_CASE(ID, F) \
  case ID: run_reduce<F, T>(lds, rec); break;
    switch (a.id[st]) {
      EXPO_RUN_FILTERS(EXPO_CASE)
      default: break;
    }
#undef EXPO_CASE
  }
}

template <typename T, int MODE, int NS>
static int chain_steps_bwd_launch(const ChainStepsBwdArgs<NS>& a, const Geom& g, int np, hipStream_t s) {
  const dim3 grid(g.blocks_x, np), block(kThreads);
  const size_t lds = size_t(a.acc_floats) * kThreads * sizeof(float);
  if (g.stream)
    hipLaunchKernelGGL((chain_steps_bwd_kernel<T, MODE, IoStream, NS>), grid, block, lds, s, a);
  else
    hipLaunchKernelGGL((chain_steps_bwd_kernel<T, MODE, IoCached, NS>), grid, block, lds, s, a);
  HIP_TRY(hipGetLastError(), "chain_steps_bwd launch");
  return EXPO_OK;
}

template <typename T, int NS>
static int chain_steps_bwd_t(const int* ids, int i0, void* const* acts, void* const* grads,
                             const float* const* params, float* records, size_t step_floats, int nb, int np, int h,
                             int w, int mode, int n_geom, hipStream_t s) {
  // filter_bwd_kernel's geometry for kGeomReduce of the whole batch (the caller has asked chain_steps_vec_path)
  const Geom g = make_geom<T>(n_geom, h, w, {}, kGeomReduce);
  const size_t ioff = size_t(nb) * h * w * 3 * sizeof(T);
  ChainStepsBwdArgs<NS> a{};
  a.dy = static_cast<const char*>(grads[i0 + 1]) + ioff;
  for (int k = 0; k < NS; ++k) {
    const int i = i0 - k;
    a.x[k] = static_cast<const char*>(acts[i]) + ioff;
    a.dx[k] = static_cast<char*>(grads[i]) + ioff;
    a.prm[k] = params[i] + size_t(nb) * kNumParams[ids[i]];
    a.rec[k] = records + size_t(i) * step_floats + size_t(nb) * g.blocks_x * kWsSlots;
    a.id[k] = ids[i];
    a.acc_at[k] = a.acc_floats;
    a.acc_floats += chain_steps_bwd_acc_floats(ids[i]);
  }
  a.hw = h * w;
  return mode == 1 ? chain_steps_bwd_launch<T, 1, NS>(a, g, np, s) : chain_steps_bwd_launch<T, 0, NS>(a, g, np, s);
}

// (declared in host_common.h) Steps i0, i0 - 1, .., i0 - cnt + 1 of a chain's backward on images [nb, nb + np) in one
// launch.  The caller has checked the vector path; ids, acts, grads and params are the chain's own arrays.
int chain_steps_bwd(const int* ids, int i0, int cnt, void* const* acts, void* const* grads,
                    const float* const* params, float* records, size_t step_floats, int nb, int np, int h, int w,
                    int dtype, int mode, int n_geom, hipStream_t s) {
  if (cnt < 2 || cnt > kChainFuseMax || cnt > i0 + 1) return fail(EXPO_E_BADARG, "chain_steps_bwd: step count");
  int acc_floats = 0;
  for (int k = 0; k < cnt; ++k) {
    if (!chain_steps_bwd_fusable(ids[i0 - k], dtype, mode) || !grads[i0 - k])
      return fail(EXPO_E_BADARG, "chain_steps_bwd: not a step of the run table with a dx");
    acc_floats += chain_steps_bwd_acc_floats(ids[i0 - k]);
  }
  if (acc_floats > kChainBwdAccFloatsMax) return fail(EXPO_E_BADARG, "chain_steps_bwd: accumulators of the run");
#define EXPO_GO(NS)                                                                                                   \
  case NS:                                                                                                            \
    return dtype == EXPO_F16                                                                                          \
               ? chain_steps_bwd_t<half_t, NS>(ids, i0, acts, grads, params, records, step_floats, nb, np, h, w, mode, \
                                               n_geom, s)                                                             \
               : chain_steps_bwd_t<float, NS>(ids, i0, acts, grads, params, records, step_floats, nb, np, h, w, mode,  \
                                              n_geom, s);
  switch (cnt) {
    EXPO_GO(2) EXPO_GO(3) EXPO_GO(4) EXPO_GO(5) EXPO_GO(6) EXPO_GO(7) EXPO_GO(8)
  }
#undef EXPO_GO
  static_assert(kChainFuseMax == 8, "one instantiation per run length");
  return fail(EXPO_E_BADARG, "chain_steps_bwd: step count");
}

}  // namespace expo
