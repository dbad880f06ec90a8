// chain_steps_bwd_rc.hip -- a run of element-wise backward steps of expo_chain_bwd in ONE launch that RECOMPUTES the
// run's interior activations instead of loading them, bit-identical to chain_steps_bwd.hip (and so to the per-step
// kernels).
//
// chain_steps_bwd_kernel loads, per group, the head's dy and the x of every step of the run: 2 c + 1 passes for c
// steps.  But acts[i + 1] is what step i's forward made of acts[i] with the parameters this launch holds anyway, and
// chain_steps.hip already reproduces that in registers bit for bit.  This kernel loads the head's dy and only the x of
// the run's LOWEST step, runs the forward of the steps below the head on it (unpack<T> -> F::load + F::fwd -> pack<T>,
// exactly chain_steps_fwd_kernel's EXPO_CASE, the value travelling PACKED between steps so that the compiler meets
// the per-step forward kernel's expression tree and rounds where it rounds), keeps every step's input in registers,
// and then runs the backward steps as chain_steps_bwd_kernel does (run_step, every dx stored): c + 2 passes.
//
// The contract this needs: acts[1..steps] handed to expo_chain_bwd are what expo_chain_fwd (or per-step
// expo_filter_fwd) made of acts[0] with these params.  include/exposure_hip.h states it; EXPO_CHAIN_BWD_RECOMPUTE=0
// keeps chain_steps_bwd_kernel for a caller that edits activations between the two calls.
//
// Everything else is chain_steps_bwd_kernel's: geometry, grid, wave walk, IoStream / IoCached, MODE.FP16_OVFL, the LDS
// accumulator columns, the record slices, the epilogue and its barriers, the per-thread group order and every addend
// order.  Gradient buffers may alias (ping-pong): the next group's dy -- and its lowest x, the pair -- are loaded
// before anything is stored; activations are never written here.
//
// Which forwards are recomputed is a static table per (filter id, storage type), EXPO_RC_FILTERS below, decided by the
// GPU comparison like EXPO_RUN_FILTERS: tests/test_hip_chain_bwd_pairs.py runs every ordered pair of the table's
// filters inside a run, every run length 2..8, both storage types, both modes and both cache policies against the
// per-step kernels, on images that hold the filters' clamp edges and values that saturate the fp16 store.  Where a step's forward is not in it, the step above keeps loading its x from
// acts (issued up front with the pair) and the sweep restarts from that loaded value: L such loads make L + 1 + c
// passes.
//
// Resources.  The backward step loop is rolled as in chain_steps_bwd_kernel (x[0] is the step about to run, the queue
// moves up after a step).  The forward sweep has no accumulators and is unrolled by template over the slot: x[k] is
// written from x[k + 1] with static register indices, no queue moves, and a slot's block-uniform switch holds the
// forward bodies of the table.  tests/test_isa_chain_steps_bwd_rc.py holds every kernel to 0 bytes of scratch and no
// spills and records the registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exposure_hip.h"
#include "filter_math.h"
#include "pixel_io.h"
#include "kernel_common.h"
#include "host_common.h"
#include "stream_bodies.h"
#include "chain_steps_bwd_body.h"

namespace expo {

// The forwards this kernel recomputes: X(id, filter, in fp16, in fp32).  A 0 keeps the load of that step's output.
#define EXPO_RC_FILTERS(X) \
  X(0, ExposureF, 1, 1) X(1, GammaF, 1, 1) X(2, WhiteBalanceF, 1, 1) X(3, SatPlusF, 1, 1) X(8, LevelF, 1, 1)

template <typename T>
__host__ __device__ constexpr bool rc_recomputable(int id) {
  switch (id) {
#define EXPO_CASE(ID, F, H, S) \
  case ID: return sizeof(T) == 2 ? H : S;
    EXPO_RC_FILTERS(EXPO_CASE)
#undef EXPO_CASE
  }
  return false;
}

// the run-time form for the ids a run can hold (EXPO_RUN_FILTERS): is this step's output loaded?  With every entry of the
// table set this is `false` at compile time and the loads below are no code at all.
template <typename T>
__host__ __device__ constexpr bool rc_keeps_load(int id) {
  switch (id) {
#define EXPO_CASE(ID, F, H, S) \
  case ID: return !(sizeof(T) == 2 ? H : S);
    EXPO_RC_FILTERS(EXPO_CASE)
#undef EXPO_CASE
  }
  return false;
}

// (declared in host_common.h)
bool chain_steps_bwd_recomputes(int id, int dtype) {
  return dtype == EXPO_F16 ? rc_recomputable<half_t>(id) : rc_recomputable<float>(id);
}

// one forward step on one group: chain_steps_fwd_kernel's EXPO_CASE.  `out` is left alone where the filter is not
// recomputed (it then holds the loaded activation).
template <typename T>
__device__ __forceinline__ RawGroup rc_forward(int id, const float* prm, int n, const RawGroup in, RawGroup out) {
  constexpr int PPL = PixTraits<T>::PPL;
#define EXPO_CASE(ID, F, H, S)                                           \
  case ID:                                                               \
    if constexpr (rc_recomputable<T>(ID)) {                              \
      const typename F::Prm q = F::load(prm + n * F::NP);                \
      float v[PPL * 3];                                                  \
      unpack<T>(in, v);                                                  \
      _Pragma("unroll") for (int k = 0; k < PPL; ++k) {                  \
        float y[3];                                                      \
        F::fwd(q, v + 3 * k, y);                                         \
        _Pragma("unroll") for (int c = 0; c < 3; ++c) v[3 * k + c] = y[c]; \
      }                                                                  \
      out = pack<T>(v);                                                  \
    }                                                                    \
    break;
  switch (id) {  // block-uniform
    EXPO_RC_FILTERS(EXPO_CASE)
    default: break;
  }
#undef EXPO_CASE
  return out;
}

// the forward sweep over slots K, K - 1, .., 0 (towards the head): x[k] = the forward of step (head - k - 1) on x[k + 1]
template <typename T, int NS, int K>
__device__ __forceinline__ void rc_sweep(const ChainStepsBwdArgs<NS>& a, int n, RawGroup (&x)[NS]) {
  if constexpr (K >= 0) {
    // the slot index made opaque: with a static index the compiler fetches every slot's id and parameter pointer at the
    // top of the kernel and keeps them (spilled SGPRs from NS = 6); this way they are scalar loads at the point of use
    int s = K + 1;
    asm volatile("" : "+s"(s));
    x[K] = rc_forward<T>(a.id[s], a.prm[s], n, x[K + 1], x[K]);
    rc_sweep<T, NS, K - 1>(a, n, x);
  }
}

// the activations the sweep does not make (the output of a step outside EXPO_RC_FILTERS), issued up front
template <typename T, class IO, int NS>
__device__ __forceinline__ void rc_load_kept(const ChainStepsBwdArgs<NS>& a, size_t off, int hw, int boff,
                                             RawGroup (&x)[NS]) {
#pragma unroll
  for (int k = 0; k + 1 < NS; ++k)
    if (rc_keeps_load<T>(a.id[k + 1]))
      x[k] = load_raw<IO::kLoadX>(make_image_rsrc(static_cast<const T*>(a.x[k]) + off, hw), boff);
}

template <typename T, int MODE, class IO, int NS>
__global__ __launch_bounds__(kThreads EXPO_BWD_MIN_WAVES) void chain_steps_bwd_rc_kernel(const ChainStepsBwdArgs<NS> a) {
  constexpr int PPL = PixTraits<T>::PPL;
  static_assert(PPL >= kAccParts, "kParts == kAccParts in both storage types");
  const int n = blockIdx.y;
  const int hw = a.hw;
  const size_t off = size_t(n) * hw * 3;
  const int lane = threadIdx.x & 63;
#if EXPO_FP16_OVFL
  // MODE.FP16_OVFL as in stream_groups: the conversions of pack<half_t> saturate at +-65504 (forward and backward)
  if constexpr (sizeof(T) == 2) __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
#endif
  const int stride = gridDim.x * kThreads;
  int gw = blockIdx.x * kThreads + (threadIdx.x & ~63);  // wave-uniform
  const bool work = gw * PPL < hw;
  const __amdgpu_buffer_rsrc_t rdy = make_image_rsrc(static_cast<const T*>(a.dy) + off, hw);
  const __amdgpu_buffer_rsrc_t rlow = make_image_rsrc(static_cast<const T*>(a.x[NS - 1]) + off, hw);
  int boff = chunk_byte_offset<T>(gw, lane);
  // the pair -- the head's dy and the lowest step's x -- and whatever the table keeps loading are in flight before
  // anything computes; after the sweep x[k] is slot k's input, x[0] always the step about to run
  RawGroup cur, x[NS];
  if (work) {
    cur = load_raw<IO::kLoadDy>(rdy, boff);
    x[NS - 1] = load_raw<IO::kLoadX>(rlow, boff);
    rc_load_kept<T, IO, NS>(a, off, hw, boff, x);
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
      // the next group's pair before anything is stored (the gradient buffers may alias, see the header)
      RawGroup nxt = cur, nlow = x[NS - 1];
      if (more) {
        nxt = load_raw<IO::kLoadDy>(rdy, bnext);
        nlow = load_raw<IO::kLoadX>(rlow, bnext);
      }
      // the forward sweep, from the lowest step's x up to the head's
      rc_sweep<T, NS, NS - 2>(a, n, x);
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
        // the registers of this step's x are free: the queue moves up
#pragma unroll
        for (int k = 0; k + 1 < NS; ++k) x[k] = x[k + 1];
      }
      if (!more) break;
      gw = gn;
      boff = bnext;
      cur = nxt;
      x[NS - 1] = nlow;
      rc_load_kept<T, IO, NS>(a, off, hw, boff, x);
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
static int chain_steps_bwd_rc_launch(const ChainStepsBwdArgs<NS>& a, const Geom& g, int np, hipStream_t s) {
  const dim3 grid(g.blocks_x, np), block(kThreads);
  const size_t lds = size_t(a.acc_floats) * kThreads * sizeof(float);
  if (g.stream)
    hipLaunchKernelGGL((chain_steps_bwd_rc_kernel<T, MODE, IoStream, NS>), grid, block, lds, s, a);
  else
    hipLaunchKernelGGL((chain_steps_bwd_rc_kernel<T, MODE, IoCached, NS>), grid, block, lds, s, a);
  HIP_TRY(hipGetLastError(), "chain_steps_bwd_rc launch");
  return EXPO_OK;
}

template <typename T, int NS>
static int chain_steps_bwd_rc_t(const int* ids, int i0, void* const* acts, void* const* grads,
                                const float* const* params, float* records, size_t step_floats, int nb, int np, int h,
                                int w, int mode, int n_geom, hipStream_t s) {
  // chain_steps_bwd_t's arguments: filter_bwd_kernel's geometry for kGeomReduce of the whole batch
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
  return mode == 1 ? chain_steps_bwd_rc_launch<T, 1, NS>(a, g, np, s) : chain_steps_bwd_rc_launch<T, 0, NS>(a, g, np, s);
}

// (declared in host_common.h) chain_steps_bwd with the run's interior activations recomputed: the same arguments, the
// same launch geometry, the same results where acts[i0 - cnt + 2 .. i0] are the forward of acts[i0 - cnt + 1].
int chain_steps_bwd_rc(const int* ids, int i0, int cnt, void* const* acts, void* const* grads,
                       const float* const* params, float* records, size_t step_floats, int nb, int np, int h, int w,
                       int dtype, int mode, int n_geom, hipStream_t s) {
  if (cnt < 2 || cnt > kChainFuseMax || cnt > i0 + 1) return fail(EXPO_E_BADARG, "chain_steps_bwd_rc: step count");
  int acc_floats = 0;
  for (int k = 0; k < cnt; ++k) {
    if (!chain_steps_bwd_fusable(ids[i0 - k], dtype, mode) || !grads[i0 - k])
      return fail(EXPO_E_BADARG, "chain_steps_bwd_rc: not a step of the run table with a dx");
    acc_floats += chain_steps_bwd_acc_floats(ids[i0 - k]);
  }
  if (acc_floats > kChainBwdAccFloatsMax) return fail(EXPO_E_BADARG, "chain_steps_bwd_rc: accumulators of the run");
#define EXPO_GO(NS)                                                                                                      \
  case NS:                                                                                                               \
    return dtype == EXPO_F16                                                                                             \
               ? chain_steps_bwd_rc_t<half_t, NS>(ids, i0, acts, grads, params, records, step_floats, nb, np, h, w, mode, \
                                                  n_geom, s)                                                             \
               : chain_steps_bwd_rc_t<float, NS>(ids, i0, acts, grads, params, records, step_floats, nb, np, h, w, mode,  \
                                                 n_geom, s);
  switch (cnt) {
    EXPO_GO(2) EXPO_GO(3) EXPO_GO(4) EXPO_GO(5) EXPO_GO(6) EXPO_GO(7) EXPO_GO(8)
  }
#undef EXPO_GO
  static_assert(kChainFuseMax == 8, "one instantiation per run length");
  return fail(EXPO_E_BADARG, "chain_steps_bwd_rc: step count");
}

}  // namespace expo
