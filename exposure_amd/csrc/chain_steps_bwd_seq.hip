// chain_steps_bwd_seq.hip -- a run of element-wise backward steps of expo_chain_bwd whose filter ids are known when
// this unit is COMPILED, in one launch of straight-line code, bit-identical to chain_steps_bwd_rc.hip (and so to the
// per-step kernels).
//
// chain_steps_bwd_rc_kernel takes any sequence of the run table: its backward step loop is rolled over a block-uniform
// switch, so the steps' x sit in a register queue that moves up after every step, the accumulators go to LDS and back
// around every step, and every step fetches its id and its parameters behind the previous step's stores.  DESIGN.md
// 3.30 measured that launch issue-bound (about 1 700 wave instructions per group).  The reference ships ONE filter
// order, so the run the chain call of its configuration collects is always the same: [S+, W, G, E] from the head down.
// For the sequences of the table below this unit holds chain_steps_bwd_seq_kernel<T, MODE, IO, Ids...>:
//  * no step loop and no switch: the sweep and the backward steps are unrolled by template over Ids;
//  * the sweep's x stay in registers of their own, nothing moves;
//  * the accumulators are registers across the groups a thread walks;
//  * every step's parameters are fetched once per wave, after the first group's loads are issued (DESIGN.md 3.1
//    "loads before parameters") and before the first store, so they are scalar loads.
//
// What it keeps of chain_steps_bwd_rc_kernel: the contract (recomputation on, interior acts never read), the kernel
// arguments, the kGeomReduce geometry of the whole batch, grid (blocks_x, np), the block-strided wave walk and the
// per-thread group order, IoStream / IoCached, MODE.FP16_OVFL, the record slices, every dx stored, the next group's
// pair loaded before anything is stored (gradient buffers may alias), an epilogue that every wave reaches with a
// barrier between two block reductions, and the kAccParts partial sums folded in run_reduce's order.  Each step is
// unpack<T> -> F::load + F::fwd / F::bwd -> pack<T>, the value travelling PACKED between steps; between two steps an
// empty asm takes the packed group, so a step stays the isolated expression tree the per-step kernel holds and the
// compiler does not keep a step's unpacked values alive into the next one.
//
// Which sequences exist is a static table, EXPO_RUN_SEQUENCES, decided by the GPU comparison like EXPO_RUN_FILTERS
// and EXPO_RC_FILTERS (tests/test_hip_chain_bwd_seq.py); every other run keeps chain_steps_bwd_rc / chain_steps_bwd.
// tests/test_isa_chain_steps_bwd_seq.py holds every kernel to 0 bytes of scratch and no spills and records the
// registers.
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

// The sequences compiled here: X(storage type, dtype, hsv_grad_mode, on, ids from the run's head down to its lowest
// step).  An entry whose kernel does not give the per-step kernels' bits is set to 0: no kernel is built for it and
// that run keeps chain_steps_bwd_rc_kernel.
#define EXPO_RUN_SEQUENCES(X)          \
  X(half_t, EXPO_F16, 0, 1, 3, 2, 1, 0) \
  X(half_t, EXPO_F16, 1, 1, 3, 2, 1, 0) \
  X(float, EXPO_F32, 0, 1, 3, 2, 1, 0)

template <int ID> struct SeqFilter;
#define EXPO_CASE(ID, F) \
  template <> struct SeqFilter<ID> { using type = F; };
EXPO_RUN_FILTERS(EXPO_CASE)
#undef EXPO_CASE

// the ids of a sequence; slot k is step (head - k) as in ChainStepsBwdArgs
template <int... Ids>
struct Seq {
  static constexpr int NS = sizeof...(Ids);
  __host__ __device__ static constexpr int id(int k) {
    constexpr int v[NS] = {Ids...};
    return v[k];
  }
  template <int K> using F = typename SeqFilter<id(K)>::type;
  template <int K>
  __host__ __device__ static constexpr int acc_at() {  // ChainStepsBwdArgs::acc_at[K]
    if constexpr (K == 0) return 0;
    else return acc_at<K - 1>() + kAccParts * F<K - 1>::NACC;
  }
};

// every step's derived parameters
template <class S, int K = 0, bool = (K < S::NS)>
struct SeqPrm {};
template <class S, int K>
struct SeqPrm<S, K, true> {
  typename S::template F<K>::Prm q;
  SeqPrm<S, K + 1> rest;
};
template <int K, class S, int J>
__device__ __forceinline__ auto& seq_prm(SeqPrm<S, J, true>& p) {
  if constexpr (K == J) return p.q;
  else return seq_prm<K>(p.rest);
}

template <class S, int K = 0>
__device__ __forceinline__ void seq_load_prm(const ChainStepsBwdArgs<S::NS>& a, int n, SeqPrm<S>& q) {
  if constexpr (K < S::NS) {
    using F = typename S::template F<K>;
    seq_prm<K>(q) = F::load(a.prm[K] + n * F::NP);
    seq_load_prm<S, K + 1>(a, n, q);
  }
}

// Groups are copied and loaded vector by vector: a whole-struct copy of a RawGroup is a 64-byte memcpy over the padding
// of its dwordx3 vectors, and in fp32 the array of groups then stays in scratch.
__device__ __forceinline__ void seq_copy(RawGroup& d, const RawGroup& s) {
#pragma unroll
  for (int j = 0; j < 4; ++j) d.q[j] = s.q[j];
}
template <int AUX>
__device__ __forceinline__ void seq_load(RawGroup& d, __amdgpu_buffer_rsrc_t rsrc, int byte_off) {
#pragma unroll
  for (int j = 0; j < 4; ++j) d.q[j] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, byte_off + j * 768, 0, AUX);  // load_raw
}

// The packed group is opaque from here on: what follows starts from these registers as it would from a reload.  It
// stands behind every pack<T> and -- on a copy -- in front of every unpack<T>:
//  * fp32: unpack<float>'s copy loop becomes a 12-byte memcpy per vector, and read straight from the kernel's groups it
//    keeps them all in scratch (272 bytes);
//  * fp16: without the one in front of unpack the sweep's Gamma forward and the Gamma backward share the v_log_f32 /
//    v_exp_f32 of the same value and the unpacked x (1 098 vector instructions, 81 of them transcendental, instead of
//    1 250 / 129), but those 48 values live across the S+ and White balance steps: 250 registers and two waves per
//    SIMD instead of 165 and three.  Measured, that variant is the slower one.
__device__ __forceinline__ void seq_fence(RawGroup& g) {
  // (through copies: an operand that is an element of the group in place keeps the whole array of groups in scratch)
  u32x3_t q0 = g.q[0], q1 = g.q[1], q2 = g.q[2], q3 = g.q[3];
  asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3));
  g.q[0] = q0, g.q[1] = q1, g.q[2] = q2, g.q[3] = q3;
}

// The register budget, in waves per SIMD, each instantiation is compiled for (and held to: no scratch).  Three is the
// occupancy of chain_steps_bwd_rc_kernel at this run length; S+ with the analytic hue gradient in fp16 has two there too.
template <typename T, int MODE>
__host__ __device__ constexpr int seq_min_waves() {
  return sizeof(T) == 2 && MODE == 1 ? 2 : 3;
}

// the forward sweep over slots K, K - 1, .., 0 (towards the head): x[k] = the forward of step (head - k - 1) on
// x[k + 1], chain_steps_fwd_kernel's EXPO_CASE
template <typename T, class S, int K>
__device__ __forceinline__ void seq_sweep(SeqPrm<S>& q, RawGroup (&x)[S::NS]) {
  if constexpr (K >= 0) {
    constexpr int PPL = PixTraits<T>::PPL;
    using F = typename S::template F<K + 1>;
    float v[PPL * 3];
    RawGroup xin;
    seq_copy(xin, x[K + 1]);
    seq_fence(xin);
    unpack<T>(xin, v);
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      float y[3];
      F::fwd(seq_prm<K + 1>(q), v + 3 * k, y);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * k + c] = y[c];
    }
    RawGroup y = pack<T>(v);
    seq_fence(y);
    seq_copy(x[K], y);
    seq_sweep<T, S, K - 1>(q, x);
  }
}

// Which backward bodies run a group in two halves (see seq_bwd): S+ with the analytic hue gradient in fp16, whose eight
// interleaved pixels would not leave the registers for two waves per SIMD.
template <class F, typename T, int MODE>
__host__ __device__ constexpr bool seq_halves() {
  return false;
}
template <>
__host__ __device__ constexpr bool seq_halves<SatPlusF, half_t, 1>() {
  return true;
}

// the backward steps K, K + 1, .., NS - 1 (away from the head): run_step with the accumulators in registers, then the
// store of the rounded gradient, which is also the next step's dy
template <typename T, int MODE, class IO, class S, int K, int NACCS>
__device__ __forceinline__ void seq_bwd(const ChainStepsBwdArgs<S::NS>& a, SeqPrm<S>& q, const RawGroup (&x)[S::NS],
                                        RawGroup& g, float (&acc)[NACCS], size_t off, int hw, int boff) {
  if constexpr (K < S::NS) {
    constexpr int PPL = PixTraits<T>::PPL;
    constexpr int kParts = kAccParts < PPL ? kAccParts : PPL;
    using F = typename S::template F<K>;
    static_assert(!F::kHasGroupBwd && F::kLutFloats == 0, "element-wise filters only");
    constexpr int at = S::template acc_at<K>();
    float v[PPL * 3], d[PPL * 3];
    RawGroup xin, gin;
    seq_copy(xin, x[K]);
    seq_copy(gin, g);
    seq_fence(xin);
    seq_fence(gin);
    unpack<T>(xin, v);
    unpack<T>(gin, d);
    auto pixels = [&](int k0, int k1) {
#pragma unroll
      for (int k = k0; k < k1; ++k) {
        float dx[3];
        F::bwd(seq_prm<K>(q), nullptr, v + 3 * k, d + 3 * k, dx, acc + at + (k % kParts) * F::NACC, MODE);
#pragma unroll
        for (int c = 0; c < 3; ++c) d[3 * k + c] = dx[c];
      }
    };
    if constexpr (seq_halves<F, T, MODE>()) {
      // the group in two halves, the second one's packed inputs behind the first one's packed results: the compiler
      // interleaves the pixels of a half only (register budget).  Every value still goes unpack<T> -> F::bwd ->
      // pack<T>; what the extra calls make of the other half is dead.
      pixels(0, PPL / 2);
      const RawGroup half = pack<T>(d);
      asm volatile("" : "+v"(xin.q[2]), "+v"(xin.q[3]), "+v"(gin.q[2]), "+v"(gin.q[3]) : "v"(half.q[0]), "v"(half.q[1]));
      float v2[PPL * 3], d2[PPL * 3];
      unpack<T>(xin, v2);
      unpack<T>(gin, d2);
#pragma unroll
      for (int i = PPL * 3 / 2; i < PPL * 3; ++i) v[i] = v2[i], d[i] = d2[i];
      pixels(PPL / 2, PPL);
    } else {
      pixels(0, PPL);
    }
    RawGroup dxg = pack<T>(d);
    store_raw<IO::kStore>(make_image_rsrc(static_cast<T*>(a.dx[K]) + off, hw), boff, dxg);
    seq_fence(dxg);
    seq_copy(g, dxg);
    seq_bwd<T, MODE, IO, S, K + 1>(a, q, x, g, acc, off, hw, boff);
  }
}

// run_reduce for steps K .. NS - 1, a barrier between two of them
template <typename T, class S, int K, int NACCS>
__device__ __forceinline__ void seq_reduce(const ChainStepsBwdArgs<S::NS>& a, int n, const float (&acc)[NACCS]) {
  if constexpr (K < S::NS) {
    constexpr int PPL = PixTraits<T>::PPL;
    constexpr int kParts = kAccParts < PPL ? kAccParts : PPL;
    using F = typename S::template F<K>;
    constexpr int at = S::template acc_at<K>();
    if (K > 0) __syncthreads();
    float r[F::NACC];
#pragma unroll
    for (int j = 0; j < F::NACC; ++j) r[j] = acc[at + j];
#pragma unroll
    for (int p = 0; p < kParts - 1; ++p)
#pragma unroll
      for (int j = 0; j < F::NACC; ++j) r[j] += acc[at + (p + 1) * F::NACC + j];
    block_reduce_record<F::NACC>(r, a.rec[K] + size_t(n) * gridDim.x * kWsSlots);
    seq_reduce<T, S, K + 1>(a, n, acc);
  }
}

template <typename T, int MODE, class IO, int... Ids>
__global__ __launch_bounds__(kThreads, (seq_min_waves<T, MODE>())) void chain_steps_bwd_seq_kernel(
    const ChainStepsBwdArgs<sizeof...(Ids)> a) {
  using S = Seq<Ids...>;
  constexpr int NS = S::NS;
  constexpr int PPL = PixTraits<T>::PPL;
  static_assert(PPL >= kAccParts, "kParts == kAccParts in both storage types");
  constexpr int NACCS = S::template acc_at<NS - 1>() + kAccParts * S::template F<NS - 1>::NACC;
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
  // a thread's accumulators, acc[ChainStepsBwdArgs::acc_at[k] + p * NACC + j]; a wave without a group reduces zeros
  float acc[NACCS];
#pragma unroll
  for (int f = 0; f < NACCS; ++f) acc[f] = 0.f;
  if (work) {
    // the pair -- the head's dy and the lowest step's x -- is in flight before the parameters are fetched
    RawGroup cur, x[NS];
    seq_load<IO::kLoadDy>(cur, rdy, boff);
    seq_load<IO::kLoadX>(x[NS - 1], rlow, boff);
    SeqPrm<S> q;
    seq_load_prm<S>(a, n, q);
    while (true) {
      const int gn = gw + stride;
      const bool more = gn * PPL < hw;  // wave-uniform
      const int bnext = chunk_byte_offset<T>(gn, lane);
      // the next group's pair before anything is stored (the gradient buffers may alias)
      RawGroup nxt, nlow;
      seq_copy(nxt, cur);
      seq_copy(nlow, x[NS - 1]);
      if (more) {
        seq_load<IO::kLoadDy>(nxt, rdy, bnext);
        seq_load<IO::kLoadX>(nlow, rlow, bnext);
      }
      // the forward sweep, from the lowest step's x up to the head's, then the backward steps from the head down
      seq_sweep<T, S, NS - 2>(q, x);
      seq_bwd<T, MODE, IO, S, 0>(a, q, x, cur, acc, off, hw, boff);
      if (!more) break;
      gw = gn;
      boff = bnext;
      seq_copy(cur, nxt);
      seq_copy(x[NS - 1], nlow);
    }
  }
  // every wave arrives here, also one without a group: each step's block reduction, a barrier between two of them
  seq_reduce<T, S, 0>(a, n, acc);
}

template <typename T, int MODE, int... Ids>
static int chain_steps_bwd_seq_launch(const int* ids, int i0, void* const* acts, void* const* grads,
                                      const float* const* params, float* records, size_t step_floats, int nb, int np,
                                      int h, int w, int n_geom, hipStream_t s) {
  constexpr int NS = sizeof...(Ids);
  // chain_steps_bwd_rc_t's arguments: filter_bwd_kernel's geometry for kGeomReduce of the whole batch
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
  const dim3 grid(g.blocks_x, np), block(kThreads);
  if (g.stream)
    hipLaunchKernelGGL((chain_steps_bwd_seq_kernel<T, MODE, IoStream, Ids...>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((chain_steps_bwd_seq_kernel<T, MODE, IoCached, Ids...>), grid, block, 0, s, a);
  HIP_TRY(hipGetLastError(), "chain_steps_bwd_seq launch");
  return EXPO_OK;
}

template <int... Ids>
static bool seq_matches(const int* ids, int i0, int cnt) {
  constexpr int NS = sizeof...(Ids);
  constexpr int v[NS] = {Ids...};
  if (cnt != NS || cnt > i0 + 1) return false;
  for (int k = 0; k < NS; ++k)
    if (ids[i0 - k] != v[k]) return false;
  return true;
}

// (declared in host_common.h)
bool chain_steps_bwd_seq_has(const int* ids, int i0, int cnt, int dtype, int mode) {
#define EXPO_CASE(T, DT, MODE, ON, ...) \
  if (ON && dtype == DT && mode == MODE && seq_matches<__VA_ARGS__>(ids, i0, cnt)) return true;
  EXPO_RUN_SEQUENCES(EXPO_CASE)
#undef EXPO_CASE
  return false;
}

// (declared in host_common.h) chain_steps_bwd_rc for a run of the table: the same arguments, the same launch
// geometry, the same results.
int chain_steps_bwd_seq(const int* ids, int i0, int cnt, void* const* acts, void* const* grads,
                        const float* const* params, float* records, size_t step_floats, int nb, int np, int h, int w,
                        int dtype, int mode, int n_geom, hipStream_t s) {
  for (int k = 0; k < cnt && k <= i0; ++k)
    if (!grads[i0 - k]) return fail(EXPO_E_BADARG, "chain_steps_bwd_seq: a step without a dx");
#define EXPO_CASE(T, DT, MODE, ON, ...)                                                                    \
  if constexpr (ON) {                                                                                      \
    if (dtype == DT && mode == MODE && seq_matches<__VA_ARGS__>(ids, i0, cnt))                             \
      return chain_steps_bwd_seq_launch<T, MODE, __VA_ARGS__>(ids, i0, acts, grads, params, records,       \
                                                              step_floats, nb, np, h, w, n_geom, s);        \
  }
  EXPO_RUN_SEQUENCES(EXPO_CASE)
#undef EXPO_CASE
  return fail(EXPO_E_BADARG, "chain_steps_bwd_seq: not a sequence of the table");
}

}  // namespace expo
