// chain_steps.hip -- several consecutive steps of expo_chain_fwd in ONE launch, bit-identical to the per-step kernels.
//
// A chain's forward launches one filter_fwd_kernel per step: step k reads acts[k] and writes acts[k+1], and step k+1
// reads back what step k has just written.  expo_chain_fwd knows every filter id, parameter pointer and activation
// pointer before its first launch, so the re-reads are work the result does not need: this kernel loads a 48-byte
// pixel group of acts[0] once, applies the steps one after the other while the group sits in registers and stores
// every intermediate acts[k+1] on the way.  8 steps: 9 passes over memory instead of 16.
//
// Why the bits do not change.  Between two steps the per-step path rounds to the storage type (pack<T>, with
// MODE.FP16_OVFL set as stream_groups sets it), stores, and the next launch loads and widens again (unpack<T>).  Here a
// step's result is packed with the same pack<T>, those very registers are stored, and the next step continues from
// unpack<T> of them -- the value a reload would have returned.  Each step's arithmetic is the device function the
// per-step kernel calls (F::load + F::fwd; curve_lut_build + curve_lut_apply for Tone / Color on the vector path),
// compiled with the flags of exposure_hip.hip (not the inference kernel's -fno-honor-nans: chain_fused.hip carries
// fp32 between steps and is a different function of its input).
//
// One thing the source does not show decides bits in fp16: where a filter ends in an fma whose only use is the
// conversion to half (S+, WNB), the compiler may select v_fma_mixlo_f16 / v_fma_mixhi_f16, which round the exact
// a * b + c ONCE, to half; v_fma_f32 + v_cvt_pk_f16_f32 rounds twice, and about one value in 2^14 comes out one fp16
// ulp apart.  The per-step kernels hold a fixed mixture of the two per element of the group (the SLP vectoriser pairs
// some elements into v_pk_fma_f32 first).  A first version of this kernel carried the unpacked fp32 values from step
// to step and got another mixture -- and a handful of differing values per image.  Hence the group is carried PACKED
// and every step is written as unpack<T> -> filter -> pack<T>, the very data flow of a per-step kernel between its
// load and its store: the compiler then builds the same expression tree per step and selects the same instructions.
// tests/test_isa_chain_steps.py counts them against the per-step kernels; tests/test_hip_chain_fuse.py holds the two
// paths to torch.equal on every activation at sizes where one such value in 2^14 cannot hide.
//
// Geometry: the grid, the wave -> chunk map and the cache policy of filter_fwd_kernel (kGeomMap of the WHOLE batch,
// IoStream / IoCached by tensor size), so a wave stores exactly the lines a per-step wave would.  The step loop is
// rolled (block-uniform switch on the filter id): any order of ids, repeats included.  Only the dwordx3 vector path
// is served; other shapes keep the per-step launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exposure_hip.h"
#include "filter_math.h"
#include "pixel_io.h"
#include "kernel_common.h"
#include "host_common.h"

namespace expo {

// everything a launch needs, by value in the kernel arguments (no device-side table, nothing to keep alive)
struct ChainStepsFwdArgs {
  const void* x;                       // acts[first step], at the chunk's first image
  void* y[kChainFuseMax];              // acts[first step + 1 + k], at the chunk's first image
  const float* prm[kChainFuseMax];     // the step's parameters, at the chunk's first image
  int id[kChainFuseMax];
  int steps, hw;
};

template <typename T, class IO>
__global__ __launch_bounds__(kThreads) void chain_steps_fwd_kernel(const ChainStepsFwdArgs a) {
  constexpr int PPL = PixTraits<T>::PPL;
  const int n = blockIdx.y;
  const int hw = a.hw;
  const size_t off = size_t(n) * hw * 3;
  const int lane = threadIdx.x & 63;
  // this wave's curve segment table (kernel_common.h), rebuilt by every Tone / Color step
  __shared__ float2_lut ftab[kWaves][32];
  float2_lut* const tab = ftab[threadIdx.x >> 6];
#if EXPO_FP16_OVFL
  // MODE.FP16_OVFL as in stream_groups: the conversions of pack<half_t> saturate at +-65504
  if constexpr (sizeof(T) == 2) __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
#endif
  const __amdgpu_buffer_rsrc_t rx = make_image_rsrc(static_cast<const T*>(a.x) + off, hw);
  const int stride = gridDim.x * kThreads;
  for (int gw = blockIdx.x * kThreads + (threadIdx.x & ~63); gw * PPL < hw; gw += stride) {  // wave-uniform
    const int boff = chunk_byte_offset<T>(gw, lane);
    // The group travels from step to step PACKED (the storage type's bits, 12 VGPRs): every step is unpack<T> ->
    // the filter -> pack<T>, the data flow between the load and the store of a per-step kernel, so the compiler meets
    // the same expression tree per step and makes the same choices in it (header: v_fma_mix).
    RawGroup cur = load_raw<IO::kLoadX>(rx, boff);
#pragma unroll 1
    for (int st = 0; st < a.steps; ++st) {
      const float* const prm = a.prm[st];
      float v[PPL * 3];
#define EXPO_CASE(ID, F)                               \
  case ID: {                                           \
    const typename F::Prm q = F::load(prm + n * F::NP); \
    unpack<T>(cur, v);                                 \
    _Pragma("unroll") for (int k = 0; k < PPL; ++k) {  \
      float y[3];                                      \
      F::fwd(q, v + 3 * k, y);                         \
      _Pragma("unroll") for (int c = 0; c < 3; ++c) v[3 * k + c] = y[c]; \
    }                                                  \
    cur = pack<T>(v);                                  \
  } break;
      switch (a.id[st]) {
        EXPO_CASE(0, ExposureF)
        EXPO_CASE(1, GammaF)
        EXPO_CASE(2, WhiteBalanceF)
        EXPO_CASE(3, SatPlusF)
        case 4:
          curve_lut_build<1>(prm[n * ToneF::NP + lane % ToneF::NP], tab);
          unpack<T>(cur, v);
          curve_lut_apply<1, PPL>(v, tab);
          cur = pack<T>(v);
          __builtin_amdgcn_wave_barrier();  // the next curve step of this wave rewrites the table
          break;
        EXPO_CASE(5, ContrastF)
        EXPO_CASE(6, WnbF)
        case 7:
          curve_lut_build<3>(prm[n * ColorF::NP + lane % ColorF::NP], tab);
          unpack<T>(cur, v);
          curve_lut_apply<3, PPL>(v, tab);
          cur = pack<T>(v);
          __builtin_amdgcn_wave_barrier();
          break;
        EXPO_CASE(8, LevelF)
        default: break;  // (ids are validated on the host)
      }
#undef EXPO_CASE
      // the rounded result is stored AND is the next step's input: what the next launch would have loaded
      store_raw<IO::kStore>(make_image_rsrc(static_cast<T*>(a.y[st]) + off, hw), boff, cur);
    }
  }
}

template <typename T>
static int chain_steps_fwd_t(const ChainStepsFwdArgs& a, int np, int h, int w, int n_geom, hipStream_t s) {
  const Geom g = make_geom<T>(n_geom, h, w, {}, kGeomMap);  // (the caller has asked chain_steps_vec_path)
  const dim3 grid(g.blocks_x, np), block(kThreads);
  if (g.stream)
    hipLaunchKernelGGL((chain_steps_fwd_kernel<T, IoStream>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((chain_steps_fwd_kernel<T, IoCached>), grid, block, 0, s, a);
  HIP_TRY(hipGetLastError(), "chain_steps_fwd launch");
  return EXPO_OK;
}

// (declared in host_common.h) Does a chain call over these activations run on the dwordx3 vector path?  Whole
// 12-byte vectors per image and 4-byte aligned bases: an image then starts a multiple of 12 bytes behind its base, so
// the answer holds for every chunk of the plan.
bool chain_steps_vec_path(void* const* acts, int steps, int h, int w, int dtype) {
  const int ppv = dtype == EXPO_F16 ? VecTraits<half_t>::PPV : VecTraits<float>::PPV;
  if ((long(h) * w) % ppv != 0) return false;
  for (int k = 0; k <= steps; ++k)
    if ((reinterpret_cast<uintptr_t>(acts[k]) & 3) != 0) return false;
  return true;
}

// (declared in host_common.h) Steps [0, cnt) of ids / acts / params on images [nb, nb + np) in one launch; the caller
// has asked chain_steps_vec_path.
int chain_steps_fwd(const int* ids, int cnt, void* const* acts, const float* const* params, int nb, int np, int h,
                    int w, int dtype, int n_geom, hipStream_t s) {
  if (cnt < 1 || cnt > kChainFuseMax) return fail(EXPO_E_BADARG, "chain_steps_fwd: step count");
  const size_t ioff = size_t(nb) * h * w * 3 * (dtype == EXPO_F16 ? 2 : 4);
  ChainStepsFwdArgs a{};
  a.x = static_cast<const char*>(acts[0]) + ioff;
  for (int k = 0; k < cnt; ++k) {
    a.y[k] = static_cast<char*>(acts[k + 1]) + ioff;
    a.prm[k] = params[k] + size_t(nb) * kNumParams[ids[k]];
    a.id[k] = ids[k];
  }
  a.steps = cnt;
  a.hw = h * w;
  return dtype == EXPO_F16 ? chain_steps_fwd_t<half_t>(a, np, h, w, n_geom, s)
                           : chain_steps_fwd_t<float>(a, np, h, w, n_geom, s);
}

}  // namespace expo
