// chain_fused.hip -- the fused multi-step forward of the high-resolution inference path
// (expo_chain_fused_fwd; /root/reference/net.py:796-821, BASELINE config 5), in its own translation unit
// because it is compiled with -fno-slp-vectorize: this kernel is compute-heavy (8 filter bodies back to
// back on values that stay in registers), and clang's SLP vectoriser turns pairs of independent fp32
// operations into v_pk_mul_f32 / v_pk_fma_f32 plus the v_mov's that assemble their operand pairs.  The
// packed forms issue at the scalar rate on gfx950 (tools/valubench), but the kernel is bound by its
// dependent chains, not by issue slots (SQ counters, profiles/r02_experiments.md r02p18/19), so the
// packing buys nothing and the moves cost: 1 203 VALU with 216 v_mov -> 24.6 us, against 1 262
// scalar VALU with 102 v_mov -> 22.7 us at 16x512x512x3 fp16 (gpurun r02p5); a hand-paired build with
// 963 VALU measured the same as this one.  The streaming kernels of exposure_hip.hip keep the default
// (-0.8 % for the chain with the flag).
// -fno-honor-nans drops the canonicalising v_max_f32 x, x, x in front of every min / max / med3 whose
// operand comes from memory or LDS (1 218 -> 1 171 VALU): a NaN pixel is not a defined input of the
// inference path (the result for such a pixel is unspecified; every other pixel is unaffected).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/exposure_hip.h"
#include "filter_math.h"
#include "pixel_io.h"
#include "kernel_common.h"
#include "host_common.h"
#include "ragged_launch.h"

#ifndef EXPO_FUSED_MIN_WAVES
#define EXPO_FUSED_MIN_WAVES  // e.g. -DEXPO_FUSED_MIN_WAVES=,8 : register budget for 8 waves per SIMD (probe builds)
#endif
#ifndef EXPO_TAPS_MIN_WAVES
#define EXPO_TAPS_MIN_WAVES  // the same for the tap kernels (,4 spills the fp16 u8 kernels: 128 VGPRs are too few)
#endif

namespace expo {

// ------------------------------------------------------- fused multi-step forward (inference)
// The high-resolution inference path (net.py:796-821; BASELINE config 5): the per-step parameters
// are regressed on the 64x64 proxy only, so by the time the full-resolution image is touched the
// whole per-image sequence (filter id, parameters) x steps is known.  These kernels apply all
// `steps` filters to a pixel group while it sits in registers (fp32 between steps -- no fp16
// rounding of intermediates): ONE read and ONE write of the image instead of one per step.
// Each wave owns exactly one 3 KiB chunk, so the per-step parameters are fetched once per wave
// through scalar loads; the step loop is rolled (block-uniform switch per step).
//
// chain_fused_run is that step loop for the PPL pixels of one group (v, fp32, in place): image sequence idn[steps] /
// prn[steps][EXPO_MAX_PARAMS] (wave-uniform), `tab` this wave's curve table in LDS, `plane` the parameter this lane
// mirrors for the curve builds.  Shared by the dense kernel (one (N, H, W, 3) tensor) and the ragged one (a list of
// images of any sizes).
// `tap(k, out)` sees the image after step k (the tap kernels below); the default does nothing and the kernels without
// taps compile to the same code as before it existed.
// chain_step is one step, OUT OF PLACE (in -> out), shared with the masked step loop further down.
template <typename T>
__device__ __forceinline__ void chain_step(int id, const float* prm, float klane, float2_lut* tab, const float* in,
                                           float* out) {
  constexpr int PPL = PixTraits<T>::PPL;
#define EXPO_CASE(ID, F)                              \
  case ID: {                                          \
    const typename F::Prm q = F::load(prm);           \
    _Pragma("unroll") for (int k = 0; k < PPL; ++k) F::fwd(q, in + 3 * k, out + 3 * k); \
  } break;
  switch (id) {
    EXPO_CASE(0, ExposureF)
    EXPO_CASE(1, GammaF)
    EXPO_CASE(2, WhiteBalanceF)
    EXPO_CASE(3, SatPlusF)
    case 4:
      curve_lut_build<1>(klane, tab);
      curve_lut_map<1, PPL>(in, out, tab);
      __builtin_amdgcn_wave_barrier();  // the next curve step of this wave rewrites the table
      break;
    EXPO_CASE(5, ContrastF)
    EXPO_CASE(6, WnbF)
    case 7:
      curve_lut_build<3>(klane, tab);
      curve_lut_map<3, PPL>(in, out, tab);
      __builtin_amdgcn_wave_barrier();
      break;
    EXPO_CASE(8, LevelF)
    default:  // id -1 (the all-zero one-hot selects nothing) -> the image becomes 0.  Written as arithmetic (clamp,
      // then x * 0 + 0: exactly +0 for every input incl. inf / NaN) rather than as 24 constant moves: those the
      // compiler executes speculatively in front of the neighbouring case (Exposure) on EVERY step.  (No
      // __builtin_unreachable() for ids outside [-1, 8] either: with it hipcc 7.2 drops the first two values of the
      // fp32 kernel's first pixel row -- found by the fp32 parity test, gpurun r03p17.)
#pragma unroll
      for (int j = 0; j < PPL * 3; ++j) out[j] = fmaf(clamp01x(in[j], -65504.0f, 65504.0f), 0.0f, 0.0f);
      break;
  }
#undef EXPO_CASE
}

struct NoTap { __device__ void operator()(int, const float*) const {} };
template <typename T, class Tap = NoTap>
__device__ inline void chain_fused_run(const int32_t* idn, const float* prn,
                                                int steps, float2_lut* tab, int plane, float* v,
                                                const Tap& tap = Tap()) {
  constexpr int PPL = PixTraits<T>::PPL;
  // The step loop below runs two steps per trip with the two pixel arrays (and the two parameter sets) swapping
  // roles, so no loop-carried value is ever copied: the rolled one-step loop paid 24 v_mov + 24 s_mov per step for its
  // loop PHIs (the coupled filters cannot update a pixel in place), ~17 % of the instructions a wave issued for an
  // 8-step sequence.
  auto apply = [&](int id, const float* prm, float klane, const float* in, float* out) {
    chain_step<T>(id, prm, klane, tab, in, out);
  };
  // software-pipelined parameter fetch: a step's id and 24 parameters (wave-uniform -> scalar loads into SGPRs)
  // are requested one step ahead, hiding the scalar-load latency; `k*` is a per-lane copy (lane l <-> parameter l)
  // for the curve table.  Two parameter sets alternate like the pixel arrays.
  float pa[EXPO_MAX_PARAMS], pb[EXPO_MAX_PARAMS];
  float ka = 0.f, kb = 0.f;
  int ia = 0, ib = 0;
  // a step past the end (the second half of the last trip of an odd-length sequence) is the identity: Exposure with
  // 0 EV, x * 2^0 = x exactly -- no extra case in the switch
  auto fetch = [&](int st, float* p, float& kl, int& id) {
    const bool live = st < steps;
    const int sn = live ? st : steps - 1;  // (past the end: any valid row)
    id = live ? idn[sn] : 0;
    kl = prn[sn * EXPO_MAX_PARAMS + plane];
#pragma unroll
    for (int j = 0; j < EXPO_MAX_PARAMS; ++j) p[j] = prn[sn * EXPO_MAX_PARAMS + j];
    if (!live) p[0] = 0.0f;
  };
  if (steps <= 0) return;
  // (the pixel arrays are locals, copied in and out -- free in SSA form.  Running the loop directly on the caller's
  // array made hipcc 7.2 allocate the fp32 kernel's store ADDRESS register inside the 96-bit data tuple of the first
  // pixel row: R and G of every 64th pixel wrong.  Caught by the fp32 parity tests, gpurun r03p17;
  // tests/test_isa_sanity.py now scans every kernel's ISA for that overlap.)
  float a[PPL * 3], w[PPL * 3];
#pragma unroll
  for (int j = 0; j < PPL * 3; ++j) a[j] = v[j];
  fetch(0, pa, ka, ia);
#pragma unroll 1
  for (int st = 0; st < steps; st += 2) {
    fetch(st + 1, pb, kb, ib);
    apply(ia, pa, ka, a, w);
    tap(st, w);
    fetch(st + 2, pa, ka, ia);
    apply(ib, pb, kb, w, a);
    tap(st + 1, a);  // (st + 1 == steps: the identity half-trip, never a tap)
  }
#pragma unroll
  for (int j = 0; j < PPL * 3; ++j) v[j] = a[j];
}

// The pixel loop of one image's share of the grid: wave chunks first_gw, first_gw + stride, ... (VEC: the dwordx3
// buffer path of pixel_io.h; otherwise the element-wise path, whose trip count is kept wave-uniform because the curve
// builds need lanes 0..23 of every wave alive -- groups past the end load zeros and store nothing).
template <typename T, bool VEC, class IO>
__device__ __forceinline__ void chain_fused_image(const int32_t* idn, const float* prn, int steps, const T* xi, T* yi,
                                                  int hw,
                                                  int groups, int first_gw, int stride, float2_lut* tab) {
  constexpr int PPL = PixTraits<T>::PPL;
  const int plane = (threadIdx.x & 63) % EXPO_MAX_PARAMS;  // which parameter this lane mirrors
  auto run = [&](float* v) { chain_fused_run<T>(idn, prn, steps, tab, plane, v); };
  if constexpr (VEC) {
    const T* const ins[1] = {xi};
    stream_groups<T, 1, true, false, IO>(ins, yi, hw, first_gw, stride,
                                         [&](float (&v)[1][PPL * 3], int) { run(v[0]); });
  } else {
    for (int g0 = first_gw; g0 < groups; g0 += stride) {
      const int g = g0 + (threadIdx.x & 63);
      float v[PPL * 3];
      load_slow<T>(xi, g, hw, v);
      run(v);
      store_slow<T>(yi, g, hw, v);
    }
  }
}

template <typename T, bool VEC, class IO>
__global__ __launch_bounds__(kThreads EXPO_FUSED_MIN_WAVES) void chain_fused_fwd_kernel(const int32_t* __restrict__ ids,
                                                                   const float* __restrict__ params, int steps,
                                                                   const T* __restrict__ x, T* __restrict__ y,
                                                                   int hw, int groups) {
  constexpr int PPL = PixTraits<T>::PPL;
  const int n = blockIdx.y;
  const size_t off = size_t(n) * hw * 3;
  const T* xi = x + off;
  T* yi = y + off;
  const int32_t* idn = ids + size_t(n) * steps;
  const float* prn = params + size_t(n) * steps * EXPO_MAX_PARAMS;
  __shared__ float2_lut curve_tab[kWaves][32];
  float2_lut* const tab = curve_tab[threadIdx.x >> 6];
  const int plane = (threadIdx.x & 63) % EXPO_MAX_PARAMS;  // which parameter this lane mirrors
  auto run = [&](float* v) { chain_fused_run<T>(idn, prn, steps, tab, plane, v); };
  const int stride = gridDim.x * kThreads;
  if constexpr (VEC) {
    const T* const ins[1] = {xi};
    stream_groups<T, 1, true, false, IO>(ins, yi, hw, blockIdx.x * kThreads + (threadIdx.x & ~63), stride,
                                     [&](float (&v)[1][PPL * 3], int) { run(v[0]); });
  } else {
    // wave-uniform trip count: curve_fwd_lut needs lanes 0..23 of every wave alive (groups past the
    // end load zeros and store nothing)
    for (int g0 = blockIdx.x * kThreads + (threadIdx.x & ~63); g0 < groups; g0 += stride) {
      const int g = g0 + (threadIdx.x & 63);
      float v[PPL * 3];
      load_slow<T>(xi, g, hw, v);
      run(v);
      store_slow<T>(yi, g, hw, v);
    }
  }
}

// ------------------------------------------------------- ragged: a list of images of any sizes in one launch
// The chain is per pixel: an image matters to it through its base address and pixel count only.  The grid is 1-D
// over the images' blocks laid end to end (image i: ceil(groups_i / kThreads) blocks, one chunk per wave as above);
// the table of up to kRaggedMaxImages images travels BY VALUE in the kernel arguments (no library-owned device
// memory, no copy; 1.6 KB of the 4 KB kernarg block).  A block finds its image by a binary search over `first` with the
// block index -- uniform, so the search, the image's pointers, its pixel count and its ids / params row are all scalar.
// The host side -- the checks of a call, its split into launches, the tables' first / n / vec and the choice among
// (IoStream | IoCached) x ANY_SLOW -- is ragged_launch.h's for every ragged pass; DESIGN.md §3.31 states its contract.
template <typename T>
struct RaggedTable {
  const T* x[kRaggedMaxImages];
  T* y[kRaggedMaxImages];
  int hw[kRaggedMaxImages];
  int first[kRaggedMaxImages + 1];  // first block of image i; first[n] = the grid's size
  int n;
  uint64_t vec;  // bit i: image i takes the dwordx3 path (the decision make_geom takes for one image)
};

// ANY_SLOW: some image of this launch needs the element-wise path (instantiated apart so that an all-vector launch
// carries exactly the dense kernel's vector code and register budget)
template <typename T, class IO, bool ANY_SLOW>
__global__ __launch_bounds__(kThreads EXPO_FUSED_MIN_WAVES) void chain_fused_fwd_ragged_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, int steps, const RaggedTable<T> tab) {
  __shared__ float2_lut curve_tab[kWaves][32];
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;  // the last image whose first block is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int i = __builtin_amdgcn_readfirstlane(lo);
  constexpr int PPL = PixTraits<T>::PPL;
  const int hw = tab.hw[i];
  const int groups = (hw + PPL - 1) / PPL;
  const int first_gw = (b - tab.first[i]) * kThreads + (threadIdx.x & ~63);
  const int stride = (tab.first[i + 1] - tab.first[i]) * kThreads;  // one trip: the image's blocks cover its groups
  const int32_t* idn = ids + size_t(i) * steps;
  const float* prn = params + size_t(i) * steps * EXPO_MAX_PARAMS;
  float2_lut* const lut = curve_tab[threadIdx.x >> 6];
  if (!ANY_SLOW || ((tab.vec >> i) & 1))
    chain_fused_image<T, true, IO>(idn, prn, steps, tab.x[i], tab.y[i], hw, groups, first_gw, stride, lut);
  else
    chain_fused_image<T, false, IO>(idn, prn, steps, tab.x[i], tab.y[i], hw, groups, first_gw, stride, lut);
}

// ------------------------------------------------------- taps: the image after chosen steps, from the same pass
// The step-by-step pictures of net.py:820-823 without reading the image back: after every step k whose bit is set in
// the (uniform) tap_mask, the running fp32 values of the pixel group are also written to tap plane j = the number of
// set bits below k.  Separate instantiations: the kernels above keep their code.
//   EXPO_TAP_STORAGE: pack<T> / store_slow<T>, the very stores of y -- the tap is what the truncated sequence writes.
//   EXPO_TAP_U8: the value rounded to T first, then saturate(rint(s * 255)).  A plane is 3 B/px and may start at any
//   byte, so on the vector path a lane's 6 (fp16) / 3 (fp32) bytes per 12-byte input vector do not map onto dwords:
//   they are staged in a per-wave LDS buffer (the wave's chunk as one contiguous 1536 / 768-byte run) and leave as
//   coalesced buffer_store_dword; a dword that is not 4-byte aligned or straddles the plane's end goes out as four
//   bounds-checked buffer_store_byte instead (exact, slower).  The element-wise path stores bytes.
//   EXPO_TAP_U16: as U8 with 65535 and little-endian shorts, 6 B/px; a plane may start at any 2-byte boundary.
//   fp32 storage: a lane's pixel per input vector is 6 bytes -- staged like U8 (1536 bytes per wave); a dword that is
//   misaligned (plane base 2 mod 4: every odd-sized plane of a dense tap tensor but the first) or straddles the plane's
//   end leaves as two bounds-checked buffer_store_short.  fp16 storage: a lane's two pixels per input vector are 12
//   bytes at exactly the storage tap's byte positions, so the codes leave as dwordx3 like EXPO_TAP_STORAGE, no
//   staging; the host side then puts the plane's base into the image's alignment test (tap_vector_store), and an
//   image whose plane is only 2-byte aligned takes the element-wise path, which stores shorts.
template <typename T>
__device__ __forceinline__ float tap_u8_level(float v) {
  const float s = float(T(v));  // rounded to the storage dtype (saturating like pack<T>; either way -> 255)
  return __builtin_amdgcn_fmed3f(__builtin_rintf(s * 255.0f), 0.0f, 255.0f);
}

template <typename T>
__device__ __forceinline__ float tap_u16_level(float v) {
  const float s = float(T(v));  // as tap_u8_level; one fp32 multiply, round half even, clamp
  return __builtin_amdgcn_fmed3f(__builtin_rintf(s * 65535.0f), 0.0f, 65535.0f);
}
template <typename T>
__device__ __forceinline__ uint32_t tap_u16_pair(float lo, float hi) {  // two codes, little-endian in one dword
  return uint32_t(tap_u16_level<T>(lo)) | (uint32_t(tap_u16_level<T>(hi)) << 16);
}

// bytes per channel value of a tap plane
template <typename T, int FMT>
constexpr int tap_elem_bytes() { return FMT == EXPO_TAP_U8 ? 1 : FMT == EXPO_TAP_U16 ? 2 : int(sizeof(T)); }
// the vector path writes the plane with the dwordx3 stores of y: its base must be 4-byte aligned like y's
template <typename T, int FMT>
constexpr bool tap_vector_store() { return FMT == EXPO_TAP_STORAGE || (FMT == EXPO_TAP_U16 && sizeof(T) == 2); }

template <typename T, bool VEC, class IO, int FMT>
struct TapSink {
  static constexpr int ES = tap_elem_bytes<T, FMT>();
  static constexpr int VPR = 3 * VecTraits<T>::PPV;  // values per lane and 12-byte input vector (a lane's row)
  static constexpr int BPR = VPR * ES;               // their bytes in a u8 / u16 plane
  char* base;        // plane 0 of this image
  size_t stride;     // bytes from plane j to plane j + 1
  uint64_t mask;
  int hw;
  uint8_t* stage;    // this wave's 4 * 64 * BPR bytes of LDS (u8 vector path, u16 vector path of fp32 storage)

  // store the values v (the group of lane `lane`, starting at wave chunk gw; element-wise path: group g = gw + lane)
  __device__ __forceinline__ void operator()(int k, int gw, int lane, const float* v) const {
    if (!((mask >> k) & 1)) return;
    constexpr int PPL = PixTraits<T>::PPL;
    const int j = __builtin_popcountll(mask & ((uint64_t(1) << k) - 1));
    char* const plane = base + size_t(j) * stride;
    if constexpr (!VEC) {
      if constexpr (FMT == EXPO_TAP_STORAGE) {
        store_slow<T>(reinterpret_cast<T*>(plane), gw + lane, hw, v);
      } else if constexpr (FMT == EXPO_TAP_U16) {
        uint16_t* const p = reinterpret_cast<uint16_t*>(plane);
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
          const int px = (gw + lane) * PPL + q;
          if (px < hw) {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[size_t(px) * 3 + c] = uint16_t(uint32_t(tap_u16_level<T>(v[q * 3 + c])));
          }
        }
      } else {
        uint8_t* const p = reinterpret_cast<uint8_t*>(plane);
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
          const int px = (gw + lane) * PPL + q;
          if (px < hw) {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[size_t(px) * 3 + c] = uint8_t(uint32_t(tap_u8_level<T>(v[q * 3 + c])));
          }
        }
      }
    } else if constexpr (FMT == EXPO_TAP_STORAGE) {
      store_raw<IO::kStore>(make_image_rsrc(reinterpret_cast<T*>(plane), hw), chunk_byte_offset<T>(gw, lane), pack<T>(v));
    } else if constexpr (FMT == EXPO_TAP_U16 && sizeof(T) == 2) {
      // two bytes per value like the storage tap: the same byte positions, the same stores (4-byte aligned plane)
      RawGroup r;
#pragma unroll
      for (int row = 0; row < 4; ++row) {
#pragma unroll
        for (int e = 0; e < 3; ++e) r.q[row][e] = tap_u16_pair<T>(v[row * 6 + e * 2], v[row * 6 + e * 2 + 1]);
      }
      store_raw<IO::kStore>(make_image_rsrc(reinterpret_cast<T*>(plane), hw), chunk_byte_offset<T>(gw, lane), r);
    } else {
      const int nbytes = hw * 3 * ES;
      const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(plane, 0, nbytes, kBufferRsrcFlags);
      // v holds 4 input vectors (rows of the chunk, 64 * BPR bytes apart in the plane), VPR values each in memory order
#pragma unroll
      for (int row = 0; row < 4; ++row) {
        uint8_t* const dst = stage + row * 64 * BPR + lane * BPR;
        if constexpr (FMT == EXPO_TAP_U16) {  // (fp32 storage: 3 shorts, 2-byte aligned in the stage)
#pragma unroll
          for (int e = 0; e < VPR; ++e) {
            const uint16_t h = uint16_t(uint32_t(tap_u16_level<T>(v[row * VPR + e])));
            __builtin_memcpy(dst + 2 * e, &h, 2);
          }
        } else if constexpr (BPR % 2 == 0) {
#pragma unroll
          for (int e = 0; e < BPR; e += 2) {
            uint32_t u = __builtin_amdgcn_cvt_pk_u8_f32(tap_u8_level<T>(v[row * BPR + e]), 0, 0);
            u = __builtin_amdgcn_cvt_pk_u8_f32(tap_u8_level<T>(v[row * BPR + e + 1]), 1, u);
            const uint16_t h = uint16_t(u);
            __builtin_memcpy(dst + e, &h, 2);
          }
        } else {
#pragma unroll
          for (int e = 0; e < BPR; ++e) dst[e] = uint8_t(uint32_t(tap_u8_level<T>(v[row * BPR + e])));
        }
      }
      __builtin_amdgcn_wave_barrier();  // one wave: its LDS operations execute in order
      const bool aligned = (reinterpret_cast<uintptr_t>(plane) & 3) == 0;
      const int chunk = gw * PPL * 3 * ES;  // the chunk's first byte in the plane
#pragma unroll
      for (int q = 0; q < BPR; ++q) {  // 4 * 64 * BPR bytes = BPR dwords per lane
        uint32_t d;
        __builtin_memcpy(&d, stage + (q * 64 + lane) * 4, 4);
        const int o = chunk + (q * 64 + lane) * 4;
        if (aligned && o + 4 <= nbytes) {
          __builtin_amdgcn_raw_buffer_store_b32(d, r, o, 0, IO::kStore);
        } else if constexpr (FMT == EXPO_TAP_U16) {  // a short past the plane's end is dropped by the bounds check
          __builtin_amdgcn_raw_buffer_store_b16(uint16_t(d), r, o, 0, IO::kStore);
          __builtin_amdgcn_raw_buffer_store_b16(uint16_t(d >> 16), r, o + 2, 0, IO::kStore);
        } else {  // bytes past the plane's end are dropped by the buffer's bounds check
#pragma unroll
          for (int b = 0; b < 4; ++b) __builtin_amdgcn_raw_buffer_store_b8(uint8_t(d >> (8 * b)), r, o + b, 0, IO::kStore);
        }
      }
      __builtin_amdgcn_wave_barrier();  // the next tap of this wave rewrites the buffer
    }
  }
};

template <typename T, int FMT>
struct TapStage {
  // the formats staged on the vector path: 4 rows x 64 lanes x a lane's bytes per row (TapSink::BPR)
  static constexpr bool kStaged = FMT == EXPO_TAP_U8 || (FMT == EXPO_TAP_U16 && sizeof(T) == 4);
  static constexpr int kBytes = kStaged ? 4 * 64 * 3 * VecTraits<T>::PPV * tap_elem_bytes<T, FMT>() : 4;
};

// chain_fused_image with taps; yi may be NULL (taps only)
template <typename T, bool VEC, class IO, int FMT>
__device__ __forceinline__ void chain_fused_image_taps(const int32_t* idn, const float* prn, int steps, const T* xi,
                                                       T* yi, int hw, int groups, int first_gw, int stride,
                                                       float2_lut* tab, const TapSink<T, VEC, IO, FMT>& sink) {
  constexpr int PPL = PixTraits<T>::PPL;
  const int lane = threadIdx.x & 63;
  const int plane = lane % EXPO_MAX_PARAMS;
  if constexpr (VEC) {
#if EXPO_FP16_OVFL
    // the fp16 stores (y and storage taps) saturate as in stream_groups, which sets this only when it stores itself
    if constexpr (sizeof(T) == 2) __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
#endif
    const T* const ins[1] = {xi};
    const __amdgpu_buffer_rsrc_t ry = make_image_rsrc(yi, hw);
    stream_groups<T, 1, false, true, IO>(ins, nullptr, hw, first_gw, stride, [&](float (&v)[1][PPL * 3], int g) {
      const int gw = g - lane;
      chain_fused_run<T>(idn, prn, steps, tab, plane, v[0], [&](int k, const float* o) { sink(k, gw, lane, o); });
      if (yi) store_raw<IO::kStore>(ry, chunk_byte_offset<T>(gw, lane), pack<T>(v[0]));
    });
  } else {
    for (int g0 = first_gw; g0 < groups; g0 += stride) {
      const int g = g0 + lane;
      float v[PPL * 3];
      load_slow<T>(xi, g, hw, v);
      chain_fused_run<T>(idn, prn, steps, tab, plane, v, [&](int k, const float* o) { sink(k, g0, lane, o); });
      if (yi) store_slow<T>(yi, g, hw, v);
    }
  }
}

template <typename T, bool VEC, class IO, int FMT>
__global__ __launch_bounds__(kThreads EXPO_TAPS_MIN_WAVES) void chain_fused_fwd_taps_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, int steps, const T* __restrict__ x,
    T* __restrict__ y, int hw, int groups, uint64_t tap_mask, char* __restrict__ taps, int n_images) {
  __shared__ float2_lut curve_tab[kWaves][32];
  __shared__ __attribute__((aligned(4))) uint8_t tap_stage[kWaves][TapStage<T, FMT>::kBytes];
  using Sink = TapSink<T, VEC, IO, FMT>;
  const int n = blockIdx.y;
  const size_t off = size_t(n) * hw * 3;
  const size_t plane_bytes = size_t(hw) * 3 * Sink::ES;
  const Sink sink{taps + size_t(n) * plane_bytes, size_t(n_images) * plane_bytes, tap_mask, hw,
                  tap_stage[threadIdx.x >> 6]};
  chain_fused_image_taps<T, VEC, IO, FMT>(ids + size_t(n) * steps, params + size_t(n) * steps * EXPO_MAX_PARAMS, steps,
                                          x + off, y ? y + off : nullptr, hw, groups,
                                          blockIdx.x * kThreads + (threadIdx.x & ~63), gridDim.x * kThreads,
                                          curve_tab[threadIdx.x >> 6], sink);
}

// the ragged table plus one tap buffer per image (512 B more by value; the kernarg block stays under 4 KB)
template <typename T>
struct RaggedTapTable {
  RaggedTable<T> t;
  char* taps[kRaggedMaxImages];
};

template <typename T, class IO, bool ANY_SLOW, int FMT>
__global__ __launch_bounds__(kThreads EXPO_TAPS_MIN_WAVES) void chain_fused_fwd_ragged_taps_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, int steps, uint64_t tap_mask,
    const RaggedTapTable<T> tt) {
  __shared__ float2_lut curve_tab[kWaves][32];
  __shared__ __attribute__((aligned(4))) uint8_t tap_stage[kWaves][TapStage<T, FMT>::kBytes];
  const RaggedTable<T>& tab = tt.t;
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;  // the last image whose first block is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int i = __builtin_amdgcn_readfirstlane(lo);
  constexpr int PPL = PixTraits<T>::PPL;
  const int hw = tab.hw[i];
  const int groups = (hw + PPL - 1) / PPL;
  const int first_gw = (b - tab.first[i]) * kThreads + (threadIdx.x & ~63);
  const int stride = (tab.first[i + 1] - tab.first[i]) * kThreads;
  const int32_t* idn = ids + size_t(i) * steps;
  const float* prn = params + size_t(i) * steps * EXPO_MAX_PARAMS;
  float2_lut* const lut = curve_tab[threadIdx.x >> 6];
  uint8_t* const stage = tap_stage[threadIdx.x >> 6];
  const size_t plane_bytes = size_t(hw) * 3 * TapSink<T, true, IO, FMT>::ES;
  if (!ANY_SLOW || ((tab.vec >> i) & 1)) {
    const TapSink<T, true, IO, FMT> sink{tt.taps[i], plane_bytes, tap_mask, hw, stage};
    chain_fused_image_taps<T, true, IO, FMT>(idn, prn, steps, tab.x[i], tab.y[i], hw, groups, first_gw, stride, lut, sink);
  } else {
    const TapSink<T, false, IO, FMT> sink{tt.taps[i], plane_bytes, tap_mask, hw, stage};
    chain_fused_image_taps<T, false, IO, FMT>(idn, prn, steps, tab.x[i], tab.y[i], hw, groups, first_gw, stride, lut,
                                              sink);
  }
}

template <typename T>
static int chain_fused_fwd_t(const int32_t* ids, const float* params, int steps, const void* x, void* y, int n,
                             int h, int w, hipStream_t s) {
  Geom g = make_geom<T>(n, h, w, {x, y}, kGeomMap);
  g.blocks_x = (g.groups + kThreads - 1) / kThreads;  // one chunk per wave: parameters fetched once
  const dim3 grid(g.blocks_x, n), block(kThreads);
  if (g.stream)
    hipLaunchKernelGGL((chain_fused_fwd_kernel<T, true, IoStream>), grid, block, 0, s, ids, params, steps, (const T*)x, (T*)y, g.hw, g.groups);
  else if (g.vec)
    hipLaunchKernelGGL((chain_fused_fwd_kernel<T, true, IoCached>), grid, block, 0, s, ids, params, steps, (const T*)x, (T*)y, g.hw, g.groups);
  else
    hipLaunchKernelGGL((chain_fused_fwd_kernel<T, false, IoCached>), grid, block, 0, s, ids, params, steps, (const T*)x, (T*)y, g.hw, g.groups);
  HIP_TRY(hipGetLastError(), "chain_fused_fwd launch");
  return EXPO_OK;
}

// ragged_launches' `fill` (ragged_launch.h) for the plain table; ys NULL = no image output
template <typename T>
static auto ragged_fill(const void* const* xs, void* const* ys, const int* hs, const int* ws) {
  return [=](RaggedTable<T>& tab, int j, int i) {
    tab.x[j] = static_cast<const T*>(xs[i]);
    tab.y[j] = ys ? static_cast<T*>(ys[i]) : nullptr;
    tab.hw[j] = hs[i] * ws[i];
    return ragged_addr(xs[i]) | ragged_addr(tab.y[j]);
  };
}

// arguments validated by the caller; the launches are ragged_launches', in order on stream s
template <typename T>
static int chain_fused_fwd_ragged_t(const int32_t* ids, const float* params, int steps, const void* const* xs,
                                    void* const* ys, const int* hs, const int* ws, int n, hipStream_t s) {
  return ragged_launches<T, RaggedTable<T>>(
      hs, ws, n, ragged_fill<T>(xs, ys, hs, ws),
      [&](auto io, auto any_slow, dim3 grid, int base, const RaggedTable<T>& tab) {
        hipLaunchKernelGGL((chain_fused_fwd_ragged_kernel<T, decltype(io), decltype(any_slow)::value>), grid,
                           dim3(kThreads), 0, s, ids + size_t(base) * steps,
                           params + size_t(base) * steps * EXPO_MAX_PARAMS, steps, tab);
        HIP_TRY(hipGetLastError(), "chain_fused_fwd_ragged launch");
        return EXPO_OK;
      });
}

// arguments validated by the caller; tap_mask != 0
template <typename T, int FMT>
static int chain_fused_fwd_taps_t(const int32_t* ids, const float* params, int steps, const void* x, void* y, int n,
                                  int h, int w, uint64_t tap_mask, void* taps, hipStream_t s) {
  // a storage tap plane is stored like y (dwordx3), and so is a u16 plane of fp16 storage: its base joins the
  // alignment test; u8 planes and the u16 planes of fp32 storage handle any base
  Geom g = make_geom<T>(n, h, w, {x, y, tap_vector_store<T, FMT>() ? taps : nullptr}, kGeomMap);
  g.blocks_x = (g.groups + kThreads - 1) / kThreads;
  const dim3 grid(g.blocks_x, n), block(kThreads);
  const T* xt = static_cast<const T*>(x);
  T* yt = static_cast<T*>(y);
  char* tp = static_cast<char*>(taps);
  if (g.stream)
    hipLaunchKernelGGL((chain_fused_fwd_taps_kernel<T, true, IoStream, FMT>), grid, block, 0, s, ids, params, steps, xt, yt, g.hw, g.groups, tap_mask, tp, n);
  else if (g.vec)
    hipLaunchKernelGGL((chain_fused_fwd_taps_kernel<T, true, IoCached, FMT>), grid, block, 0, s, ids, params, steps, xt, yt, g.hw, g.groups, tap_mask, tp, n);
  else
    hipLaunchKernelGGL((chain_fused_fwd_taps_kernel<T, false, IoCached, FMT>), grid, block, 0, s, ids, params, steps, xt, yt, g.hw, g.groups, tap_mask, tp, n);
  HIP_TRY(hipGetLastError(), "chain_fused_fwd_taps launch");
  return EXPO_OK;
}

// the same with a tap buffer per image.  A storage tap plane is stored like y (dwordx3), and so is a u16 plane of fp16
// storage: its base joins the alignment test (tap_vector_store); u8 planes and the u16 planes of fp32 storage take any.
template <typename T, int FMT>
static auto ragged_taps_fill(const void* const* xs, void* const* ys, const int* hs, const int* ws, void* const* taps) {
  return [=](RaggedTapTable<T>& tt, int j, int i) {
    tt.taps[j] = static_cast<char*>(taps[i]);
    return ragged_fill<T>(xs, ys, hs, ws)(tt.t, j, i) | (tap_vector_store<T, FMT>() ? ragged_addr(taps[i]) : 0);
  };
}

// arguments validated by the caller; tap_mask != 0, ys NULL = no image output
template <typename T, int FMT>
static int chain_fused_fwd_ragged_taps_t(const int32_t* ids, const float* params, int steps, const void* const* xs,
                                         void* const* ys, const int* hs, const int* ws, int n, uint64_t tap_mask,
                                         void* const* taps, hipStream_t s) {
  return ragged_launches<T, RaggedTapTable<T>>(
      hs, ws, n, ragged_taps_fill<T, FMT>(xs, ys, hs, ws, taps),
      [&](auto io, auto any_slow, dim3 grid, int base, const RaggedTapTable<T>& tt) {
        hipLaunchKernelGGL((chain_fused_fwd_ragged_taps_kernel<T, decltype(io), decltype(any_slow)::value, FMT>), grid,
                           dim3(kThreads), 0, s, ids + size_t(base) * steps,
                           params + size_t(base) * steps * EXPO_MAX_PARAMS, steps, tap_mask, tt);
        HIP_TRY(hipGetLastError(), "chain_fused_fwd_ragged_taps launch");
        return EXPO_OK;
      });
}

// kernel arguments of the ragged tap kernel: ids, params, steps, tap_mask, the table
static_assert(sizeof(RaggedTapTable<half_t>) + 32 <= 4096, "the ragged tap table must fit the 4 KB kernarg block");

// ------------------------------------------------------- masked: the fused pass with cfg.masking on
// Filter.apply with the spatial mask of filters.py:110-148 at every step, fused like the pass above: the mask of a
// pixel needs its (row, column), the luminance of the running value -- what the previous step left in registers -- and
// six per-image numbers per step, so nothing keeps the steps from running back to back on a pixel group.
//   v_{k+1} = fma(m, process(v_k) - v_k, v_k),  m = MaskPrm(mask_params[i][k], ...).eval_rc(row, col, v_k).m
// (the masked lerp of apply_fwd_body, exposure_hip.hip); id -1 makes the image +0 without a mask.
// Coordinates: a group's first (row, column) is found once per group and kept (2 VGPRs); every step re-walks the
// group's other pixels from it with PixelWalk (a few integer operations per pixel, held in step with the pixel
// arithmetic by its ordering anchor) instead of carrying 2 * PPL grid values through the step loop.
// Mask constants: the six numbers of a step are wave-uniform and are fetched one step ahead, with the id and the
// parameters; the image's geometry (grid constants, the walk's steps) is set up once per wave in `geo`.
struct NoSink { __device__ __forceinline__ void operator()(int, int, int, const float*) const {} };

// `geo` with the coefficients of one step's six mask parameters (MaskPrm::load's own arithmetic; its geometry part
// is constant-folded away here)
__device__ __forceinline__ MaskPrm mask_step(MaskPrm geo, const float* mp, float sharp, float min_strength) {
  const MaskPrm s = MaskPrm::load(mp, sharp, min_strength, 1, 1);
  geo.a = s.a; geo.b = s.b; geo.c = s.c; geo.d2 = s.d2; geo.k = s.k; geo.S = s.S;
  return geo;
}

// chain_fused_run with the mask: mpn[steps][6] the image's mask rows, (row0, col0) the group's first pixel
template <typename T, bool VEC, class Tap>
__device__ inline void chain_fused_masked_run(const int32_t* idn, const float* prn, const float* mpn, int steps,
                                              const MaskPrm& geo, float sharp, float min_strength, int row0, int col0,
                                              float2_lut* tab, int plane, float* v, const Tap& tap) {
  constexpr int PPL = PixTraits<T>::PPL;
  // one step, out of place; `masked` is uniform: false for id -1 (the image is +0, whatever the mask) and for the
  // padding half-trip, which therefore stays Exposure with 0 EV alone, x * 2^0 = x exactly for every value
  auto apply = [&](int id, bool masked, const float* prm, const float* mp, float klane, const float* in, float* out) {
    chain_step<T>(id, prm, klane, tab, in, out);
    if (masked) {
      const MaskPrm mk = mask_step(geo, mp, sharp, min_strength);
      int row = row0, col = col0;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (k > 0) mk.pw.step(pixel_step_is_b<T, VEC>(k), row, col);
        const float m = mk.eval_rc(row, col, in + 3 * k).m;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * k + c] = fmaf(m, out[3 * k + c] - in[3 * k + c], in[3 * k + c]);
        PixelWalk::after(row, col, out[3 * k]);
      }
    }
  };
  float pa[EXPO_MAX_PARAMS], pb[EXPO_MAX_PARAMS], qa[6], qb[6];
  float ka = 0.f, kb = 0.f;
  int ia = 0, ib = 0;
  bool ma = false, mb = false;
  auto fetch = [&](int st, float* p, float* q, float& kl, int& id, bool& masked) {
    const bool live = st < steps;
    const int sn = live ? st : steps - 1;  // (past the end: any valid row)
    id = live ? idn[sn] : 0;
    masked = live && id >= 0;
    kl = prn[sn * EXPO_MAX_PARAMS + plane];
#pragma unroll
    for (int j = 0; j < EXPO_MAX_PARAMS; ++j) p[j] = prn[sn * EXPO_MAX_PARAMS + j];
#pragma unroll
    for (int j = 0; j < 6; ++j) q[j] = mpn[sn * 6 + j];
    if (!live) p[0] = 0.0f;
  };
  if (steps <= 0) return;
  float a[PPL * 3], w[PPL * 3];  // (locals, copied in and out: see chain_fused_run)
#pragma unroll
  for (int j = 0; j < PPL * 3; ++j) a[j] = v[j];
  fetch(0, pa, qa, ka, ia, ma);
#pragma unroll 1
  for (int st = 0; st < steps; st += 2) {
    fetch(st + 1, pb, qb, kb, ib, mb);
    apply(ia, ma, pa, qa, ka, a, w);
    tap(st, w);
    fetch(st + 2, pa, qa, ka, ia, ma);
    apply(ib, mb, pb, qb, kb, w, a);
    tap(st + 1, a);  // (st + 1 == steps: the identity half-trip, never a tap)
  }
#pragma unroll
  for (int j = 0; j < PPL * 3; ++j) v[j] = a[j];
}

// one image's share of the grid, with or without taps (Sink = NoSink); yi may be NULL with taps
template <typename T, bool VEC, class IO, class Sink>
__device__ __forceinline__ void chain_fused_masked_image(const int32_t* idn, const float* prn, const float* mpn,
                                                         int steps, float sharp, float min_strength, const T* xi, T* yi,
                                                         int h, int w, int first_gw, int stride, float2_lut* tab,
                                                         const Sink& sink) {
  constexpr int PPL = PixTraits<T>::PPL;
  const int hw = h * w, groups = (hw + PPL - 1) / PPL;
  const int lane = threadIdx.x & 63;
  const int plane = lane % EXPO_MAX_PARAMS;
  const float none[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const MaskPrm geo = MaskPrm::load(none, sharp, min_strength, h, w, pixel_step_a<T, VEC>(), pixel_step_b<T, VEC>());
  auto run = [&](float* v, int g, int gw) {
    int row0, col0;
    geo.pw.start(pixel_index<T, VEC>(g, 0, lane), row0, col0);
    chain_fused_masked_run<T, VEC>(idn, prn, mpn, steps, geo, sharp, min_strength, row0, col0, tab, plane, v,
                                   [&](int k, const float* o) { sink(k, gw, lane, o); });
  };
  if constexpr (VEC) {
#if EXPO_FP16_OVFL
    // the fp16 stores (y and storage taps) saturate as in stream_groups, which sets this only when it stores itself
    if constexpr (sizeof(T) == 2) __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
#endif
    const T* const ins[1] = {xi};
    const __amdgpu_buffer_rsrc_t ry = make_image_rsrc(yi, hw);
    stream_groups<T, 1, false, false, IO>(ins, nullptr, hw, first_gw, stride, [&](float (&v)[1][PPL * 3], int g) {
      const int gw = g - lane;
      run(v[0], g, gw);
      if (yi) store_raw<IO::kStore>(ry, chunk_byte_offset<T>(gw, lane), pack<T>(v[0]));
    });
  } else {
    for (int g0 = first_gw; g0 < groups; g0 += stride) {  // wave-uniform trip count, as chain_fused_image
      const int g = g0 + lane;
      float v[PPL * 3];
      load_slow<T>(xi, g, hw, v);
      run(v, g, g0);
      if (yi) store_slow<T>(yi, g, hw, v);
    }
  }
}

// the ragged table with each image's height and width (the mask's grid) and its tap buffer
template <typename T>
struct MaskedRaggedTable {
  const T* x[kRaggedMaxImages];
  T* y[kRaggedMaxImages];
  char* taps[kRaggedMaxImages];
  int h[kRaggedMaxImages], w[kRaggedMaxImages];
  int first[kRaggedMaxImages + 1];
  int n;
  uint64_t vec;
};
// kernel arguments: ids, params, mask_params, steps, sharp, min_strength, tap_mask, the table
static_assert(sizeof(MaskedRaggedTable<half_t>) + 48 <= 4096, "the masked ragged table must fit the 4 KB kernarg block");

template <typename T, class IO, bool ANY_SLOW, int FMT>
__global__ __launch_bounds__(kThreads) void chain_fused_masked_ragged_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, const float* __restrict__ mask_params, int steps,
    float sharp, float min_strength, uint64_t tap_mask, const MaskedRaggedTable<T> tab) {
  __shared__ float2_lut curve_tab[kWaves][32];
  __shared__ __attribute__((aligned(4))) uint8_t tap_stage[kWaves][TapStage<T, FMT>::kBytes];
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;  // the last image whose first block is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int i = __builtin_amdgcn_readfirstlane(lo);
  const int h = tab.h[i], w = tab.w[i];
  const int first_gw = (b - tab.first[i]) * kThreads + (threadIdx.x & ~63);
  const int stride = (tab.first[i + 1] - tab.first[i]) * kThreads;
  const int32_t* idn = ids + size_t(i) * steps;
  const float* prn = params + size_t(i) * steps * EXPO_MAX_PARAMS;
  const float* mpn = mask_params + size_t(i) * steps * 6;
  float2_lut* const lut = curve_tab[threadIdx.x >> 6];
  auto image = [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    if constexpr (FMT == kTapNone) {
      chain_fused_masked_image<T, VEC, IO>(idn, prn, mpn, steps, sharp, min_strength, tab.x[i], tab.y[i], h, w,
                                           first_gw, stride, lut, NoSink());
    } else {
      using Sink = TapSink<T, VEC, IO, FMT>;
      const Sink sink{tab.taps[i], size_t(h) * w * 3 * Sink::ES, tap_mask, h * w, tap_stage[threadIdx.x >> 6]};
      chain_fused_masked_image<T, VEC, IO>(idn, prn, mpn, steps, sharp, min_strength, tab.x[i], tab.y[i], h, w,
                                           first_gw, stride, lut, sink);
    }
  };
  if (!ANY_SLOW || ((tab.vec >> i) & 1)) image(std::true_type());
  else image(std::false_type());
}

// ragged_launches' `fill` for the masked table; FMT kTapNone: taps unused; ys NULL = no image output
template <typename T, int FMT>
static auto masked_fill(const void* const* xs, void* const* ys, const int* hs, const int* ws, void* const* taps) {
  return [=](MaskedRaggedTable<T>& tab, int j, int i) {
    tab.x[j] = static_cast<const T*>(xs[i]);
    tab.y[j] = ys ? static_cast<T*>(ys[i]) : nullptr;
    tab.taps[j] = FMT == kTapNone ? nullptr : static_cast<char*>(taps[i]);
    tab.h[j] = hs[i];
    tab.w[j] = ws[i];
    return ragged_addr(xs[i]) | ragged_addr(tab.y[j]) | (tap_vector_store<T, FMT>() ? ragged_addr(tab.taps[j]) : 0);
  };
}

// arguments validated by the caller; FMT kTapNone: tap_mask == 0
template <typename T, int FMT>
static int chain_fused_masked_ragged_t(const int32_t* ids, const float* params, const float* mask_params, int steps,
                                       float sharp, float min_strength, const void* const* xs, void* const* ys,
                                       const int* hs, const int* ws, int n, uint64_t tap_mask, void* const* taps,
                                       hipStream_t s) {
  return ragged_launches<T, MaskedRaggedTable<T>>(
      hs, ws, n, masked_fill<T, FMT>(xs, ys, hs, ws, taps),
      [&](auto io, auto any_slow, dim3 grid, int base, const MaskedRaggedTable<T>& tab) {
        hipLaunchKernelGGL((chain_fused_masked_ragged_kernel<T, decltype(io), decltype(any_slow)::value, FMT>), grid,
                           dim3(kThreads), 0, s, ids + size_t(base) * steps,
                           params + size_t(base) * steps * EXPO_MAX_PARAMS, mask_params + size_t(base) * steps * 6, steps,
                           sharp, min_strength, tap_mask, tab);
        HIP_TRY(hipGetLastError(), "chain_fused_masked_fwd_ragged launch");
        return EXPO_OK;
      });
}

}  // namespace expo

// (chain_fused_codes.hip includes this file for the templates above and defines this: the exports below, and with them
// every instantiation of the kernels above, belong to this unit alone)
#ifndef EXPO_CHAIN_FUSED_TEMPLATES_ONLY
using namespace expo;

extern "C" {

int expo_chain_fused_fwd(const int32_t* filter_ids, const float* params, int steps, const void* x, void* y, int n,
                         int h, int w, int dtype, void* stream) {
  if (int rc = check_common(n, h, w, dtype)) return rc;
  if (steps < 0 || steps > 64) return fail(EXPO_E_BADARG, "steps must be in [0, 64]");
  if (n == 0) return EXPO_OK;
  if (!x || !y || (steps > 0 && (!filter_ids || !params))) return fail(EXPO_E_BADARG, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == EXPO_F16 ? chain_fused_fwd_t<half_t>(filter_ids, params, steps, x, y, n, h, w, s)
                           : chain_fused_fwd_t<float>(filter_ids, params, steps, x, y, n, h, w, s);
}

int expo_chain_fused_fwd_ragged(const int32_t* filter_ids, const float* params, int steps, const void* const* xs,
                                void* const* ys, const int* hs, const int* ws, int n, int dtype, void* stream) {
  bool go;
  if (int rc = ragged_check_args(steps, xs, ys, false, hs, ws, n, dtype, 0, EXPO_TAP_STORAGE, nullptr, true,
                                 filter_ids && params, &go))
    return rc;
  if (!go) return EXPO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == EXPO_F16 ? chain_fused_fwd_ragged_t<half_t>(filter_ids, params, steps, xs, ys, hs, ws, n, s)
                           : chain_fused_fwd_ragged_t<float>(filter_ids, params, steps, xs, ys, hs, ws, n, s);
}

int expo_chain_fused_fwd_taps(const int32_t* filter_ids, const float* params, int steps, const void* x, void* y,
                              int n, int h, int w, int dtype, uint64_t tap_mask, int tap_format, void* taps,
                              void* stream) {
  if (int rc = check_common(n, h, w, dtype)) return rc;
  if (steps < 0 || steps > 64) return fail(EXPO_E_BADARG, "steps must be in [0, 64]");
  if (int rc = check_taps(steps, tap_mask, tap_format)) return rc;
  if (!y && !tap_mask) return fail(EXPO_E_BADARG, "nothing to write (y NULL and tap_mask 0)");
  if (n == 0) return EXPO_OK;
  if (!x || (tap_mask && !taps) || (steps > 0 && (!filter_ids || !params))) return fail(EXPO_E_BADARG, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dispatch_dtype_tap(dtype, tap_mask, tap_format, [&](auto t, auto fmt) {
    using T = decltype(t);
    constexpr int FMT = decltype(fmt)::value;
    if constexpr (FMT == kTapNone) return chain_fused_fwd_t<T>(filter_ids, params, steps, x, y, n, h, w, s);
    else return chain_fused_fwd_taps_t<T, FMT>(filter_ids, params, steps, x, y, n, h, w, tap_mask, taps, s);
  });
}

int expo_chain_fused_fwd_ragged_taps(const int32_t* filter_ids, const float* params, int steps,
                                     const void* const* xs, void* const* ys, const int* hs, const int* ws, int n,
                                     int dtype, uint64_t tap_mask, int tap_format, void* const* taps, void* stream) {
  bool go;
  if (int rc = ragged_check_args(steps, xs, ys, true, hs, ws, n, dtype, tap_mask, tap_format, taps, true,
                                 filter_ids && params, &go))
    return rc;
  if (!go) return EXPO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dispatch_dtype_tap(dtype, tap_mask, tap_format, [&](auto t, auto fmt) {
    using T = decltype(t);
    constexpr int FMT = decltype(fmt)::value;
    if constexpr (FMT == kTapNone) return chain_fused_fwd_ragged_t<T>(filter_ids, params, steps, xs, ys, hs, ws, n, s);
    else return chain_fused_fwd_ragged_taps_t<T, FMT>(filter_ids, params, steps, xs, ys, hs, ws, n, tap_mask, taps, s);
  });
}

int expo_chain_fused_masked_fwd_ragged(const int32_t* filter_ids, const float* params, const float* mask_params,
                                       int steps, float maximum_sharpness, float minimum_strength,
                                       const void* const* xs, void* const* ys, const int* hs, const int* ws, int n,
                                       int dtype, uint64_t tap_mask, int tap_format, void* const* taps, void* stream) {
  bool go;
  if (int rc = ragged_check_args(steps, xs, ys, true, hs, ws, n, dtype, tap_mask, tap_format, taps, true,
                                 filter_ids && params && mask_params, &go))
    return rc;
  if (!go) return EXPO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dispatch_dtype_tap(dtype, tap_mask, tap_format, [&](auto t, auto fmt) {
    return chain_fused_masked_ragged_t<decltype(t), decltype(fmt)::value>(filter_ids, params, mask_params, steps,
                                                                          maximum_sharpness, minimum_strength, xs, ys,
                                                                          hs, ws, n, tap_mask, taps, s);
  });
}

}  // extern "C"
#endif  // EXPO_CHAIN_FUSED_TEMPLATES_ONLY
