// codes_lut.hip -- integer pictures straight from the integer codes of the image files (expo_codes_lut_ragged;
// DESIGN.md §3.24): out_i[p][c] = luts_i[code_i(p, c)] for the 3 output channels (grey replicated, alpha dropped).
// The caller builds the 2^bits-entry tables on the host with its own expressions (evaluate.input_luts: the `linear` and
// `input_tone_mapped` pictures of the reference's GAN.eval), so the device only gathers and the pictures are bit for bit
// the host's.  Default flags (csrc/build.sh): the kernel moves bytes, 1-8 B in and 3 or 6 B out per pixel.
//   vector path       a lane-row is the 12-byte output vector of PPV pixels (uint8 entries 4, uint16 entries 2) at
//                     pixel_io.h's coalesced positions, stored as one dwordx3; its PPV * C codes come in with the widest
//                     loads their size allows (codes_loader.h; 24 and 32 bytes as two loads).  Rows past the end of the
//                     image read code 0 and their stores are dropped by the buffer's bounds check.
//   element-wise path per image, block-uniform: codes or output not 4-byte aligned, or hw % PPV != 0.
//   tables            8-bit codes: staged in LDS once per block.  16-bit codes with uint8 entries (64 KiB): staged in
//                     LDS by blocks that then walk several chunks (`trips`) so the fill is amortised -- the gather
//                     through the caches is bound by L2 requests, as decode_kernel's (profiles/input_pictures.md:
//                     0.19 of the copy rate against 0.95 from LDS); EXPO_CODES_LUT_LDS16=0 selects it all the same.
//                     uint16 entries, or a table that is not 16-byte aligned: through the caches.
#include <limits.h>

#include "codes_loader.h"
#include "host_common.h"

namespace expo {

namespace {

constexpr int kLutMaxImages = 64;
constexpr int kLutRows = 4;        // 12-byte output vectors per lane in a wave's chunk (3 KiB of output per wave)
constexpr int kLutLdsTrips = 16;   // chunks a block of the LDS-staged 16-bit variant walks at most
constexpr long kLutLdsBlocks = 1024;  // ... fewer while the launch would have fewer blocks than this

// up to 64 images by value in the kernel arguments (1.6 KB): codes, output, pixel count, first block of each image
// (first[n] = the grid's size) and a bit per image for the vector path
struct LutTable {
  const void* codes[kLutMaxImages];
  void* out[kLutMaxImages];
  int hw[kLutMaxImages];
  int first[kLutMaxImages + 1];
  int n;
  uint64_t vec;
};
// kernel arguments: the table, luts, lut_stride, trips
static_assert(sizeof(LutTable) + 16 <= 4096, "the table must fit the 4 KB kernarg block");

// the NB code bytes of one lane-row: load_code_row, in two halves beyond 16 bytes
template <typename CT, int NB, int AUX>
__device__ __forceinline__ void load_codes(__amdgpu_buffer_rsrc_t rin, int off, CT* c) {
  if constexpr (NB > 16) {
    load_code_row<CT, NB / 2, AUX>(rin, off, c);
    load_code_row<CT, NB / 2, AUX>(rin, off + NB / 2, c + NB / 2 / int(sizeof(CT)));
  } else {
    load_code_row<CT, NB, AUX>(rin, off, c);
  }
}

// LDS16: 16-bit codes with the table staged in LDS (uint8 entries; the table is 16-byte aligned); a block walks up to
// `trips` consecutive chunks of its image (1 in every other variant)
template <typename CT, int C, typename OT, class IO, bool LDS16>
__global__ __launch_bounds__(kThreads) void codes_lut_kernel(const LutTable tab, const OT* __restrict__ luts,
                                                             int lut_stride, int trips) {
  constexpr int BITS = 8 * int(sizeof(CT));
  constexpr bool LDS = BITS == 8 || LDS16;
  constexpr int PPV = 12 / (3 * int(sizeof(OT)));
  constexpr int CHUNK_PX = 64 * kLutRows * PPV;
  constexpr int BLOCK_PX = kWaves * CHUNK_PX;
  static_assert(!LDS16 || (sizeof(CT) == 2 && sizeof(OT) == 1), "the LDS-staged 16-bit table has uint8 entries");
  static_assert(kThreads == 256, "one thread per entry of an 8-bit table");
  __shared__ __attribute__((aligned(16))) OT lut[LDS ? (1 << BITS) : 1];
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;  // the last image whose first block is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int i = __builtin_amdgcn_readfirstlane(lo);
  const OT* t = luts + size_t(i) * size_t(lut_stride);
  if constexpr (LDS16) {  // 64 KiB as 16 dwordx4 per thread
    const u32x4_t* src = reinterpret_cast<const u32x4_t*>(t);
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(lut);
#pragma unroll 4
    for (int e = threadIdx.x; e < (1 << BITS) / 16; e += kThreads) dst[e] = src[e];
    __syncthreads();
  } else if constexpr (LDS) {  // before any wave leaves: every thread stages one entry
    lut[threadIdx.x] = t[threadIdx.x];
    __syncthreads();
  }
  auto look = [&](uint32_t k) -> OT {
    if constexpr (LDS) return lut[k];
    else return t[k];
  };
  const int hw = tab.hw[i];
  const CT* codes = static_cast<const CT*>(tab.codes[i]);
  OT* out = static_cast<OT*>(tab.out[i]);
  const bool vec = (tab.vec >> i) & 1;
  const __amdgpu_buffer_rsrc_t rin =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<CT*>(codes), 0, hw * C * int(sizeof(CT)), kBufferRsrcFlags);
  const __amdgpu_buffer_rsrc_t rout =
      __builtin_amdgcn_make_buffer_rsrc(out, 0, hw * 3 * int(sizeof(OT)), kBufferRsrcFlags);
  const int lane = threadIdx.x & 63;
  for (int trip = 0; trip < trips; ++trip) {
    const int px0 = ((b - tab.first[i]) * trips + trip) * BLOCK_PX;
    if (px0 >= hw) break;  // block-uniform
    if (vec) {
      constexpr int NB = PPV * C * int(sizeof(CT));  // code bytes per lane-row
      const int wpx = px0 + (threadIdx.x >> 6) * CHUNK_PX;
      if (wpx >= hw) continue;  // wave-uniform (no barrier inside the loop)
      CT c[kLutRows][PPV * C];
#pragma unroll
      for (int r = 0; r < kLutRows; ++r)
        load_codes<CT, NB, IO::kLoadX>(rin, (wpx + r * 64 * PPV + lane * PPV) * C * int(sizeof(CT)), c[r]);
#pragma unroll
      for (int r = 0; r < kLutRows; ++r) {
        OT o[PPV * 3];
#pragma unroll
        for (int p = 0; p < PPV; ++p) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) o[p * 3 + ch] = look(c[r][p * C + (C == 1 ? 0 : ch)]);
        }
        u32x3_t w;
        __builtin_memcpy(&w, o, 12);
        __builtin_amdgcn_raw_buffer_store_b96(w, rout, (wpx + r * 64 * PPV + lane * PPV) * (12 / PPV), 0, IO::kStore);
      }
    } else {
#pragma unroll
      for (int k = 0; k < BLOCK_PX / kThreads; ++k) {
        const int p = px0 + k * kThreads + threadIdx.x;
        if (p < hw) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) out[size_t(p) * 3 + ch] = look(codes[size_t(p) * C + (C == 1 ? 0 : ch)]);
        }
      }
    }
  }
}

// 16-bit codes, uint8 entries: stage the table in LDS?  EXPO_CODES_LUT_LDS16 = 0 / 1 overrides the default.
bool codes_lut_lds16() {
  const char* v = getenv("EXPO_CODES_LUT_LDS16");
  if (v && *v) return atoi(v) != 0;
  return true;  // measured 0.95 against 0.19 of the copy rate at 16 x 24 MP, 0.58 against 0.18 at 16 x 512x512
                // (profiles/input_pictures.md)
}

// arguments validated by the caller
template <typename CT, int C, typename OT>
int codes_lut_t(const void* const* codes, const int* hs, const int* ws, int n, const void* luts, int lut_stride,
                void* const* outs, hipStream_t s) {
  constexpr int PPV = 12 / (3 * int(sizeof(OT)));
  constexpr int BLOCK_PX = kWaves * 64 * kLutRows * PPV;
  constexpr bool CAN_LDS16 = sizeof(CT) == 2 && sizeof(OT) == 1;
  long bytes = 0;  // cache policy from the bytes of the whole call
  for (int i = 0; i < n; ++i) bytes += long(hs[i]) * ws[i] * (C * long(sizeof(CT)) + 3L * long(sizeof(OT)));
  const bool stream = bytes >= stream_min_bytes();
  // the LDS-staged table is copied as dwordx4: every image's table must be 16-byte aligned
  const bool lds16 = CAN_LDS16 && codes_lut_lds16() && (reinterpret_cast<uintptr_t>(luts) & 15) == 0 &&
                     (lut_stride & 15) == 0;
  for (int base = 0; base < n; base += kLutMaxImages) {
    const int m = n - base < kLutMaxImages ? n - base : kLutMaxImages;
    long chunks = 0;
    for (int j = 0; j < m; ++j) chunks += (long(hs[base + j]) * ws[base + j] + BLOCK_PX - 1) / BLOCK_PX;
    int trips = 1;
    if (lds16) {
      const long t = chunks / kLutLdsBlocks;
      trips = t < 1 ? 1 : t > kLutLdsTrips ? kLutLdsTrips : int(t);
    }
    LutTable tab = {};
    tab.n = m;
    long blocks = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j, hw = hs[i] * ws[i];
      tab.codes[j] = codes[i];
      tab.out[j] = outs[i];
      tab.hw[j] = hw;
      tab.first[j] = int(blocks);
      blocks += (hw + BLOCK_PX * trips - 1) / (BLOCK_PX * trips);
      const uintptr_t a = reinterpret_cast<uintptr_t>(codes[i]) | reinterpret_cast<uintptr_t>(outs[i]);
      if ((a & 3) == 0 && hw % PPV == 0) tab.vec |= uint64_t(1) << j;
    }
    if (blocks > INT_MAX) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    tab.first[m] = int(blocks);
    const OT* lb = static_cast<const OT*>(luts) + size_t(base) * size_t(lut_stride);
    const dim3 grid(static_cast<unsigned>(blocks)), block(kThreads);
    if constexpr (CAN_LDS16) {
      if (lds16) {
        if (stream)
          hipLaunchKernelGGL((codes_lut_kernel<CT, C, OT, IoStream, true>), grid, block, 0, s, tab, lb, lut_stride, trips);
        else
          hipLaunchKernelGGL((codes_lut_kernel<CT, C, OT, IoCached, true>), grid, block, 0, s, tab, lb, lut_stride, trips);
        HIP_TRY(hipGetLastError(), "codes_lut launch");
        continue;
      }
    }
    if (stream)
      hipLaunchKernelGGL((codes_lut_kernel<CT, C, OT, IoStream, false>), grid, block, 0, s, tab, lb, lut_stride, trips);
    else
      hipLaunchKernelGGL((codes_lut_kernel<CT, C, OT, IoCached, false>), grid, block, 0, s, tab, lb, lut_stride, trips);
    HIP_TRY(hipGetLastError(), "codes_lut launch");
  }
  return EXPO_OK;
}

template <typename CT, typename OT, typename... A>
int codes_lut_channels(int channels, A... a) {
  if (channels == 1) return codes_lut_t<CT, 1, OT>(a...);
  if (channels == 3) return codes_lut_t<CT, 3, OT>(a...);
  return codes_lut_t<CT, 4, OT>(a...);
}

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

int expo_codes_lut_ragged(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                          const void* luts, int lut_stride, int out_bits, void* const* outs, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (channels != 1 && channels != 3 && channels != 4) return fail(EXPO_E_BADARG, "channels must be 1, 3 or 4");
  if (code_bits != 8 && code_bits != 16) return fail(EXPO_E_BADARG, "code_bits must be 8 or 16");
  if (out_bits != 8 && out_bits != 16) return fail(EXPO_E_BADARG, "out_bits must be 8 or 16");
  if (lut_stride != 0 && lut_stride < (1 << code_bits))
    return fail(EXPO_E_BADARG, "lut_stride must be 0 (one shared table) or at least 2^code_bits entries");
  if (n == 0) return EXPO_OK;
  if (!codes || !hs || !ws || !luts || !outs) return fail(EXPO_E_BADARG, "null pointer");
  if (out_bits == 16 && (reinterpret_cast<uintptr_t>(luts) & 1) != 0)
    return fail(EXPO_E_BADARG, "16-bit luts must be 2-byte aligned");
  for (int i = 0; i < n; ++i) {
    if (hs[i] < 1 || ws[i] < 1) return fail(EXPO_E_BADARG, "h >= 1, w >= 1 required");
    const long hw = long(hs[i]) * ws[i];
    if (hw * channels * (code_bits / 8) > (1L << 31) - 8192)
      return fail(EXPO_E_BADARG, "the codes of one image must be smaller than 2 GiB");
    if (hw * 3 * (out_bits / 8) > (1L << 31) - 8192)
      return fail(EXPO_E_BADARG, "one picture must be smaller than 2 GiB");
    if (!codes[i] || !outs[i]) return fail(EXPO_E_BADARG, "null image pointer");
    if (code_bits == 16 && (reinterpret_cast<uintptr_t>(codes[i]) & 1) != 0)
      return fail(EXPO_E_BADARG, "16-bit codes must be 2-byte aligned");
    if (out_bits == 16 && (reinterpret_cast<uintptr_t>(outs[i]) & 1) != 0)
      return fail(EXPO_E_BADARG, "16-bit pictures must be 2-byte aligned");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (code_bits == 8) {
    if (out_bits == 8) return codes_lut_channels<uint8_t, uint8_t>(channels, codes, hs, ws, n, luts, lut_stride, outs, s);
    return codes_lut_channels<uint8_t, uint16_t>(channels, codes, hs, ws, n, luts, lut_stride, outs, s);
  }
  if (out_bits == 8) return codes_lut_channels<uint16_t, uint8_t>(channels, codes, hs, ws, n, luts, lut_stride, outs, s);
  return codes_lut_channels<uint16_t, uint16_t>(channels, codes, hs, ws, n, luts, lut_stride, outs, s);
}

}  // extern "C"
