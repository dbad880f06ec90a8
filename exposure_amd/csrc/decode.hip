// decode.hip -- the input side of inference on the device: the integer codes of an image file (8- or 16-bit, 1, 3 or
// 4 channels, as the file holds them) to the linear NHWC storage tensor that evaluate.load_image + .to(dtype) gives.
// expo_decode_ragged / expo_decode_workspace_bytes; DESIGN.md §3.17.
//
// The caller supplies the float32 table of load_image's own expression over the code range, so the decode is a
// gather: out = cast(table[k]), or, normalised by the image's largest code m, cast(table[k] / (2 table[m])).
// With normalisation a call is three launches per 64 images (the ragged table of chain_fused.hip):
//   decode_max_kernel     one uint32 record per block: the largest code of its 16 KiB of codes (alpha masked off)
//   decode_finish_kernel  per image: the largest record m, then the image's normalised table in the storage dtype,
//                         T(table[k] / (2 table[m])) with the IEEE float32 division (this unit is compiled with the
//                         default, correctly rounded division: no fast-math, no -fno-honor-nans)
//   decode_kernel         gather only; 8-bit tables are staged in LDS, 16-bit ones are read through L2
// Without normalisation it is the decode launch alone, casting the caller's table on the fly.
// expo_decode_tables / expo_decode_tables_bytes stop after the tables: decode_max_kernel and
// decode_finish_kernel as above, the finish writing into the caller's buffer, or decode_cast_kernel for the one shared
// table T(table[k]) of a call without normalisation.  Their consumers gather at load time (proxy.hip,
// chain_fused_codes.hip).
// expo_codes_max_ragged stops after the maxima: decode_max_kernel, then codes_max_finish_kernel
// writing each image's largest code as an int32 -- the m_i above, also for calls that never normalise.
#include <limits.h>

#include "host_common.h"

namespace expo {

namespace {

constexpr int kDecodeMaxImages = 64;
constexpr int kDecodeRows = 4;  // 12-byte output vectors per lane in a wave's chunk (3 KiB of output per wave)
constexpr int kMaxRows = 4;     // 16-byte code vectors per thread of a max block
constexpr int kMaxBlockBytes = kThreads * 16 * kMaxRows;  // 16 KiB of codes per max record
constexpr int kFinishEntries = 4096;                      // table entries one finish block writes

// up to 64 images by value in the kernel arguments (1.6 KB): codes, output, pixel count, first block of each image
// (first[n] = the grid's size) and a bit per image for the vector path
struct DecodeTable {
  const void* codes[kDecodeMaxImages];
  void* out[kDecodeMaxImages];
  int hw[kDecodeMaxImages];
  int first[kDecodeMaxImages + 1];
  int n;
  uint64_t vec;
};

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// the last image whose first block is <= b (uniform: scalar search over the kernel arguments)
__device__ __forceinline__ int find_image(const DecodeTable& tab, int b) {
  int lo = 0, hi = tab.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

template <typename CT>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, kBufferRsrcFlags);
}

__device__ __forceinline__ uint32_t block_max(uint32_t m) {
  __shared__ uint32_t part[kWaves];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), o, 64)));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  return max(max(part[0], part[1]), max(part[2], part[3]));
}

// the largest code of a 16-byte vector that starts on a pixel (C == 4: the alpha samples masked off)
template <typename CT, int C>
__device__ __forceinline__ uint32_t max_codes(u32x4_t q, uint32_t m) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t w = q[k];
    if constexpr (sizeof(CT) == 1) {
      if constexpr (C == 4) w &= 0x00ffffffu;
      m = max(m, max(max(w & 0xffu, (w >> 8) & 0xffu), max((w >> 16) & 0xffu, w >> 24)));
    } else {
      if constexpr (C == 4) w &= (k & 1) ? 0xffffu : 0xffffffffu;
      m = max(m, max(w & 0xffffu, w >> 16));
    }
  }
  return m;
}

// one record per block: the largest code of the channels that reach the output in bytes [16 KiB lb, 16 KiB (lb + 1))
// of image i's codes.  Vector path (4-byte aligned codes): dwordx4 per lane, coalesced; the codes after the last
// whole 16-byte vector go element-wise in the image's last block.  Element-wise path otherwise.
template <typename CT, int C, class IO>
__global__ __launch_bounds__(kThreads) void decode_max_kernel(const DecodeTable tab, uint32_t* __restrict__ records) {
  const int b = blockIdx.x;
  const int i = find_image(tab, b);
  const int count = tab.hw[i] * C;
  const int lb = b - tab.first[i];
  const CT* codes = static_cast<const CT*>(tab.codes[i]);
  uint32_t m = 0;
  if ((tab.vec >> i) & 1) {
    const int bytes = count * int(sizeof(CT));
    const __amdgpu_buffer_rsrc_t rsrc = make_rsrc<CT>(codes, bytes);
    const int nvec = bytes / 16;
    u32x4_t q[kMaxRows];
#pragma unroll
    for (int r = 0; r < kMaxRows; ++r) {
      const int v = (lb * kMaxRows + r) * kThreads + threadIdx.x;
      q[r] = v < nvec ? __builtin_amdgcn_raw_buffer_load_b128(rsrc, v * 16, 0, IO::kLoadX) : u32x4_t{0, 0, 0, 0};
    }
#pragma unroll
    for (int r = 0; r < kMaxRows; ++r) m = max_codes<CT, C>(q[r], m);
    if (lb == tab.first[i + 1] - tab.first[i] - 1) {
      for (int e = nvec * 16 / int(sizeof(CT)) + threadIdx.x; e < count; e += kThreads)
        if (C != 4 || (e & 3) != 3) m = max(m, uint32_t(codes[e]));
    }
  } else {
    constexpr int per = kMaxBlockBytes / int(sizeof(CT));
    const int end = min(count, (lb + 1) * per);
    for (int e = lb * per + threadIdx.x; e < end; e += kThreads)
      if (C != 4 || (e & 3) != 3) m = max(m, uint32_t(codes[e]));
  }
  m = block_max(m);
  if (threadIdx.x == 0) records[b] = m;
}

// grid (slices, images): every block finds image j's largest code from its records (first[] of the max pass), then
// writes its slice of the normalised table T(table[k] / (2 table[m])); all-zero codes give 0 / 0 = NaN, as numpy
// NAN_TABLE (expo_decode_tables): a table whose divisor is 0 is NaN in EVERY entry, not only in those the image's codes
// read (entry k > 0 of an all-zero image would be table[k] / 0 = inf; no code of the image reads it, so a gather gives
// the same either way).  The instantiation of expo_decode_ragged is the kernel as it was.
template <typename T, int BITS, bool NAN_TABLE = false>
__global__ __launch_bounds__(kThreads) void decode_finish_kernel(const DecodeTable tab, const uint32_t* __restrict__ records,
                                                                 const float* __restrict__ table, T* __restrict__ tables) {
  constexpr int entries = 1 << BITS;
  const int j = blockIdx.y;
  uint32_t m = 0;
  for (int r = tab.first[j] + threadIdx.x; r < tab.first[j + 1]; r += kThreads) m = max(m, records[r]);
  m = block_max(m);
  float d = 2.0f * table[m];
  if constexpr (NAN_TABLE) d = d == 0.0f ? __builtin_nanf("") : d;
  T* tj = tables + size_t(j) * entries;
  const int e0 = blockIdx.x * kFinishEntries;
  const int e1 = min(entries, e0 + kFinishEntries);
  for (int e = e0 + threadIdx.x; e < e1; e += kThreads) tj[e] = T(table[e] / d);
}

// expo_codes_max_ragged's finish, one block per image: image j's largest record, as an int32
__global__ __launch_bounds__(kThreads) void codes_max_finish_kernel(const DecodeTable tab, const uint32_t* __restrict__ records,
                                                                    int32_t* __restrict__ maxima) {
  const int j = blockIdx.x;
  uint32_t m = 0;
  for (int r = tab.first[j] + threadIdx.x; r < tab.first[j + 1]; r += kThreads) m = max(m, records[r]);
  m = block_max(m);
  if (threadIdx.x == 0) maxima[j] = int32_t(m);
}

// the shared table of a call without normalisation, in the storage dtype
template <typename T>
__global__ __launch_bounds__(kThreads) void decode_cast_kernel(const float* __restrict__ table, T* __restrict__ tables,
                                                               int entries) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e < entries) tables[e] = T(table[e]);
}

// The gather.  Vector path (codes and output 4-byte aligned, whole 12-byte output vectors): a lane-row is the
// 12-byte output vector of PPV pixels (fp16 2, fp32 1) at the chain's coalesced positions (pixel_io.h), stored as
// one dwordx3; its PPV * C codes are loaded with the widest access their size allows.  Rows past the end of the image
// read 0 and their stores are dropped by the buffer's bounds check.  Element-wise path otherwise.
// NORM: tables = the normalised T tables of this launch's images, [n][2^BITS]; else the caller's float table.
template <typename CT, int C, typename T, bool NORM, class IO>
__global__ __launch_bounds__(kThreads) void decode_kernel(const DecodeTable tab, const void* __restrict__ tables) {
  constexpr int BITS = 8 * int(sizeof(CT));
  constexpr bool LDS = BITS == 8;
  constexpr int PPV = VecTraits<T>::PPV;
  constexpr int CHUNK_PX = 64 * kDecodeRows * PPV;
  constexpr int BLOCK_PX = kWaves * CHUNK_PX;
  static_assert(!LDS || kThreads == 256, "one thread per entry of an 8-bit table");
  __shared__ T lut[LDS ? 256 : 1];
  const int b = blockIdx.x;
  const int i = find_image(tab, b);
  const int hw = tab.hw[i];
  const int px0 = (b - tab.first[i]) * BLOCK_PX;
  const T* ttab = static_cast<const T*>(tables) + (size_t(i) << BITS);
  const float* ftab = static_cast<const float*>(tables);
  if constexpr (LDS) {
    lut[threadIdx.x] = NORM ? ttab[threadIdx.x] : T(ftab[threadIdx.x]);
    __syncthreads();
  }
  auto look = [&](uint32_t k) -> T {
    if constexpr (LDS) return lut[k];
    else if constexpr (NORM) return ttab[k];
    else return T(ftab[k]);
  };
  const CT* codes = static_cast<const CT*>(tab.codes[i]);
  T* out = static_cast<T*>(tab.out[i]);
  if ((tab.vec >> i) & 1) {
    constexpr int NB = PPV * C * int(sizeof(CT));  // code bytes per lane-row
    const int lane = threadIdx.x & 63;
    const int wpx = px0 + (threadIdx.x >> 6) * CHUNK_PX;
    if (wpx >= hw) return;  // wave-uniform
    const __amdgpu_buffer_rsrc_t rin = make_rsrc<CT>(codes, hw * C * int(sizeof(CT)));
    const __amdgpu_buffer_rsrc_t rout = make_rsrc<T>(out, hw * 3 * int(sizeof(T)));
    CT c[kDecodeRows][PPV * C];
#pragma unroll
    for (int r = 0; r < kDecodeRows; ++r) {
      const int off = (wpx + r * 64 * PPV + lane * PPV) * C * int(sizeof(CT));
      if constexpr (NB == 16) {
        const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rin, off, 0, IO::kLoadX);
        __builtin_memcpy(c[r], &q, NB);
      } else if constexpr (NB == 12) {
        const u32x3_t q = __builtin_amdgcn_raw_buffer_load_b96(rin, off, 0, IO::kLoadX);
        __builtin_memcpy(c[r], &q, NB);
      } else if constexpr (NB == 8) {
        const u32x2_t q = __builtin_amdgcn_raw_buffer_load_b64(rin, off, 0, IO::kLoadX);
        __builtin_memcpy(c[r], &q, NB);
      } else if constexpr (NB == 4) {
        const uint32_t q = __builtin_amdgcn_raw_buffer_load_b32(rin, off, 0, IO::kLoadX);
        __builtin_memcpy(c[r], &q, NB);
      } else if constexpr (NB % 2 == 0) {  // 2 or 6 bytes: 2-byte aligned
        uint16_t q[NB / 2];
#pragma unroll
        for (int k = 0; k < NB / 2; ++k) q[k] = __builtin_amdgcn_raw_buffer_load_b16(rin, off + 2 * k, 0, IO::kLoadX);
        __builtin_memcpy(c[r], q, NB);
      } else {  // 1 or 3 bytes
        uint8_t q[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) q[k] = __builtin_amdgcn_raw_buffer_load_b8(rin, off + k, 0, IO::kLoadX);
        __builtin_memcpy(c[r], q, NB);
      }
    }
#pragma unroll
    for (int r = 0; r < kDecodeRows; ++r) {
      T o[PPV * 3];
#pragma unroll
      for (int p = 0; p < PPV; ++p) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[p * 3 + ch] = look(c[r][p * C + (C == 1 ? 0 : ch)]);
      }
      u32x3_t w;
      __builtin_memcpy(&w, o, 12);
      __builtin_amdgcn_raw_buffer_store_b96(w, rout, (wpx + r * 64 * PPV + lane * PPV) * (12 / PPV), 0,
                                           IO::kStore);
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

template <typename T> constexpr int decode_block_px() { return kWaves * 64 * kDecodeRows * VecTraits<T>::PPV; }

inline long max_blocks(long code_bytes) { return (code_bytes + kMaxBlockBytes - 1) / kMaxBlockBytes; }
inline size_t round_up256(size_t x) { return (x + 255) & ~size_t(255); }

// workspace of the normalising calls: per launch of up to 64 images, one uint32 record per max block, then one table
// per image (sized for float32 entries, whatever the storage dtype); launches reuse it in stream order.  -1 when a
// launch has more than INT_MAX max blocks.
long workspace_need(int n, const int* hs, const int* ws, int channels, int code_bits) {
  long need = 0;
  for (int base = 0; base < n; base += kDecodeMaxImages) {
    const int m = n - base < kDecodeMaxImages ? n - base : kDecodeMaxImages;
    long blocks = 0;
    for (int j = 0; j < m; ++j) blocks += max_blocks(long(hs[base + j]) * ws[base + j] * channels * (code_bits / 8));
    if (blocks > INT_MAX) return -1;
    const long bytes = long(round_up256(size_t(blocks) * 4)) + long(m) * (4L << code_bits);
    need = bytes > need ? bytes : need;
  }
  return need;
}

// arguments validated by the caller
template <typename CT, int C, typename T>
int decode_ragged_t(const void* const* codes, const int* hs, const int* ws, int n, const float* table, int normalize,
                    void* const* outs, void* workspace, hipStream_t s) {
  constexpr int BITS = 8 * int(sizeof(CT));
  constexpr int PPV = VecTraits<T>::PPV;
  long bytes = 0;  // cache policy from the bytes of the whole call
  for (int i = 0; i < n; ++i) bytes += long(hs[i]) * ws[i] * (C * long(sizeof(CT)) + 3L * long(sizeof(T)));
  const bool stream = bytes >= stream_min_bytes();
  for (int base = 0; base < n; base += kDecodeMaxImages) {
    const int m = n - base < kDecodeMaxImages ? n - base : kDecodeMaxImages;
    DecodeTable dt = {}, mt = {};
    dt.n = mt.n = m;
    long dblocks = 0, mblocks = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j, hw = hs[i] * ws[i];
      dt.codes[j] = mt.codes[j] = codes[i];
      dt.out[j] = outs[i];
      dt.hw[j] = mt.hw[j] = hw;
      dt.first[j] = int(dblocks);
      mt.first[j] = int(mblocks);
      dblocks += (hw + decode_block_px<T>() - 1) / decode_block_px<T>();
      mblocks += max_blocks(long(hw) * C * long(sizeof(CT)));
      const bool in4 = (reinterpret_cast<uintptr_t>(codes[i]) & 3) == 0;
      if (in4) mt.vec |= uint64_t(1) << j;
      if (in4 && (reinterpret_cast<uintptr_t>(outs[i]) & 3) == 0 && hw % PPV == 0) dt.vec |= uint64_t(1) << j;
    }
    if (dblocks > INT_MAX || mblocks > INT_MAX) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    dt.first[m] = int(dblocks);
    mt.first[m] = int(mblocks);
    const dim3 block(kThreads);
    const void* tabs = table;
    if (normalize) {
      uint32_t* rec = static_cast<uint32_t*>(workspace);
      T* ttab = reinterpret_cast<T*>(static_cast<char*>(workspace) + round_up256(size_t(mblocks) * 4));
      if (stream)
        hipLaunchKernelGGL((decode_max_kernel<CT, C, IoStream>), dim3(unsigned(mblocks)), block, 0, s, mt, rec);
      else
        hipLaunchKernelGGL((decode_max_kernel<CT, C, IoCached>), dim3(unsigned(mblocks)), block, 0, s, mt, rec);
      HIP_TRY(hipGetLastError(), "decode_max launch");
      const int slices = (1 << BITS) > kFinishEntries ? (1 << BITS) / kFinishEntries : 1;
      hipLaunchKernelGGL((decode_finish_kernel<T, BITS>), dim3(slices, m), block, 0, s, mt, rec, table, ttab);
      HIP_TRY(hipGetLastError(), "decode_finish launch");
      tabs = ttab;
    }
    const dim3 grid(static_cast<unsigned>(dblocks));
    if (normalize && stream)
      hipLaunchKernelGGL((decode_kernel<CT, C, T, true, IoStream>), grid, block, 0, s, dt, tabs);
    else if (normalize)
      hipLaunchKernelGGL((decode_kernel<CT, C, T, true, IoCached>), grid, block, 0, s, dt, tabs);
    else if (stream)
      hipLaunchKernelGGL((decode_kernel<CT, C, T, false, IoStream>), grid, block, 0, s, dt, tabs);
    else
      hipLaunchKernelGGL((decode_kernel<CT, C, T, false, IoCached>), grid, block, 0, s, dt, tabs);
    HIP_TRY(hipGetLastError(), "decode launch");
  }
  return EXPO_OK;
}

// arguments validated by the caller; normalize: image i's table at tables + i * 2^BITS, the records of a launch in the
// workspace (launches reuse it in stream order)
template <typename CT, int C, typename T>
int decode_tables_t(const void* const* codes, const int* hs, const int* ws, int n, const float* table, void* tables,
                    void* workspace, hipStream_t s) {
  constexpr int BITS = 8 * int(sizeof(CT));
  long bytes = 0;
  for (int i = 0; i < n; ++i) bytes += long(hs[i]) * ws[i] * C * long(sizeof(CT));
  const bool stream = bytes >= stream_min_bytes();
  for (int base = 0; base < n; base += kDecodeMaxImages) {
    const int m = n - base < kDecodeMaxImages ? n - base : kDecodeMaxImages;
    DecodeTable mt = {};
    mt.n = m;
    long mblocks = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j, hw = hs[i] * ws[i];
      mt.codes[j] = codes[i];
      mt.hw[j] = hw;
      mt.first[j] = int(mblocks);
      mblocks += max_blocks(long(hw) * C * long(sizeof(CT)));
      if ((reinterpret_cast<uintptr_t>(codes[i]) & 3) == 0) mt.vec |= uint64_t(1) << j;
    }
    if (mblocks > INT_MAX) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    mt.first[m] = int(mblocks);
    const dim3 block(kThreads);
    uint32_t* rec = static_cast<uint32_t*>(workspace);
    T* ttab = static_cast<T*>(tables) + (size_t(base) << BITS);
    if (stream)
      hipLaunchKernelGGL((decode_max_kernel<CT, C, IoStream>), dim3(unsigned(mblocks)), block, 0, s, mt, rec);
    else
      hipLaunchKernelGGL((decode_max_kernel<CT, C, IoCached>), dim3(unsigned(mblocks)), block, 0, s, mt, rec);
    HIP_TRY(hipGetLastError(), "decode_max launch");
    const int slices = (1 << BITS) > kFinishEntries ? (1 << BITS) / kFinishEntries : 1;
    hipLaunchKernelGGL((decode_finish_kernel<T, BITS, true>), dim3(slices, m), block, 0, s, mt, rec, table, ttab);
    HIP_TRY(hipGetLastError(), "decode_finish launch");
  }
  return EXPO_OK;
}

// arguments validated by the caller: decode_max_kernel's records of a launch in the workspace (launches reuse it in
// stream order), then the finish into maxima
template <typename CT, int C>
int codes_max_t(const void* const* codes, const int* hs, const int* ws, int n, int32_t* maxima, void* workspace,
                hipStream_t s) {
  long bytes = 0;
  for (int i = 0; i < n; ++i) bytes += long(hs[i]) * ws[i] * C * long(sizeof(CT));
  const bool stream = bytes >= stream_min_bytes();
  for (int base = 0; base < n; base += kDecodeMaxImages) {
    const int m = n - base < kDecodeMaxImages ? n - base : kDecodeMaxImages;
    DecodeTable mt = {};
    mt.n = m;
    long mblocks = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j, hw = hs[i] * ws[i];
      mt.codes[j] = codes[i];
      mt.hw[j] = hw;
      mt.first[j] = int(mblocks);
      mblocks += max_blocks(long(hw) * C * long(sizeof(CT)));
      if ((reinterpret_cast<uintptr_t>(codes[i]) & 3) == 0) mt.vec |= uint64_t(1) << j;
    }
    if (mblocks > INT_MAX) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    mt.first[m] = int(mblocks);
    const dim3 block(kThreads);
    uint32_t* rec = static_cast<uint32_t*>(workspace);
    if (stream)
      hipLaunchKernelGGL((decode_max_kernel<CT, C, IoStream>), dim3(unsigned(mblocks)), block, 0, s, mt, rec);
    else
      hipLaunchKernelGGL((decode_max_kernel<CT, C, IoCached>), dim3(unsigned(mblocks)), block, 0, s, mt, rec);
    HIP_TRY(hipGetLastError(), "decode_max launch");
    hipLaunchKernelGGL(codes_max_finish_kernel, dim3(unsigned(m)), block, 0, s, mt, rec, maxima + base);
    HIP_TRY(hipGetLastError(), "codes_max_finish launch");
  }
  return EXPO_OK;
}

template <typename CT>
int codes_max_channels(int channels, const void* const* codes, const int* hs, const int* ws, int n, int32_t* maxima,
                       void* workspace, hipStream_t s) {
  if (channels == 1) return codes_max_t<CT, 1>(codes, hs, ws, n, maxima, workspace, s);
  if (channels == 3) return codes_max_t<CT, 3>(codes, hs, ws, n, maxima, workspace, s);
  return codes_max_t<CT, 4>(codes, hs, ws, n, maxima, workspace, s);
}

template <typename CT, typename T>
int decode_tables_channels(int channels, const void* const* codes, const int* hs, const int* ws, int n,
                           const float* table, void* tables, void* workspace, hipStream_t s) {
  if (channels == 1) return decode_tables_t<CT, 1, T>(codes, hs, ws, n, table, tables, workspace, s);
  if (channels == 3) return decode_tables_t<CT, 3, T>(codes, hs, ws, n, table, tables, workspace, s);
  return decode_tables_t<CT, 4, T>(codes, hs, ws, n, table, tables, workspace, s);
}

template <typename T>
int decode_cast_t(const float* table, void* tables, int entries, hipStream_t s) {
  hipLaunchKernelGGL((decode_cast_kernel<T>), dim3(unsigned((entries + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     table, static_cast<T*>(tables), entries);
  HIP_TRY(hipGetLastError(), "decode_cast launch");
  return EXPO_OK;
}

template <typename CT, typename T>
int decode_channels(int channels, const void* const* codes, const int* hs, const int* ws, int n, const float* table,
                    int normalize, void* const* outs, void* workspace, hipStream_t s) {
  if (channels == 1) return decode_ragged_t<CT, 1, T>(codes, hs, ws, n, table, normalize, outs, workspace, s);
  if (channels == 3) return decode_ragged_t<CT, 3, T>(codes, hs, ws, n, table, normalize, outs, workspace, s);
  return decode_ragged_t<CT, 4, T>(codes, hs, ws, n, table, normalize, outs, workspace, s);
}

// kernel arguments of the decode kernels: the table and one pointer
static_assert(sizeof(DecodeTable) + 8 <= 4096, "the decode table must fit the 4 KB kernarg block");

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

size_t expo_decode_workspace_bytes(int n, const int* hs, const int* ws, int channels, int code_bits) {
  if (n < 1 || !hs || !ws || (channels != 1 && channels != 3 && channels != 4) || (code_bits != 8 && code_bits != 16))
    return 0;
  for (int i = 0; i < n; ++i)
    if (hs[i] < 1 || ws[i] < 1) return 0;
  const long need = workspace_need(n, hs, ws, channels, code_bits);
  return need < 0 ? 0 : size_t(need);
}

int expo_decode_ragged(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                       const float* table, int normalize, void* const* outs, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (channels != 1 && channels != 3 && channels != 4) return fail(EXPO_E_BADARG, "channels must be 1, 3 or 4");
  if (code_bits != 8 && code_bits != 16) return fail(EXPO_E_BADARG, "code_bits must be 8 or 16");
  if (normalize != 0 && normalize != 1) return fail(EXPO_E_BADARG, "normalize must be 0 or 1");
  if (dtype != EXPO_F16 && dtype != EXPO_F32) return fail(EXPO_E_BADDTYPE, "dtype must be EXPO_F16 or EXPO_F32");
  if (n == 0) return EXPO_OK;
  if (!codes || !hs || !ws || !table || !outs) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (int rc = check_common(1, hs[i], ws[i], dtype)) return rc;
    if (long(hs[i]) * ws[i] * channels * (code_bits / 8) > (1L << 31) - 8192)
      return fail(EXPO_E_BADARG, "the codes of one image must be smaller than 2 GiB");
    if (!codes[i] || !outs[i]) return fail(EXPO_E_BADARG, "null image pointer");
  }
  if (normalize) {
    const long need = workspace_need(n, hs, ws, channels, code_bits);
    if (need < 0) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3) != 0)
      return fail(EXPO_E_BADARG, "normalize needs a 4-byte aligned workspace");
    if (workspace_bytes < size_t(need))
      return fail(EXPO_E_BADARG, "workspace too small (expo_decode_workspace_bytes)");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (code_bits == 8)
    return dtype == EXPO_F16 ? decode_channels<uint8_t, half_t>(channels, codes, hs, ws, n, table, normalize, outs, workspace, s)
                             : decode_channels<uint8_t, float>(channels, codes, hs, ws, n, table, normalize, outs, workspace, s);
  return dtype == EXPO_F16 ? decode_channels<uint16_t, half_t>(channels, codes, hs, ws, n, table, normalize, outs, workspace, s)
                           : decode_channels<uint16_t, float>(channels, codes, hs, ws, n, table, normalize, outs, workspace, s);
}

size_t expo_decode_tables_bytes(int n, int code_bits, int normalize, int dtype) {
  if (n < 1 || (code_bits != 8 && code_bits != 16) || (normalize != 0 && normalize != 1) ||
      (dtype != EXPO_F16 && dtype != EXPO_F32))
    return 0;
  return (size_t(normalize ? n : 1) << code_bits) * (dtype == EXPO_F16 ? 2 : 4);
}

int expo_decode_tables(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                       const float* table, int normalize, void* tables, size_t tables_bytes, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (channels != 1 && channels != 3 && channels != 4) return fail(EXPO_E_BADARG, "channels must be 1, 3 or 4");
  if (code_bits != 8 && code_bits != 16) return fail(EXPO_E_BADARG, "code_bits must be 8 or 16");
  if (normalize != 0 && normalize != 1) return fail(EXPO_E_BADARG, "normalize must be 0 or 1");
  if (dtype != EXPO_F16 && dtype != EXPO_F32) return fail(EXPO_E_BADDTYPE, "dtype must be EXPO_F16 or EXPO_F32");
  if (n == 0) return 0;
  if (!table || !tables || (normalize && (!codes || !hs || !ws))) return fail(EXPO_E_BADARG, "null pointer");
  if ((reinterpret_cast<uintptr_t>(tables) & 3) != 0) return fail(EXPO_E_BADARG, "tables must be 4-byte aligned");
  if (tables_bytes < expo_decode_tables_bytes(n, code_bits, normalize, dtype))
    return fail(EXPO_E_BADARG, "tables buffer too small (expo_decode_tables_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!normalize) {
    const int rc = dtype == EXPO_F16 ? decode_cast_t<half_t>(table, tables, 1 << code_bits, s)
                                     : decode_cast_t<float>(table, tables, 1 << code_bits, s);
    return rc;  // EXPO_OK = 0: one shared table
  }
  for (int i = 0; i < n; ++i) {
    if (int rc = check_common(1, hs[i], ws[i], dtype)) return rc;
    if (long(hs[i]) * ws[i] * channels * (code_bits / 8) > (1L << 31) - 8192)
      return fail(EXPO_E_BADARG, "the codes of one image must be smaller than 2 GiB");
    if (!codes[i]) return fail(EXPO_E_BADARG, "null image pointer");
  }
  const long need = workspace_need(n, hs, ws, channels, code_bits);
  if (need < 0) return fail(EXPO_E_BADARG, "too many blocks in one launch");
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3) != 0)
    return fail(EXPO_E_BADARG, "normalize needs a 4-byte aligned workspace");
  if (workspace_bytes < size_t(need)) return fail(EXPO_E_BADARG, "workspace too small (expo_decode_workspace_bytes)");
  int rc;
  if (code_bits == 8)
    rc = dtype == EXPO_F16 ? decode_tables_channels<uint8_t, half_t>(channels, codes, hs, ws, n, table, tables, workspace, s)
                           : decode_tables_channels<uint8_t, float>(channels, codes, hs, ws, n, table, tables, workspace, s);
  else
    rc = dtype == EXPO_F16 ? decode_tables_channels<uint16_t, half_t>(channels, codes, hs, ws, n, table, tables, workspace, s)
                           : decode_tables_channels<uint16_t, float>(channels, codes, hs, ws, n, table, tables, workspace, s);
  return rc != EXPO_OK ? rc : 1 << code_bits;
}

int expo_codes_max_ragged(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                          int32_t* maxima, void* workspace, size_t workspace_bytes, void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (channels != 1 && channels != 3 && channels != 4) return fail(EXPO_E_BADARG, "channels must be 1, 3 or 4");
  if (code_bits != 8 && code_bits != 16) return fail(EXPO_E_BADARG, "code_bits must be 8 or 16");
  if (n == 0) return EXPO_OK;
  if (!codes || !hs || !ws || !maxima) return fail(EXPO_E_BADARG, "null pointer");
  if ((reinterpret_cast<uintptr_t>(maxima) & 3) != 0) return fail(EXPO_E_BADARG, "maxima must be 4-byte aligned");
  for (int i = 0; i < n; ++i) {
    if (int rc = check_common(1, hs[i], ws[i], EXPO_F16)) return rc;
    if (long(hs[i]) * ws[i] * channels * (code_bits / 8) > (1L << 31) - 8192)
      return fail(EXPO_E_BADARG, "the codes of one image must be smaller than 2 GiB");
    if (!codes[i]) return fail(EXPO_E_BADARG, "null image pointer");
  }
  const long need = workspace_need(n, hs, ws, channels, code_bits);
  if (need < 0) return fail(EXPO_E_BADARG, "too many blocks in one launch");
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3) != 0)
    return fail(EXPO_E_BADARG, "a 4-byte aligned workspace is needed");
  if (workspace_bytes < size_t(need)) return fail(EXPO_E_BADARG, "workspace too small (expo_decode_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (code_bits == 8) return codes_max_channels<uint8_t>(channels, codes, hs, ws, n, maxima, workspace, s);
  return codes_max_channels<uint16_t>(channels, codes, hs, ws, n, maxima, workspace, s);
}

}  // extern "C"
