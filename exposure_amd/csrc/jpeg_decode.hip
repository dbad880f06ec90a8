// jpeg_decode.hip -- baseline JPEG files decoded on the device (expo_jpeg_decode_ragged) into the
// (H, W, 3) uint8 codes that PIL's open + convert('RGB') gives, bit for bit: T.81 §F.2.2 entropy decoding, libjpeg's
// "islow" inverse transform, its triangle-filter chroma upsampling and its colour conversion.  Default flags
// (csrc/build.sh).  Integer code only: no float, nothing zero-filled by the caller.  Per call one memset node for the
// status words, then three launches per group of up to 64 pictures, in stream order:
//   jpeg_entropy_kernel  a lane per segment (a restart interval; a file without DRI is one segment).  The segments come
//                        from one list over the group, so the lanes of a wave may belong to different pictures: the
//                        Huffman tables are read from the picture's plan through the cache, not staged in LDS.  A lane
//                        walks its MCUs and stages each block in its own 128-byte LDS slot (zeroed, then scattered into
//                        through the zigzag), which leaves as eight 16-byte stores.  Every read is clamped to the file,
//                        every write goes to the lane's own blocks, every loop is bounded by the geometry.
//   jpeg_idct_kernel     32 blocks per workgroup, eight threads per block: dequantise a row each into LDS, a column
//                        each, a row each, clamp, and store the real samples into the component's plane
//   jpeg_rgb_kernel      a thread per chroma sample: its 1, 2 x 1 or 2 x 2 output pixels, upsampled, converted and
//                        stored as bytes (any alignment of the output)
// The serial routines are jpeg_decode.h's, which tools/jpeg_decode_rehearse.cpp runs on the host.
#include <limits.h>

#include "host_common.h"
#include "jpeg_decode.h"

namespace expo {

namespace {

using namespace jpegdec;

constexpr int kDecMaxImages = 64;
constexpr int kEntropyThreads = 64;     // one wave: 64 segments
constexpr int kSlotVecs = 9;            // a lane's LDS slot: 128 bytes and 16 of padding, in 16-byte vectors
constexpr int kIdctBlocks = 32;         // blocks per workgroup of kThreads = 8 x 32 threads
constexpr int kIdctStride = 72;         // a block's int32 in LDS: eight rows of 9
static_assert(kThreads == 8 * kIdctBlocks, "eight threads per block");

// up to 64 pictures by value in the kernel arguments (3.4 KB)
struct DecTable {
  const uint8_t* file[kDecMaxImages];
  const uint8_t* plan[kDecMaxImages];
  uint8_t* out[kDecMaxImages];
  int64_t base[kDecMaxImages];       // the picture's part of the workspace (jpegdec::layout)
  int file_bytes[kDecMaxImages];
  uint32_t hw[kDecMaxImages];        // h << 16 | w
  uint8_t mode[kDecMaxImages];       // sampling | ncomp << 2
  int first_seg[kDecMaxImages + 1];  // first segment, first workgroup of the idct and of the rgb launch
  int first_idct[kDecMaxImages + 1];
  int first_rgb[kDecMaxImages + 1];
  int n;
};
static_assert(sizeof(DecTable) + 32 <= 4096, "the table must fit the 4 KB kernarg block");

// the last image whose first entry is <= b (b uniform over the wave)
__device__ __forceinline__ int find_image(const int* first, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

__device__ __forceinline__ Geometry table_geometry(const DecTable& tab, int j) {
  const uint32_t hw = tab.hw[j];
  const int mode = tab.mode[j];
  return geometry(int(hw >> 16), int(hw & 0xFFFFu), mode & 3, mode >> 2);
}

__global__ __launch_bounds__(kEntropyThreads) void jpeg_entropy_kernel(const DecTable tab, uint8_t* __restrict__ ws,
                                                                       int32_t* __restrict__ status) {
  __shared__ uint4 slots[kEntropyThreads * kSlotVecs];
  const int lane = int(threadIdx.x);
  const int total = tab.first_seg[tab.n];
  const int seg0 = int(blockIdx.x) * kEntropyThreads;
  const int seg = seg0 + lane;
  // the pictures of this wave's segments: uniform bounds, a lane keeps the last one that starts at or before its segment
  const int jlo = find_image(tab.first_seg, tab.n, seg0);
  const int jhi = find_image(tab.first_seg, tab.n, seg0 + kEntropyThreads - 1 < total - 1 ? seg0 + kEntropyThreads - 1 : total - 1);
  const uint8_t* file = nullptr;
  const uint8_t* planp = nullptr;
  int64_t base = 0;
  int file_bytes = 0, first = 0, pic = 0, mode = 4;
  uint32_t hw = (1u << 16) | 1u;
  for (int j = jlo; j <= jhi; ++j) {
    const int f = tab.first_seg[j];
    if (seg >= f) {
      file = tab.file[j], planp = tab.plan[j], base = tab.base[j], file_bytes = tab.file_bytes[j];
      first = f, pic = j, mode = tab.mode[j], hw = tab.hw[j];
    }
  }
  if (seg >= total) return;
  const Geometry g = geometry(int(hw >> 16), int(hw & 0xFFFFu), mode & 3, mode >> 2);
  const int k = seg - first;  // 0 <= k < nsegs: the host checked nsegs against the geometry
  const int st = decode_segment(file, file_bytes, planp, g, k, &slots[lane * kSlotVecs], reinterpret_cast<uint4*>(ws + base),
                                make_uint4(0u, 0u, 0u, 0u));
  if (st) atomicOr(&status[pic], st);
}

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const DecTable tab, uint8_t* __restrict__ ws) {
  __shared__ int32_t lds[kIdctBlocks * kIdctStride];
  const int j = find_image(tab.first_idct, tab.n, int(blockIdx.x));
  const Geometry g = table_geometry(tab, j);
  const Layout lay = layout(tab.base[j], g);
  const PlanHead* plan = reinterpret_cast<const PlanHead*>(tab.plan[j]);
  const int t = int(threadIdx.x), lb = t >> 3, r = t & 7;
  const int64_t b = int64_t(int(blockIdx.x) - tab.first_idct[j]) * kIdctBlocks + lb;
  const bool live = b < blocks(g);
  int32_t* mine = &lds[lb * kIdctStride];
  int comp = 0, brow = 0, bcol = 0;
  if (live) {
    const int64_t m = b / g.bpm;
    const int jj = int(b - m * g.bpm);
    comp = block_component(g, jj);
    block_place(g, m, jj, &brow, &bcol);
    // row r of the block, dequantised
    const uint4 raw = *reinterpret_cast<const uint4*>(ws + lay.coef + b * 128 + r * 16);
    const uint2 q = *reinterpret_cast<const uint2*>(&plan->q[plan->tq[comp] & 3][r * 8]);
    const uint32_t cw[4] = {raw.x, raw.y, raw.z, raw.w};
    const uint32_t qw[2] = {q.x, q.y};
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const int32_t coef = int16_t(cw[x >> 1] >> (16 * (x & 1)));
      mine[r * 9 + x] = coef * int32_t((qw[x >> 2] >> (8 * (x & 3))) & 255u);
    }
  }
  __syncthreads();
  if (live) {  // column r
    int32_t in[8], o[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) in[v] = mine[v * 9 + r];
    idct_pass(in, 11, o);
#pragma unroll
    for (int v = 0; v < 8; ++v) mine[v * 9 + r] = o[v];
  }
  __syncthreads();
  if (live) {  // row r
    int32_t in[8], o[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) in[x] = mine[r * 9 + x];
    idct_pass(in, 18, o);
    const int y = brow * 8 + r, x0 = bcol * 8, pw = plane_w(g, comp);
    if (y < plane_h(g, comp) && x0 < pw) {  // only real samples are stored
      // (selects, not lay.plane[comp]: a dynamic index would move the struct into LDS)
      const int64_t plane = comp == 0 ? lay.plane[0] : comp == 1 ? lay.plane[1] : lay.plane[2];
      uint8_t* dst = ws + plane + int64_t(y) * plane_stride(g, comp) + x0;
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        lo |= uint32_t(clamp255(o[x] + 128)) << (8 * x);
        hi |= uint32_t(clamp255(o[x + 4] + 128)) << (8 * x);
      }
      if (x0 + 8 <= pw) {
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
      } else {
        for (int x = 0; x < pw - x0; ++x) dst[x] = uint8_t((x < 4 ? lo >> (8 * x) : hi >> (8 * (x - 4))) & 255u);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_rgb_kernel(const DecTable tab, const uint8_t* __restrict__ ws) {
  const int j = find_image(tab.first_rgb, tab.n, int(blockIdx.x));
  const Geometry g = table_geometry(tab, j);
  const Layout lay = layout(tab.base[j], g);
  const int dh = plane_h(g, g.ncomp - 1), dw = plane_w(g, g.ncomp - 1);  // the chroma plane's (grey: the picture's) samples
  const int64_t u = int64_t(int(blockIdx.x) - tab.first_rgb[j]) * kThreads + int(threadIdx.x);
  if (u >= int64_t(dh) * dw) return;
  rgb_unit(g, lay, ws, tab.out[j], int(u / dw), int(u % dw));
}

}  // namespace

}  // namespace expo

using namespace expo;

namespace {

// bytes of workspace of images [base, base + m): the pictures' parts behind one another
int64_t group_workspace(const int* hs, const int* ws, const int* samplings, const int* ncomps, int base, int m, int64_t* bases) {
  int64_t at = 0;
  for (int j = 0; j < m; ++j) {
    if (bases) bases[j] = at;
    at = jpegdec::layout(at, jpegdec::geometry(hs[base + j], ws[base + j], samplings[base + j], ncomps[base + j])).end;
  }
  return at;
}

}  // namespace

// Not exported: the inverse transform and the colour kernel for pictures [base, base + m) (m <= 64) whose parts of the
// workspace start at bases[0..m), for csrc/jpeg_decode_sync.hip, which fills the coefficients in its own way.  With
// enqueue false it only checks the grids.
namespace expo {
int jpeg_decode_reconstruct(const void* const* plans, const int* hs, const int* ws, const int* samplings, const int* ncomps,
                            int base, int m, const int64_t* bases, void* const* outs, void* workspace, void* stream, bool enqueue) {
  DecTable tab = {};
  tab.n = m;
  int64_t idct = 0, units = 0;
  for (int j = 0; j < m; ++j) {
    const int i = base + j;
    const jpegdec::Geometry g = jpegdec::geometry(hs[i], ws[i], samplings[i], ncomps[i]);
    tab.plan[j] = static_cast<const uint8_t*>(plans[i]);
    tab.out[j] = static_cast<uint8_t*>(outs[i]);
    tab.base[j] = bases[j];
    tab.hw[j] = uint32_t(hs[i]) << 16 | uint32_t(ws[i]);
    tab.mode[j] = uint8_t(samplings[i] | ncomps[i] << 2);
    if (idct <= INT_MAX) tab.first_idct[j] = int(idct);
    if (units <= INT_MAX) tab.first_rgb[j] = int(units);
    idct += (jpegdec::blocks(g) + kIdctBlocks - 1) / kIdctBlocks;
    units += (int64_t(jpegdec::plane_h(g, g.ncomp - 1)) * jpegdec::plane_w(g, g.ncomp - 1) + kThreads - 1) / kThreads;
  }
  if (idct > INT_MAX || units > INT_MAX) return fail(EXPO_E_BADARG, "too many blocks in one launch");
  if (!enqueue) return EXPO_OK;
  tab.first_idct[m] = int(idct), tab.first_rgb[m] = int(units);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(unsigned(idct)), dim3(kThreads), 0, s, tab, static_cast<uint8_t*>(workspace));
  HIP_TRY(hipGetLastError(), "jpeg_idct launch");
  hipLaunchKernelGGL(jpeg_rgb_kernel, dim3(unsigned(units)), dim3(kThreads), 0, s, tab, static_cast<const uint8_t*>(workspace));
  HIP_TRY(hipGetLastError(), "jpeg_rgb launch");
  return EXPO_OK;
}
}  // namespace expo

extern "C" {

size_t expo_jpeg_decode_plan_bytes(int nsegs) { return nsegs < 1 ? 0 : size_t(jpegdec::plan_bytes(nsegs)); }

size_t expo_jpeg_decode_workspace_bytes(const int* hs, const int* ws, const int* samplings, const int* ncomps, int n) {
  if (n < 1 || !hs || !ws || !samplings || !ncomps) return 0;
  for (int i = 0; i < n; ++i)
    if (!jpegdec::valid_picture(hs[i], ws[i], samplings[i], ncomps[i])) return 0;
  int64_t most = 0;  // a launch group at a time uses it
  for (int base = 0; base < n; base += kDecMaxImages) {
    const int64_t need = group_workspace(hs, ws, samplings, ncomps, base, n - base < kDecMaxImages ? n - base : kDecMaxImages, nullptr);
    most = need > most ? need : most;
  }
  return size_t(most);
}

int expo_jpeg_decode_ragged(const void* const* files, const int64_t* file_bytes, const void* const* plans, const int* hs,
                            const int* ws, const int* samplings, const int* ncomps, const int* nsegs, int n,
                            void* const* outs, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  // everything is checked before anything is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (n == 0) return EXPO_OK;
  if (!hs || !ws || !samplings || !ncomps || !nsegs || !file_bytes) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (hs[i] < 1 || ws[i] < 1 || hs[i] > jpegdec::kMaxDim || ws[i] > jpegdec::kMaxDim) return fail(EXPO_E_BADARG, "h and w in 1..65535 required");
    if (samplings[i] < 0 || samplings[i] > 2) return fail(EXPO_E_BADARG, "sampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)");
    if (ncomps[i] != 1 && ncomps[i] != 3) return fail(EXPO_E_BADARG, "ncomps must be 1 or 3");
    if (ncomps[i] == 1 && samplings[i] != 0) return fail(EXPO_E_BADARG, "a grey picture has sampling 0");
    if (!jpegdec::valid_segments(jpegdec::geometry(hs[i], ws[i], samplings[i], ncomps[i]), nsegs[i]))
      return fail(EXPO_E_BADARG, "nsegs must be ceil(mcus / Ri) of a restart interval Ri");
    if (file_bytes[i] < 0 || file_bytes[i] > INT_MAX) return fail(EXPO_E_BADARG, "file_bytes in 0..2^31-1 required");
  }
  if (!files || !plans || !outs || !status) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (!files[i] || !plans[i] || !outs[i]) return fail(EXPO_E_BADARG, "null picture pointer");
    if ((reinterpret_cast<uintptr_t>(plans[i]) & 15) != 0) return fail(EXPO_E_BADARG, "a plan must be 16-byte aligned");
  }
  if (workspace_bytes < expo_jpeg_decode_workspace_bytes(hs, ws, samplings, ncomps, n)) return fail(EXPO_E_BADARG, "workspace too small");
  if (!workspace) return fail(EXPO_E_BADARG, "null workspace");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(EXPO_E_BADARG, "the workspace must be 16-byte aligned");
  for (int base = 0; base < n; base += kDecMaxImages) {  // the grids of every group, before the first launch
    int64_t segs = 0, idct = 0, units = 0;
    for (int i = base; i < n && i < base + kDecMaxImages; ++i) {
      const jpegdec::Geometry g = jpegdec::geometry(hs[i], ws[i], samplings[i], ncomps[i]);
      segs += nsegs[i];
      idct += (jpegdec::blocks(g) + kIdctBlocks - 1) / kIdctBlocks;
      units += (int64_t(jpegdec::plane_h(g, g.ncomp - 1)) * jpegdec::plane_w(g, g.ncomp - 1) + kThreads - 1) / kThreads;
    }
    if (segs > INT_MAX - kEntropyThreads || idct > INT_MAX || units > INT_MAX) return fail(EXPO_E_BADARG, "too many blocks in one launch");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* wsp = static_cast<uint8_t*>(workspace);
  HIP_TRY(hipMemsetAsync(status, 0, size_t(n) * sizeof(int32_t), s), "jpeg_decode status memset");
  for (int base = 0; base < n; base += kDecMaxImages) {
    const int m = n - base < kDecMaxImages ? n - base : kDecMaxImages;
    DecTable tab = {};
    tab.n = m;
    group_workspace(hs, ws, samplings, ncomps, base, m, tab.base);
    int64_t segs = 0, idct = 0, units = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j;
      const jpegdec::Geometry g = jpegdec::geometry(hs[i], ws[i], samplings[i], ncomps[i]);
      tab.file[j] = static_cast<const uint8_t*>(files[i]);
      tab.plan[j] = static_cast<const uint8_t*>(plans[i]);
      tab.out[j] = static_cast<uint8_t*>(outs[i]);
      tab.file_bytes[j] = int(file_bytes[i]);
      tab.hw[j] = uint32_t(hs[i]) << 16 | uint32_t(ws[i]);
      tab.mode[j] = uint8_t(samplings[i] | ncomps[i] << 2);
      tab.first_seg[j] = int(segs);
      tab.first_idct[j] = int(idct);
      tab.first_rgb[j] = int(units);
      segs += nsegs[i];
      idct += (jpegdec::blocks(g) + kIdctBlocks - 1) / kIdctBlocks;
      units += (int64_t(jpegdec::plane_h(g, g.ncomp - 1)) * jpegdec::plane_w(g, g.ncomp - 1) + kThreads - 1) / kThreads;
    }
    tab.first_seg[m] = int(segs), tab.first_idct[m] = int(idct), tab.first_rgb[m] = int(units);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(unsigned((segs + kEntropyThreads - 1) / kEntropyThreads)), dim3(kEntropyThreads),
                       0, s, tab, wsp, status + base);
    HIP_TRY(hipGetLastError(), "jpeg_entropy launch");
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(unsigned(idct)), dim3(kThreads), 0, s, tab, wsp);
    HIP_TRY(hipGetLastError(), "jpeg_idct launch");
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3(unsigned(units)), dim3(kThreads), 0, s, tab, wsp);
    HIP_TRY(hipGetLastError(), "jpeg_rgb launch");
  }
  return EXPO_OK;
}

}  // extern "C"
