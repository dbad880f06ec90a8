// jpeg_decode_sync.hip -- baseline JPEG files without restart markers decoded in parallel on the device
// (expo_jpeg_decode_sync_ragged).  Such a file is one segment; it is cut into subsequences of sub_bytes
// file bytes, every subsequence is walked speculatively by a lane of its own, the lanes agree on their entry states,
// the agreement is verified, and every coefficient lands where the serial walk of jpeg_decode.hip would put it.  Default
// flags (csrc/build.sh).  Integer code only.  Per call one memset node for the status and one for the info words, then
// per group of up to 64 pictures, in stream order:
//   jpeg_sync_settle_kernel  256 lanes own 256 consecutive subsequences of one picture.  Round 0: every lane walks from the
//                            speculative state 0.  Every further round a lane takes the exit of the lane before it as its
//                            entry and walks again only if that changed; the loop ends when no lane of the workgroup
//                            changed (at most 256 rounds).  It is launched 1 + grid_rounds times; from the second launch
//                            on a workgroup's first lane takes the last exit of the workgroup before it, as the launch
//                            before left it in a ping-pong array, and a workgroup none of whose entries changes leaves
//                            after one comparison.
//   jpeg_sync_scan_kernel    one workgroup per picture: in[0] = 0 and in[i] = out[i - 1] up to the first dead exit prove by
//                            induction that every state is the serial walk's; the exclusive prefix sums of the blocks
//                            and of the DC differences give every subsequence its first block and its predictors; the
//                            picture's settled, good_blocks and last emitting subsequence, its status flag, its info word
//   a memset node            over the coefficients of the group's sync pictures
//   jpeg_sync_emit_kernel    a lane per subsequence of the settled pictures walks again and stores: plain 2-byte stores
//                            into zeroed coefficients, only into blocks below good_blocks
//   jpeg_sync_serial_kernel  a lane per segment runs jpeg_decode.h's decode_segment as jpeg_entropy_kernel does, for the
//                            pictures with restart intervals, those of one subsequence and those the scan found
//                            unsettled; a lane of a settled picture leaves at once
//   jpeg_idct_kernel, jpeg_rgb_kernel   jpeg_decode.hip's own, through its launcher
// The serial routines are jpeg_decode_sync.h's, which tools/jpeg_sync_rehearse.cpp runs on the host.
#include <limits.h>

#include "host_common.h"
#include "jpeg_decode_sync.h"

namespace expo {

// jpeg_decode.hip's launcher of the inverse transform and the colour kernel
int jpeg_decode_reconstruct(const void* const* plans, const int* hs, const int* ws, const int* samplings, const int* ncomps,
                            int base, int m, const int64_t* bases, void* const* outs, void* workspace, void* stream, bool enqueue);

namespace {

using namespace jpegsync;

constexpr int kSyncMaxImages = 64;
constexpr int kSerialThreads = 64;  // one wave: 64 segments
constexpr int kSlotVecs = 9;        // a lane's LDS slot: 128 bytes and 16 of padding, in 16-byte vectors
constexpr int kMaxSubs = 1 << 26;   // 2^31 file bytes in subsequences of 32
constexpr int kNone = INT_MAX;

// up to 64 pictures by value in the kernel arguments
struct SyncTable {
  const uint8_t* file[kSyncMaxImages];
  const uint8_t* plan[kSyncMaxImages];
  int64_t base[kSyncMaxImages];         // the picture's part of the workspace (jpegdec::layout)
  int64_t sbase[kSyncMaxImages];        // a sync picture's states (jpegsync::sync_layout)
  int file_bytes[kSyncMaxImages];
  uint32_t hw[kSyncMaxImages];          // h << 16 | w
  int nsubs[kSyncMaxImages];            // the host's count
  int first_group[kSyncMaxImages + 1];  // first workgroup of the settle and of the emit launch (sync pictures have some)
  int first_seg[kSyncMaxImages + 1];    // first segment of the serial launch
  uint8_t mode[kSyncMaxImages];         // sampling | ncomp << 2 | sync << 4
  int n, sub_bytes, round;
};
static_assert(sizeof(SyncTable) + 32 <= 4096, "the table must fit the 4 KB kernarg block");

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

__device__ __forceinline__ Geometry table_geometry(const SyncTable& tab, int j) {
  const uint32_t hw = tab.hw[j];
  const int mode = tab.mode[j];
  return geometry(int(hw >> 16), int(hw & 0xFFFFu), mode & 3, (mode >> 2) & 3);
}

// the subsequences the lanes may touch: the host's count (the workspace has that many) and no more than the segment has
__device__ __forceinline__ int live_subs(const SyncTable& tab, int pic, const Segment& seg) {
  const int64_t have = sub_count(seg.end - seg.begin, tab.sub_bytes);
  return have < tab.nsubs[pic] ? int(have) : tab.nsubs[pic];
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_settle_kernel(const SyncTable tab, uint8_t* __restrict__ ws) {
  __shared__ uint32_t exits[2][kGroup];
  const int lane = int(threadIdx.x);
  const int pic = find_image(tab.first_group, tab.n, int(blockIdx.x));
  const int wg = int(blockIdx.x) - tab.first_group[pic];
  const Geometry g = table_geometry(tab, pic);
  const uint8_t* file = tab.file[pic];
  const uint8_t* planp = tab.plan[pic];
  const int file_bytes = tab.file_bytes[pic], sub_bytes = tab.sub_bytes, round = tab.round;
  const Segment seg = plan_segment(planp, file_bytes);
  const SyncLayout lay = sync_layout(tab.sbase[pic], tab.nsubs[pic]);
  uint32_t* ins = reinterpret_cast<uint32_t*>(ws + lay.in);
  uint32_t* outs = reinterpret_cast<uint32_t*>(ws + lay.out);
  uint4* pays = reinterpret_cast<uint4*>(ws + lay.pay);
  uint32_t* edge = reinterpret_cast<uint32_t*>(ws + lay.edge);
  const int64_t groups = sync_groups(tab.nsubs[pic]);
  const int i = wg * kGroup + lane;
  const bool live = i < live_subs(tab, pic, seg);
  SubBits u;
  u.pos = seg.end, u.bits = 0;
  if (live) u = sub_bits(file, seg, sub_bytes, i);
  uint32_t in = 0, out = 0;
  Payload pay = {0u, {0u, 0u, 0u}};
  bool changed = false, dirty = false;
  if (round == 0) {
    changed = live;
  } else if (live) {
    in = ins[i], out = outs[i];
    const uint4 p = pays[i];
    pay.n = p.x, pay.dc[0] = p.y, pay.dc[1] = p.z, pay.dc[2] = p.w;
    if (lane == 0 && wg > 0) {
      const uint32_t before = edge[((round - 1) & 1) * groups + wg - 1];
      changed = before != in;
      in = before;
    }
  }
  if (changed) {
    out = walk(file, file_bytes, planp, g, seg, sub_bytes, u, in, &pay);
    dirty = true;
  }
  int buf = 0;
  for (int e = 0; e < kGroup; ++e) {
    exits[buf][lane] = out;
    if (!__syncthreads_or(changed ? 1 : 0)) break;
    const uint32_t before = lane > 0 ? exits[buf][lane - 1] : in;
    changed = live && before != in;
    if (changed) {
      in = before;
      out = walk(file, file_bytes, planp, g, seg, sub_bytes, u, in, &pay);
      dirty = true;
    }
    buf ^= 1;
  }
  if (live && dirty) {
    ins[i] = in, outs[i] = out;
    pays[i] = make_uint4(pay.n, pay.dc[0], pay.dc[1], pay.dc[2]);
  }
  if (live && lane == kGroup - 1) edge[(round & 1) * groups + wg] = out;
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_scan_kernel(const SyncTable tab, uint8_t* __restrict__ ws,
                                                                int32_t* __restrict__ status, int32_t* __restrict__ info) {
  __shared__ uint4 sums[2][kGroup];
  __shared__ int first_dead, first_bad;
  __shared__ uint32_t verdict[2];  // the blocks ended before the error, its flag
  const int pic = int(blockIdx.x), lane = int(threadIdx.x);
  if (!(tab.mode[pic] >> 4)) return;
  const Geometry g = table_geometry(tab, pic);
  const Segment seg = plan_segment(tab.plan[pic], tab.file_bytes[pic]);
  const int nsubs = tab.nsubs[pic];
  const SyncLayout lay = sync_layout(tab.sbase[pic], nsubs);
  const uint32_t* ins = reinterpret_cast<const uint32_t*>(ws + lay.in);
  const uint32_t* outs = reinterpret_cast<const uint32_t*>(ws + lay.out);
  const uint4* pays = reinterpret_cast<const uint4*>(ws + lay.pay);
  uint4* firsts = reinterpret_cast<uint4*>(ws + lay.first);
  bool settled = sub_count(seg.end - seg.begin, tab.sub_bytes) == nsubs;  // a wrong count: the serial lane decodes
  int64_t blocks_before = 0;  // the carried totals: uniform
  uint32_t dc0 = 0, dc1 = 0, dc2 = 0;
  int dead_at = kNone;
  for (int chunk = 0; settled && chunk < nsubs; chunk += kGroup) {
    if (lane == 0) first_dead = kNone, first_bad = kNone;
    __syncthreads();
    const int i = chunk + lane;
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
    uint32_t flag = 0;
    if (i < nsubs) {
      const uint4 p = pays[i];
      if (ins[i] != (i ? outs[i - 1] : 0u)) atomicMin(&first_bad, lane);
      if (outs[i] & kDead) atomicMin(&first_dead, lane);
      mine = make_uint4(p.x & kCountMask, p.y, p.z, p.w);
      flag = p.x >> 28;
    }
    int buf = 0;
    sums[0][lane] = mine;
    __syncthreads();
    for (int d = 1; d < kGroup; d <<= 1) {
      uint4 v = sums[buf][lane];
      if (lane >= d) {
        const uint4 o = sums[buf][lane - d];
        v.x += o.x, v.y += o.y, v.z += o.z, v.w += o.w;
      }
      sums[buf ^ 1][lane] = v;
      buf ^= 1;
      __syncthreads();
    }
    const uint4 incl = sums[buf][lane], total = sums[buf][kGroup - 1];
    const int dead = first_dead, bad = first_bad;
    const int last = dead != kNone ? dead : (nsubs - chunk < kGroup ? nsubs - chunk : kGroup) - 1;
    if (bad <= last) {
      settled = false;
    } else {
      if (lane <= last) {
        const int64_t first = blocks_before + (incl.x - mine.x);
        firsts[i] = make_uint4(uint32_t(first < kBlockCap ? first : kBlockCap), dc0 + incl.y - mine.y, dc1 + incl.z - mine.z,
                               dc2 + incl.w - mine.w);
        if (lane == dead) {
          const int64_t ended = blocks_before + incl.x;
          verdict[0] = uint32_t(ended < kBlockCap ? ended : kBlockCap), verdict[1] = flag;
        }
      }
      blocks_before += total.x;
      blocks_before = blocks_before < kBlockCap ? blocks_before : kBlockCap;
      dc0 += total.y, dc1 += total.z, dc2 += total.w;
      if (dead != kNone) dead_at = chunk + dead;
    }
    __syncthreads();
    if (dead_at != kNone) break;
  }
  if (lane != 0) return;
  const int64_t all = blocks(g);
  int64_t ended = blocks_before;
  int flag = kTruncated;  // no error and too few blocks: the serial lane's next symbol finds no bits
  if (dead_at != kNone) ended = verdict[0], flag = int(verdict[1]);
  uint32_t* result = reinterpret_cast<uint32_t*>(ws + lay.result);
  if (settled) {
    // the walk behind the picture's last block reads the padding bits, which the serial lane never reads: an error there,
    // or blocks beyond the picture's, is none
    const int64_t good = ended < all ? ended : all;
    if (ended < all) atomicOr(&status[pic], flag);
    result[0] = 1u, result[1] = uint32_t(good), result[2] = uint32_t(dead_at != kNone ? dead_at : nsubs - 1);
  } else {
    result[0] = 0u, result[1] = 0u, result[2] = 0u;
  }
  result[3] = 0u;
  if (info) info[pic] = settled ? 1 : 2;
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_emit_kernel(const SyncTable tab, uint8_t* __restrict__ ws) {
  const int pic = find_image(tab.first_group, tab.n, int(blockIdx.x));
  const int i = (int(blockIdx.x) - tab.first_group[pic]) * kGroup + int(threadIdx.x);
  const SyncLayout lay = sync_layout(tab.sbase[pic], tab.nsubs[pic]);
  const uint4 result = *reinterpret_cast<const uint4*>(ws + lay.result);
  if (!result.x || i > int(result.z) || i >= tab.nsubs[pic]) return;  // settled: the host's count is the segment's
  const Geometry g = table_geometry(tab, pic);
  const int file_bytes = tab.file_bytes[pic];
  const Segment seg = plan_segment(tab.plan[pic], file_bytes);
  const SubBits u = sub_bits(tab.file[pic], seg, tab.sub_bytes, i);
  const uint32_t in = reinterpret_cast<const uint32_t*>(ws + lay.in)[i];
  const uint4 first = reinterpret_cast<const uint4*>(ws + lay.first)[i];
  const uint32_t pred[3] = {first.y, first.z, first.w};
  emit(tab.file[pic], file_bytes, tab.plan[pic], g, seg, tab.sub_bytes, u, in, int64_t(first.x), pred, int64_t(result.y),
       reinterpret_cast<int16_t*>(ws + tab.base[pic]));
}

__global__ __launch_bounds__(kSerialThreads) void jpeg_sync_serial_kernel(const SyncTable tab, uint8_t* __restrict__ ws,
                                                                          int32_t* __restrict__ status) {
  __shared__ uint4 slots[kSerialThreads * kSlotVecs];
  const int lane = int(threadIdx.x);
  const int total = tab.first_seg[tab.n];
  const int seg0 = int(blockIdx.x) * kSerialThreads;
  const int seg = seg0 + lane;
  // the pictures of this wave's segments: uniform bounds, a lane keeps the last one that starts at or before its segment
  const int jlo = find_image(tab.first_seg, tab.n, seg0);
  const int jhi = find_image(tab.first_seg, tab.n, seg0 + kSerialThreads - 1 < total - 1 ? seg0 + kSerialThreads - 1 : total - 1);
  const uint8_t* file = nullptr;
  const uint8_t* planp = nullptr;
  int64_t base = 0, sbase = 0;
  int file_bytes = 0, first = 0, pic = 0, mode = 4, nsubs = 1;
  uint32_t hw = (1u << 16) | 1u;
  for (int j = jlo; j <= jhi; ++j) {
    const int f = tab.first_seg[j];
    if (seg >= f) {
      file = tab.file[j], planp = tab.plan[j], base = tab.base[j], sbase = tab.sbase[j], file_bytes = tab.file_bytes[j];
      first = f, pic = j, mode = tab.mode[j], hw = tab.hw[j], nsubs = tab.nsubs[j];
    }
  }
  if (seg >= total) return;
  if (mode >> 4 && *reinterpret_cast<const uint32_t*>(ws + sync_layout(sbase, nsubs).result)) return;  // settled
  const Geometry g = geometry(int(hw >> 16), int(hw & 0xFFFFu), mode & 3, (mode >> 2) & 3);
  const int k = seg - first;  // 0 <= k < nsegs: the host checked nsegs against the geometry
  const int st = decode_segment(file, file_bytes, planp, g, k, &slots[lane * kSlotVecs], reinterpret_cast<uint4*>(ws + base),
                                make_uint4(0u, 0u, 0u, 0u));
  if (st) atomicOr(&status[pic], st);
}

// the workspace of images [base, base + m): the pictures' parts behind one another as expo_jpeg_decode_ragged lays them
// out, then the sync pictures' states
int64_t group_workspace(const int* hs, const int* ws, const int* samplings, const int* ncomps, const int* nsegs, const int* nsubs,
                        int base, int m, int64_t* bases, int64_t* sbases) {
  int64_t at = 0;
  for (int j = 0; j < m; ++j) {
    if (bases) bases[j] = at;
    at = layout(at, geometry(hs[base + j], ws[base + j], samplings[base + j], ncomps[base + j])).end;
  }
  for (int j = 0; j < m; ++j) {
    if (sbases) sbases[j] = at;
    if (is_sync(nsegs[base + j], nsubs[base + j])) at = sync_layout(at, nsubs[base + j]).end;
  }
  return at;
}

bool valid_counts(const int* hs, const int* ws, const int* samplings, const int* ncomps, const int* nsegs, const int* nsubs, int i) {
  return valid_picture(hs[i], ws[i], samplings[i], ncomps[i]) &&
         valid_segments(geometry(hs[i], ws[i], samplings[i], ncomps[i]), nsegs[i]) && nsubs[i] >= 1 && nsubs[i] <= kMaxSubs &&
         (nsegs[i] == 1 || nsubs[i] == 1);
}

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

size_t expo_jpeg_decode_sync_workspace_bytes(const int* hs, const int* ws, const int* samplings, const int* ncomps,
                                             const int* nsegs, const int* nsubs, int n) {
  if (n < 1 || !hs || !ws || !samplings || !ncomps || !nsegs || !nsubs) return 0;
  for (int i = 0; i < n; ++i)
    if (!valid_counts(hs, ws, samplings, ncomps, nsegs, nsubs, i)) return 0;
  int64_t most = 0;  // a launch group at a time uses it
  for (int base = 0; base < n; base += kSyncMaxImages) {
    const int64_t need = group_workspace(hs, ws, samplings, ncomps, nsegs, nsubs, base, n - base < kSyncMaxImages ? n - base : kSyncMaxImages,
                                         nullptr, nullptr);
    most = need > most ? need : most;
  }
  return size_t(most);
}

int expo_jpeg_decode_sync_ragged(const void* const* files, const int64_t* file_bytes, const void* const* plans, const int* hs,
                                 const int* ws, const int* samplings, const int* ncomps, const int* nsegs, const int* nsubs,
                                 int n, int sub_bytes, int grid_rounds, void* const* outs, int32_t* status, int32_t* info,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  // everything is checked before anything is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (n == 0) return EXPO_OK;
  if (!valid_sub_bytes(sub_bytes)) return fail(EXPO_E_BADARG, "sub_bytes must be a multiple of 16 in 32..65536");
  if (grid_rounds < 0 || grid_rounds > kMaxGridRounds) return fail(EXPO_E_BADARG, "grid_rounds in 0..16 required");
  if (!hs || !ws || !samplings || !ncomps || !nsegs || !nsubs || !file_bytes) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (hs[i] < 1 || ws[i] < 1 || hs[i] > kMaxDim || ws[i] > kMaxDim) return fail(EXPO_E_BADARG, "h and w in 1..65535 required");
    if (samplings[i] < 0 || samplings[i] > 2) return fail(EXPO_E_BADARG, "sampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)");
    if (ncomps[i] != 1 && ncomps[i] != 3) return fail(EXPO_E_BADARG, "ncomps must be 1 or 3");
    if (ncomps[i] == 1 && samplings[i] != 0) return fail(EXPO_E_BADARG, "a grey picture has sampling 0");
    if (!valid_segments(geometry(hs[i], ws[i], samplings[i], ncomps[i]), nsegs[i]))
      return fail(EXPO_E_BADARG, "nsegs must be ceil(mcus / Ri) of a restart interval Ri");
    if (file_bytes[i] < 0 || file_bytes[i] > INT_MAX) return fail(EXPO_E_BADARG, "file_bytes in 0..2^31-1 required");
    if (nsubs[i] < 1 || nsubs[i] > kMaxSubs) return fail(EXPO_E_BADARG, "nsubs in 1..2^26 required");
    if (nsegs[i] != 1 && nsubs[i] != 1) return fail(EXPO_E_BADARG, "nsubs must be 1 for a picture with restart intervals");
  }
  if (!files || !plans || !outs || !status) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (!files[i] || !plans[i] || !outs[i]) return fail(EXPO_E_BADARG, "null picture pointer");
    if ((reinterpret_cast<uintptr_t>(plans[i]) & 15) != 0) return fail(EXPO_E_BADARG, "a plan must be 16-byte aligned");
  }
  if (workspace_bytes < expo_jpeg_decode_sync_workspace_bytes(hs, ws, samplings, ncomps, nsegs, nsubs, n))
    return fail(EXPO_E_BADARG, "workspace too small");
  if (!workspace) return fail(EXPO_E_BADARG, "null workspace");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(EXPO_E_BADARG, "the workspace must be 16-byte aligned");
  int64_t bases[kSyncMaxImages], sbases[kSyncMaxImages];
  for (int base = 0; base < n; base += kSyncMaxImages) {  // the grids of every group, before the first launch
    const int m = n - base < kSyncMaxImages ? n - base : kSyncMaxImages;
    int64_t segs = 0;
    for (int i = base; i < base + m; ++i) segs += nsegs[i];
    if (segs > INT_MAX - kSerialThreads) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    group_workspace(hs, ws, samplings, ncomps, nsegs, nsubs, base, m, bases, sbases);
    const int rc = jpeg_decode_reconstruct(plans, hs, ws, samplings, ncomps, base, m, bases, outs, workspace, stream, false);
    if (rc != EXPO_OK) return rc;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* wsp = static_cast<uint8_t*>(workspace);
  HIP_TRY(hipMemsetAsync(status, 0, size_t(n) * sizeof(int32_t), s), "jpeg_decode_sync status memset");
  if (info) HIP_TRY(hipMemsetAsync(info, 0, size_t(n) * sizeof(int32_t), s), "jpeg_decode_sync info memset");
  for (int base = 0; base < n; base += kSyncMaxImages) {
    const int m = n - base < kSyncMaxImages ? n - base : kSyncMaxImages;
    SyncTable tab = {};
    tab.n = m, tab.sub_bytes = sub_bytes;
    group_workspace(hs, ws, samplings, ncomps, nsegs, nsubs, base, m, tab.base, tab.sbase);
    int64_t segs = 0, groups = 0, zero_from = -1, zero_to = -1;
    for (int j = 0; j < m; ++j) {
      const int i = base + j;
      const bool sync = is_sync(nsegs[i], nsubs[i]);
      tab.file[j] = static_cast<const uint8_t*>(files[i]);
      tab.plan[j] = static_cast<const uint8_t*>(plans[i]);
      tab.file_bytes[j] = int(file_bytes[i]);
      tab.hw[j] = uint32_t(hs[i]) << 16 | uint32_t(ws[i]);
      tab.nsubs[j] = nsubs[i];
      tab.mode[j] = uint8_t(samplings[i] | ncomps[i] << 2 | (sync ? 16 : 0));
      tab.first_group[j] = int(groups);
      tab.first_seg[j] = int(segs);
      segs += nsegs[i];
      if (sync) {
        groups += sync_groups(nsubs[i]);
        if (zero_from < 0) zero_from = tab.base[j];
        zero_to = tab.base[j] + blocks(geometry(hs[i], ws[i], samplings[i], ncomps[i])) * 128;
      }
    }
    tab.first_group[m] = int(groups), tab.first_seg[m] = int(segs);
    if (groups > 0) {
      for (int round = 0; round <= grid_rounds; ++round) {
        tab.round = round;
        hipLaunchKernelGGL(jpeg_sync_settle_kernel, dim3(unsigned(groups)), dim3(kGroup), 0, s, tab, wsp);
        HIP_TRY(hipGetLastError(), "jpeg_sync_settle launch");
      }
      hipLaunchKernelGGL(jpeg_sync_scan_kernel, dim3(unsigned(m)), dim3(kGroup), 0, s, tab, wsp, status + base,
                         info ? info + base : nullptr);
      HIP_TRY(hipGetLastError(), "jpeg_sync_scan launch");
      // from the first sync picture's coefficients to the last one's: the planes in between are written later
      HIP_TRY(hipMemsetAsync(wsp + zero_from, 0, size_t(zero_to - zero_from), s), "jpeg_decode_sync coefficient memset");
      hipLaunchKernelGGL(jpeg_sync_emit_kernel, dim3(unsigned(groups)), dim3(kGroup), 0, s, tab, wsp);
      HIP_TRY(hipGetLastError(), "jpeg_sync_emit launch");
    }
    hipLaunchKernelGGL(jpeg_sync_serial_kernel, dim3(unsigned((segs + kSerialThreads - 1) / kSerialThreads)), dim3(kSerialThreads), 0, s,
                       tab, wsp, status + base);
    HIP_TRY(hipGetLastError(), "jpeg_sync_serial launch");
    const int rc = jpeg_decode_reconstruct(plans, hs, ws, samplings, ncomps, base, m, tab.base, outs, workspace, stream, true);
    if (rc != EXPO_OK) return rc;
  }
  return EXPO_OK;
}

}  // extern "C"
