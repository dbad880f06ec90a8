// jpeg_sync_rehearse.cpp -- the integer routines of exposure_amd/csrc/jpeg_decode_sync.h on the host, without a GPU: a
// serial walk through the phases of csrc/jpeg_decode_sync.hip's launches -- the settle launches with their workgroups of
// 256 lanes, their rounds and the ping-pong boundary words, the scan, the coefficient memset, the emit, the serial
// fallback -- and jpeg_decode.hip's reconstruction, over whole files.  Its own main; build it with the sanitizers and
// run it directly:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/jpeg_sync_rehearse.cpp -o jpeg_sync_rehearse
//   jpeg_sync_rehearse selftest
//   jpeg_sync_rehearse decode SUB_BYTES GRID_ROUNDS in.jpg in.plan H W SAMPLING NCOMPS NSEGS out.rgb [the same eight ...]
// in.plan is the blob of exposure_amd/jpeg_decode.py's parse.  The file, the plan, the workspace and the output live in
// heap buffers of exactly the sizes the ABI reports, the workspace full of a sentinel, so a read or write that the
// device would have to clamp shows under AddressSanitizer.  Prints per file its status word and its info word;
// out.rgb is H*W*3 bytes (tests/test_jpeg_sync_host.py compares all three with the restatement).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../exposure_amd/csrc/jpeg_decode_sync.h"

using namespace expo::jpegsync;

namespace {

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

struct Vec16 {
  uint32_t a[4];
};

bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* in = fopen(path, "rb");
  if (!in) return false;
  fseek(in, 0, SEEK_END);
  const long n = ftell(in);
  fseek(in, 0, SEEK_SET);
  out->resize(size_t(n));
  const bool ok = n == 0 || fread(out->data(), 1, size_t(n), in) == size_t(n);
  fclose(in);
  return ok;
}

// jpeg_sync_settle_kernel, launch `round`: workgroup by workgroup, the lanes of a round one after another on the exits
// the round before left (the kernel's double buffer)
void settle_launch(const uint8_t* file, int64_t file_bytes, const uint8_t* planp, const Geometry& g, const Segment& seg,
                   int sub_bytes, int nsubs, int round, uint8_t* ws, const SyncLayout& lay) {
  uint32_t* ins = reinterpret_cast<uint32_t*>(ws + lay.in);
  uint32_t* outs = reinterpret_cast<uint32_t*>(ws + lay.out);
  Payload* pays = reinterpret_cast<Payload*>(ws + lay.pay);
  uint32_t* edge = reinterpret_cast<uint32_t*>(ws + lay.edge);
  const int64_t groups = sync_groups(nsubs);
  const int64_t have = sub_count(seg.end - seg.begin, sub_bytes);
  const int live_subs = have < nsubs ? int(have) : nsubs;
  for (int wg = 0; wg < groups; ++wg) {
    uint32_t in[kGroup], out[kGroup], shown[kGroup];
    Payload pay[kGroup];
    SubBits u[kGroup];
    bool live[kGroup], changed[kGroup], dirty[kGroup];
    for (int lane = 0; lane < kGroup; ++lane) {
      const int i = wg * kGroup + lane;
      live[lane] = i < live_subs;
      u[lane].pos = seg.end, u[lane].bits = 0;
      if (live[lane]) u[lane] = sub_bits(file, seg, sub_bytes, i);
      in[lane] = 0, out[lane] = 0, pay[lane] = Payload{0, {0, 0, 0}};
      changed[lane] = false, dirty[lane] = false;
      if (round == 0) {
        changed[lane] = live[lane];
      } else if (live[lane]) {
        in[lane] = ins[i], out[lane] = outs[i], pay[lane] = pays[i];
        if (lane == 0 && wg > 0) {
          const uint32_t before = edge[((round - 1) & 1) * groups + wg - 1];
          changed[lane] = before != in[lane];
          in[lane] = before;
        }
      }
      if (changed[lane]) {
        out[lane] = walk(file, file_bytes, planp, g, seg, sub_bytes, u[lane], in[lane], &pay[lane]);
        dirty[lane] = true;
      }
    }
    for (int e = 0; e < kGroup; ++e) {
      bool any = false;
      for (int lane = 0; lane < kGroup; ++lane) shown[lane] = out[lane], any = any || changed[lane];
      if (!any) break;
      for (int lane = 0; lane < kGroup; ++lane) {
        const uint32_t before = lane > 0 ? shown[lane - 1] : in[lane];
        changed[lane] = live[lane] && before != in[lane];
        if (changed[lane]) {
          in[lane] = before;
          out[lane] = walk(file, file_bytes, planp, g, seg, sub_bytes, u[lane], in[lane], &pay[lane]);
          dirty[lane] = true;
        }
      }
    }
    for (int lane = 0; lane < kGroup; ++lane) {
      const int i = wg * kGroup + lane;
      if (live[lane] && dirty[lane]) ins[i] = in[lane], outs[i] = out[lane], pays[i] = pay[lane];
      if (live[lane] && lane == kGroup - 1) edge[(round & 1) * groups + wg] = out[lane];
    }
  }
}

// jpeg_sync_scan_kernel: chunk by chunk with the carried totals; -> the status flag it sets
int scan(const Geometry& g, const Segment& seg, int sub_bytes, int nsubs, uint8_t* ws, const SyncLayout& lay) {
  const uint32_t* ins = reinterpret_cast<const uint32_t*>(ws + lay.in);
  const uint32_t* outs = reinterpret_cast<const uint32_t*>(ws + lay.out);
  const Payload* pays = reinterpret_cast<const Payload*>(ws + lay.pay);
  uint32_t* firsts = reinterpret_cast<uint32_t*>(ws + lay.first);
  uint32_t* result = reinterpret_cast<uint32_t*>(ws + lay.result);
  bool settled = sub_count(seg.end - seg.begin, sub_bytes) == nsubs;
  int64_t blocks_before = 0, ended = 0;
  uint32_t dc[3] = {0, 0, 0};
  int dead_at = -1, flag = kTruncated;
  for (int chunk = 0; settled && chunk < nsubs && dead_at < 0; chunk += kGroup) {
    const int count = nsubs - chunk < kGroup ? nsubs - chunk : kGroup;
    int dead = -1, bad = -1;
    for (int lane = count - 1; lane >= 0; --lane) {
      const int i = chunk + lane;
      if (ins[i] != (i ? outs[i - 1] : 0u)) bad = lane;
      if (outs[i] & kDead) dead = lane;
    }
    const int last = dead >= 0 ? dead : count - 1;
    if (bad >= 0 && bad <= last) {
      settled = false;
      break;
    }
    for (int lane = 0; lane <= last; ++lane) {
      const int i = chunk + lane;
      firsts[4 * i] = uint32_t(blocks_before < kBlockCap ? blocks_before : kBlockCap);
      firsts[4 * i + 1] = dc[0], firsts[4 * i + 2] = dc[1], firsts[4 * i + 3] = dc[2];
      blocks_before += pays[i].n & kCountMask;
      for (int c = 0; c < 3; ++c) dc[c] += pays[i].dc[c];
      if (lane == dead) dead_at = i, flag = int(pays[i].n >> 28);
    }
    blocks_before = blocks_before < kBlockCap ? blocks_before : kBlockCap;
  }
  ended = blocks_before;
  const int64_t all = blocks(g);
  int status = 0;
  if (settled) {
    if (ended < all) status = flag;
    result[0] = 1, result[1] = uint32_t(ended < all ? ended : all), result[2] = uint32_t(dead_at >= 0 ? dead_at : nsubs - 1);
  } else {
    result[0] = 0, result[1] = 0, result[2] = 0;
  }
  result[3] = 0;
  return status;
}

// the launches of one call on one picture; every buffer of exactly its size, on the heap
int decode_file(const std::vector<uint8_t>& file, const std::vector<uint8_t>& plan, int h, int w, int sampling, int ncomp,
                int nsegs, int sub_bytes, int grid_rounds, std::vector<uint8_t>* rgb_out, int* info) {
  const Geometry g = geometry(h, w, sampling, ncomp);
  const Layout lay = layout(0, g);
  CHECK(int64_t(plan.size()) == plan_bytes(nsegs) && valid_segments(g, nsegs) && valid_sub_bytes(sub_bytes));
  std::vector<Vec16> planv(plan.size() / 16);
  memcpy(planv.data(), plan.data(), plan.size());
  const uint8_t* planp = reinterpret_cast<const uint8_t*>(planv.data());
  const Segment seg = plan_segment(planp, int64_t(file.size()));
  const int nsubs = nsegs == 1 ? int(sub_count(seg.end - seg.begin, sub_bytes)) : 1;  // what Plan.nsubs gives the call
  const bool sync = is_sync(nsegs, nsubs);
  const SyncLayout slay = sync_layout(lay.end, nsubs);
  const int64_t ws_bytes = sync ? slay.end : lay.end;
  CHECK(ws_bytes % 16 == 0);
  std::vector<Vec16> wsv(size_t(ws_bytes) / 16, Vec16{{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}});
  uint8_t* ws = reinterpret_cast<uint8_t*>(wsv.data());
  int status = 0;
  *info = 0;
  bool settled = false;
  if (sync) {
    for (int round = 0; round <= grid_rounds; ++round)
      settle_launch(file.data(), int64_t(file.size()), planp, g, seg, sub_bytes, nsubs, round, ws, slay);
    status |= scan(g, seg, sub_bytes, nsubs, ws, slay);
    const uint32_t* result = reinterpret_cast<const uint32_t*>(ws + slay.result);
    settled = result[0] != 0;
    *info = settled ? 1 : 2;
    memset(ws + lay.coef, 0, size_t(blocks(g)) * 128);  // the memset node
    if (settled) {  // jpeg_sync_emit_kernel: a lane per subsequence
      const uint32_t* ins = reinterpret_cast<const uint32_t*>(ws + slay.in);
      const uint32_t* firsts = reinterpret_cast<const uint32_t*>(ws + slay.first);
      for (int i = 0; i < nsubs && i <= int(result[2]); ++i) {
        const SubBits u = sub_bits(file.data(), seg, sub_bytes, i);
        const uint32_t pred[3] = {firsts[4 * i + 1], firsts[4 * i + 2], firsts[4 * i + 3]};
        emit(file.data(), int64_t(file.size()), planp, g, seg, sub_bytes, u, ins[i], int64_t(firsts[4 * i]), pred, int64_t(result[1]),
             reinterpret_cast<int16_t*>(ws + lay.coef));
      }
    }
  }
  if (!settled) {  // jpeg_sync_serial_kernel: a lane per segment, its own slot
    for (int k = 0; k < nsegs; ++k) {
      Vec16 slot[8];
      status |= decode_segment(file.data(), int64_t(file.size()), planp, g, k, slot, reinterpret_cast<Vec16*>(ws + lay.coef), Vec16{{0, 0, 0, 0}});
    }
  }
  // jpeg_idct_kernel: eight "threads" per block over a block's 72 int32 of LDS, in the kernel's three phases
  const PlanHead* head = reinterpret_cast<const PlanHead*>(planp);
  const int64_t nblk = blocks(g);
  for (int64_t b = 0; b < nblk; ++b) {
    int32_t mine[72];
    for (int e = 0; e < 72; ++e) mine[e] = 0x5A5A5A5A;
    const int64_t m = b / g.bpm;
    const int jj = int(b - m * g.bpm);
    const int comp = block_component(g, jj);
    int brow, bcol;
    block_place(g, m, jj, &brow, &bcol);
    const int16_t* coef = reinterpret_cast<const int16_t*>(ws + lay.coef + b * 128);
    const uint8_t* q = head->q[head->tq[comp] & 3];
    for (int r = 0; r < 8; ++r)
      for (int x = 0; x < 8; ++x) mine[r * 9 + x] = int32_t(coef[r * 8 + x]) * int32_t(q[r * 8 + x]);
    for (int r = 0; r < 8; ++r) {
      int32_t in[8], o[8];
      for (int v = 0; v < 8; ++v) in[v] = mine[v * 9 + r];
      idct_pass(in, 11, o);
      for (int v = 0; v < 8; ++v) mine[v * 9 + r] = o[v];
    }
    for (int r = 0; r < 8; ++r) {
      int32_t in[8], o[8];
      for (int x = 0; x < 8; ++x) in[x] = mine[r * 9 + x];
      idct_pass(in, 18, o);
      const int y = brow * 8 + r, x0 = bcol * 8, pw = plane_w(g, comp);
      if (y < plane_h(g, comp) && x0 < pw) {
        uint8_t* dst = ws + lay.plane[comp] + int64_t(y) * plane_stride(g, comp) + x0;
        const int nx = x0 + 8 <= pw ? 8 : pw - x0;
        for (int x = 0; x < nx; ++x) dst[x] = uint8_t(clamp255(o[x] + 128));
      }
    }
  }
  // jpeg_rgb_kernel: a thread per chroma sample
  rgb_out->assign(size_t(h) * size_t(w) * 3, 0xA5);
  const int dh = plane_h(g, g.ncomp - 1), dw = plane_w(g, g.ncomp - 1);
  for (int uy = 0; uy < dh; ++uy)
    for (int ux = 0; ux < dw; ++ux) rgb_unit(g, lay, ws, rgb_out->data(), uy, ux);
  return status;
}

int selftest() {
  CHECK(valid_sub_bytes(32) && valid_sub_bytes(65536) && !valid_sub_bytes(16) && !valid_sub_bytes(40) && !valid_sub_bytes(65552));
  CHECK(sub_count(0, 32) == 1 && sub_count(32, 32) == 1 && sub_count(33, 32) == 2 && sub_count(64, 32) == 2);
  CHECK(pack_state(31, 5, 63) == (31u | 5u << 5 | 63u << 8) && !(pack_state(31, 7, 63) & kDead));
  // the workspace pieces: 300 subsequences are two workgroups
  const SyncLayout l = sync_layout(64, 300);
  CHECK(l.in == 64 && l.out == 64 + 1200 && l.pay == l.out + 1200 && l.first == l.pay + 4800 && l.edge == l.first + 4800 &&
        l.result == l.edge + 16 && l.end == l.result + 16);
  CHECK(sync_layout(0, 2).end == 16 + 16 + 32 + 32 + 16 + 16);
  // the bits of a subsequence: a stuffed 00 at its start is dropped, an FF at its end is its own
  uint8_t bytes[70];
  for (int e = 0; e < 70; ++e) bytes[e] = uint8_t(e + 1);
  bytes[33] = 0xFF, bytes[34] = 0x00;  // begin = 3: subsequence 0 is [3, 35), subsequence 1 [35, 67), subsequence 2 [67, 70)
  bytes[66] = 0xFF, bytes[67] = 0x00;
  const Segment seg = {3, 70};
  SubBits u = sub_bits(bytes, seg, 32, 0);
  CHECK(u.pos == 3 && u.bits == 8 * 31);
  u = sub_bits(bytes, seg, 32, 1);
  CHECK(u.pos == 35 && u.bits == 8 * 32);
  u = sub_bits(bytes, seg, 32, 2);
  CHECK(u.pos == 68 && u.bits == 8 * 2);
  bytes[2] = 0xFF, bytes[3] = 0x00;  // an FF before `begin` is not the segment's
  u = sub_bits(bytes, seg, 32, 0);
  CHECK(u.pos == 3 && u.bits == 8 * 31);
  printf("jpeg_sync_rehearse selftest: ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc >= 12 && (argc - 4) % 8 == 0 && !strcmp(argv[1], "decode")) {
    const int sub_bytes = atoi(argv[2]), grid_rounds = atoi(argv[3]);
    if (!valid_sub_bytes(sub_bytes) || grid_rounds < 0 || grid_rounds > kMaxGridRounds) {
      fprintf(stderr, "sub_bytes a multiple of 16 in 32..65536 and grid_rounds in 0..16 required\n");
      return 2;
    }
    for (char** a = argv + 4; a < argv + argc; a += 8) {  // one line of output per file: its status and info words
      const int h = atoi(a[2]), w = atoi(a[3]), sampling = atoi(a[4]), ncomp = atoi(a[5]), nsegs = atoi(a[6]);
      if (!valid_picture(h, w, sampling, ncomp) || !valid_segments(geometry(h, w, sampling, ncomp), nsegs)) {
        fprintf(stderr, "h, w in 1..65535, sampling 0..2, ncomps 1 or 3 and nsegs = ceil(mcus / Ri) required\n");
        return 2;
      }
      std::vector<uint8_t> file, plan, out;
      if (!read_file(a[0], &file) || !read_file(a[1], &plan) || int64_t(plan.size()) != plan_bytes(nsegs)) {
        fprintf(stderr, "cannot read %s or its plan of %d segments\n", a[0], nsegs);
        return 2;
      }
      int info = 0;
      const int status = decode_file(file, plan, h, w, sampling, ncomp, nsegs, sub_bytes, grid_rounds, &out, &info);
      FILE* f = fopen(a[7], "wb");
      if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) {
        fprintf(stderr, "cannot write %s\n", a[7]);
        return 2;
      }
      fclose(f);
      printf("%d %d\n", status, info);
    }
    return 0;
  }
  fprintf(stderr, "usage: jpeg_sync_rehearse selftest | decode SUB_BYTES GRID_ROUNDS (in.jpg in.plan H W SAMPLING NCOMPS NSEGS out.rgb)...\n");
  return 2;
}
