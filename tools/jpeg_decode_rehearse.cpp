// jpeg_decode_rehearse.cpp -- the integer routines of exposure_amd/csrc/jpeg_decode.h on the host, without a GPU: a
// serial walk through the phases of csrc/jpeg_decode.hip's three kernels, lane by lane and thread by thread, over whole
// files.  Its own main; build it with the sanitizers and run it directly:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/jpeg_decode_rehearse.cpp -o jpeg_decode_rehearse
//   jpeg_decode_rehearse selftest
//   jpeg_decode_rehearse decode in.jpg in.plan H W SAMPLING NCOMPS NSEGS out.rgb [the same eight for further files ...]
// in.plan is the blob of exposure_amd/jpeg_decode.py's parse.  The file, the plan, the workspace and the output live in
// heap buffers of exactly the sizes the ABI reports, the workspace full of a sentinel, so a read or write that the
// device would have to clamp shows under AddressSanitizer.  Prints the status word; out.rgb is H*W*3 bytes
// (tests/test_jpeg_decode_host.py compares it with the NumPy restatement).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../exposure_amd/csrc/jpeg_decode.h"

using namespace expo::jpegdec;

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

// the three launches on one picture; every buffer of exactly its size, on the heap
int decode_file(const std::vector<uint8_t>& file, const std::vector<uint8_t>& plan, int h, int w, int sampling, int ncomp,
                int nsegs, std::vector<uint8_t>* rgb_out) {
  const Geometry g = geometry(h, w, sampling, ncomp);
  const Layout lay = layout(0, g);
  CHECK(int64_t(plan.size()) == plan_bytes(nsegs) && valid_segments(g, nsegs));
  // the workspace is allocated as 16-byte vectors (the kernel's stores are that wide), full of a sentinel
  std::vector<Vec16> wsv(size_t(lay.end + 15) / 16, Vec16{{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}});
  CHECK(lay.end % 16 == 0);
  uint8_t* ws = reinterpret_cast<uint8_t*>(wsv.data());
  // the plan at a 16-byte aligned address of its own, the file at an odd one
  std::vector<Vec16> planv(plan.size() / 16);
  memcpy(planv.data(), plan.data(), plan.size());
  const uint8_t* planp = reinterpret_cast<const uint8_t*>(planv.data());
  // jpeg_entropy_kernel: a lane per segment, its own slot
  int status = 0;
  for (int k = 0; k < nsegs; ++k) {
    Vec16 slot[8];
    status |= decode_segment(file.data(), int64_t(file.size()), planp, g, k, slot, reinterpret_cast<Vec16*>(ws + lay.coef), Vec16{{0, 0, 0, 0}});
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
        CHECK(x0 + 8 <= plane_stride(g, comp));  // the kernel's 8-byte store stays inside the row
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
  // geometry: MCUs, blocks, planes and the workspace of the three samplings and grey
  Geometry g = geometry(17, 33, 2, 3);
  CHECK(g.mx == 3 && g.my == 2 && g.bpm == 6 && blocks(g) == 36 && plane_h(g, 1) == 9 && plane_w(g, 1) == 17 && plane_stride(g, 1) == 24);
  g = geometry(17, 33, 1, 3);
  CHECK(g.mx == 3 && g.my == 3 && g.bpm == 4 && plane_h(g, 2) == 17 && plane_w(g, 2) == 17);
  g = geometry(1, 1, 0, 1);
  CHECK(blocks(g) == 1 && layout(0, g).end == 128 + 16);
  g = geometry(65535, 65535, 0, 3);
  CHECK(mcus(g) == int64_t(8192) * 8192 && layout(0, g).end > int64_t(65535) * 65535 * 3);
  CHECK(valid_segments(geometry(8, 1040, 0, 3), 130) && valid_segments(geometry(64, 64, 0, 3), 1) && !valid_segments(geometry(64, 64, 0, 3), 65) &&
        !valid_segments(geometry(64, 64, 0, 3), 0) && !valid_segments(geometry(80, 80, 0, 3), 60));  // 100 MCUs: Ri 2 gives 50, Ri 1 gives 100
  CHECK(plan_bytes(1) == 1808 + 16 && plan_bytes(2) == 1808 + 16 && plan_bytes(3) == 1808 + 32);
  // block places: 4:2:0's four Y blocks of MCU 4 of a 3-wide picture
  g = geometry(32, 48, 2, 3);
  int br, bc;
  block_place(g, 4, 3, &br, &bc);
  CHECK(br == 3 && bc == 3 && block_component(g, 3) == 0 && block_component(g, 4) == 1 && block_component(g, 5) == 2);
  block_place(g, 4, 5, &br, &bc);
  CHECK(br == 1 && bc == 1);
  // the 8-point pass: a lone DC gives a flat block, (dc << 13 + 1024) >> 11 = 4 dc, then (4 dc << 13 + 2^17) >> 18
  int32_t in[8] = {100, 0, 0, 0, 0, 0, 0, 0}, o[8];
  idct_pass(in, 11, o);
  for (int e = 0; e < 8; ++e) CHECK(o[e] == 400);
  in[0] = 400;
  idct_pass(in, 18, o);
  for (int e = 0; e < 8; ++e) CHECK(o[e] == 13);  // (400 * 8192 + 131072) >> 18 = 13
  // the largest inputs of the section's bound leave int32 alone (the arithmetic is unsigned, so the sanitizer is silent
  // either way; the restatement asserts the bound)
  for (int e = 0; e < 8; ++e) in[e] = e & 1 ? -32767 : 32767;
  idct_pass(in, 11, o);
  // upsampling taps and colour at their extremes
  CHECK(up2x1_even(0, 255) == 191 && up2x1_odd(255, 255) == 255 && up2x2_even(up2x2_row(255, 255), up2x2_row(255, 255)) == 255 &&
        up2x2_odd(0, 0) == 0);
  uint8_t px[3];
  rgb(255, 255, 255, px);
  CHECK(px[0] == 255 && px[2] == 255);
  rgb(0, 0, 0, px);
  CHECK(px[0] == 0 && px[2] == 0 && px[1] == 135);
  // the bit reader: FF 00 is one FF; a segment's end inside the file; ranges the file does not have are clamped
  const uint8_t bytes[] = {0xFF, 0x00, 0x12, 0xFF};
  BitReader r = open_bits(bytes, 4, 0, 4);
  fill(r);
  CHECK(r.nbits == 24 && (r.acc >> 40) == 0xFF12FFu);
  r = open_bits(bytes, 4, -5, 99);
  CHECK(r.pos == 0 && r.end == 4);
  r = open_bits(bytes, 4, 7, 2);
  CHECK(r.pos == 4 && r.end == 4);
  printf("jpeg_decode_rehearse selftest: ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc >= 10 && (argc - 2) % 8 == 0 && !strcmp(argv[1], "decode")) {
    for (char** a = argv + 2; a < argv + argc; a += 8) {  // one line of output per file: its status word
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
      const int status = decode_file(file, plan, h, w, sampling, ncomp, nsegs, &out);
      FILE* f = fopen(a[7], "wb");
      if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) {
        fprintf(stderr, "cannot write %s\n", a[7]);
        return 2;
      }
      fclose(f);
      printf("%d\n", status);
    }
    return 0;
  }
  fprintf(stderr, "usage: jpeg_decode_rehearse selftest | decode (in.jpg in.plan H W SAMPLING NCOMPS NSEGS out.rgb)...\n");
  return 2;
}
