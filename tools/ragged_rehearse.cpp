// ragged_rehearse.cpp -- the host-side launch scaffold of the fused ragged inference passes
// (exposure_amd/csrc/ragged_launch.h) without a GPU: ragged_launches with the units' own table types
// and fills and a `launch` that prints what it was handed instead of enqueueing a kernel.  Host code only, built with
// the sanitizers; no HIP runtime function is called, the addresses are numbers that nothing dereferences.
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all tools/ragged_rehearse.cpp -o ragged_rehearse
//   ragged_rehearse TABLE DTYPE FMT YS < images
//     TABLE  ragged | taps | masked | codes      DTYPE  f16 | f32
//     FMT    -1 (no taps) | an EXPO_TAP_* value  YS     0: the call's ys is NULL
//     images one line per image: h w in y taps (the three addresses in hex)
// One line per launch (stream, any_slow, grid, base, n, first[0..n], vec), then one per slot with what `fill` stored.
// tests/test_ragged_launch_host.py compares the output with its own restatement of the rule.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#define EXPO_CHAIN_FUSED_TEMPLATES_ONLY
#include "../exposure_amd/csrc/chain_fused.hip"
#include "../exposure_amd/csrc/codes_image.h"

namespace expo {
thread_local std::string g_err;
}

using namespace expo;

namespace {

uintptr_t num(const void* p) { return reinterpret_cast<uintptr_t>(p); }

template <typename T>
void print_slot(const RaggedTable<T>& t, int j) {
  printf("  slot %d x=0x%" PRIxPTR " y=0x%" PRIxPTR " hw=%d\n", j, num(t.x[j]), num(t.y[j]), t.hw[j]);
}
template <typename T>
void print_slot(const RaggedTapTable<T>& t, int j) {
  printf("  slot %d x=0x%" PRIxPTR " y=0x%" PRIxPTR " hw=%d taps=0x%" PRIxPTR "\n", j, num(t.t.x[j]), num(t.t.y[j]),
         t.t.hw[j], num(t.taps[j]));
}
template <typename T>
void print_slot(const MaskedRaggedTable<T>& t, int j) {
  printf("  slot %d x=0x%" PRIxPTR " y=0x%" PRIxPTR " h=%d w=%d taps=0x%" PRIxPTR "\n", j, num(t.x[j]), num(t.y[j]),
         t.h[j], t.w[j], num(t.taps[j]));
}
template <typename T>
void print_slot(const CodesTable<T>& t, int j) {
  printf("  slot %d codes=0x%" PRIxPTR " y=0x%" PRIxPTR " hw=%d taps=0x%" PRIxPTR "\n", j, num(t.codes[j]), num(t.y[j]),
         t.hw[j], num(t.taps[j]));
}

struct Call {
  std::vector<int> hs, ws;
  std::vector<const void*> in;
  std::vector<void*> ys, taps;
  bool have_ys;
};

template <typename T, class Tab, class Fill>
int rehearse(const Call& c, const Fill& fill) {
  return ragged_launches<T, Tab>(
      c.hs.data(), c.ws.data(), int(c.hs.size()), fill,
      [&](auto io, auto any_slow, dim3 grid, int base, const Tab& tab) {
        const auto& core = RaggedCore<const Tab>::of(tab);
        printf("launch stream=%d any_slow=%d grid=%u,%u,%u base=%d n=%d first=",
               int(std::is_same<decltype(io), IoStream>::value), int(decltype(any_slow)::value), grid.x, grid.y, grid.z,
               base, core.n);
        for (int j = 0; j <= core.n; ++j) printf("%s%d", j ? "," : "", core.first[j]);
        printf(" vec=0x%" PRIx64 "\n", core.vec);
        for (int j = 0; j < core.n; ++j) print_slot(tab, j);
        return EXPO_OK;
      });
}

template <typename T, int FMT>
int rehearse_table(const char* table, const Call& c) {
  void* const* ys = c.have_ys ? c.ys.data() : nullptr;
  const int *hs = c.hs.data(), *ws = c.ws.data();
  if (!strcmp(table, "masked"))
    return rehearse<T, MaskedRaggedTable<T>>(c, masked_fill<T, FMT>(c.in.data(), ys, hs, ws, c.taps.data()));
  if (!strcmp(table, "codes"))
    return rehearse<T, CodesTable<T>>(c, codes_fill<T, FMT>(c.in.data(), ys, hs, ws, c.taps.data()));
  if constexpr (FMT == kTapNone) {
    if (!strcmp(table, "ragged")) return rehearse<T, RaggedTable<T>>(c, ragged_fill<T>(c.in.data(), ys, hs, ws));
  } else {
    if (!strcmp(table, "taps"))
      return rehearse<T, RaggedTapTable<T>>(c, ragged_taps_fill<T, FMT>(c.in.data(), ys, hs, ws, c.taps.data()));
  }
  return fail(EXPO_E_BADARG, "no such table for this FMT");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) return fprintf(stderr, "usage: ragged_rehearse TABLE DTYPE FMT YS < images\n"), 2;
  Call c;
  c.have_ys = atoi(argv[4]) != 0;
  int h, w;
  uint64_t in, y, taps;
  while (scanf("%d %d %" SCNx64 " %" SCNx64 " %" SCNx64, &h, &w, &in, &y, &taps) == 5) {
    c.hs.push_back(h);
    c.ws.push_back(w);
    c.in.push_back(reinterpret_cast<const void*>(uintptr_t(in)));
    c.ys.push_back(reinterpret_cast<void*>(uintptr_t(y)));
    c.taps.push_back(reinterpret_cast<void*>(uintptr_t(taps)));
  }
  const int dtype = !strcmp(argv[2], "f16") ? EXPO_F16 : EXPO_F32;
  const int fmt = atoi(argv[3]);
  const int rc = dispatch_dtype_tap(dtype, fmt != kTapNone, fmt, [&](auto t, auto f) {
    return rehearse_table<decltype(t), decltype(f)::value>(argv[1], c);
  });
  if (rc != EXPO_OK) return fprintf(stderr, "error %d: %s\n", rc, g_err.c_str()), 1;
  return 0;
}
