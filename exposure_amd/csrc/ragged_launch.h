// ragged_launch.h -- the host side that the fused ragged inference passes share (chain_fused.hip, chain_fused_curves.hip,
// chain_fused_codes.hip, chain_fused_curves_codes.hip): the argument checks of a call, the dtype x
// tap-format dispatch and the split of a call into launches with their by-value tables.  Host code only, and none of it
// calls the HIP runtime: tools/ragged_rehearse.cpp drives it without a device.
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "host_common.h"

namespace expo {

constexpr int kRaggedMaxImages = 64;  // images of one launch: its table travels by value in the kernel arguments
constexpr int kTapNone = -1;          // FMT of a kernel without taps (an EXPO_TAP_* format otherwise)

inline int check_taps(int steps, uint64_t tap_mask, int tap_format) {
  if (tap_format != EXPO_TAP_STORAGE && tap_format != EXPO_TAP_U8 && tap_format != EXPO_TAP_U16)
    return fail(EXPO_E_BADARG, "tap_format must be EXPO_TAP_STORAGE, EXPO_TAP_U8 or EXPO_TAP_U16");
  if (steps < 64 && (tap_mask >> steps) != 0) return fail(EXPO_E_BADARG, "tap_mask has a bit >= steps");
  return EXPO_OK;
}

struct NoExtraCheck { int operator()(int) const { return EXPO_OK; } };

// The checks of a ragged pass, all of them before its first launch: the scalars, then the pointers.  EXPO_OK with
// *go = false: nothing to do (n == 0, which is looked at only after every scalar has passed).
//   in          the images' inputs (xs, or codes)
//   ys_optional ys may be NULL when there are taps to write (every pass but expo_chain_fused_fwd_ragged, which passes
//               tap_mask 0 and EXPO_TAP_STORAGE)
//   arrays_ok   the pass's other arrays that any image needs are there (tables)
//   steps_ok    the arrays that steps > 0 reads are there (filter_ids, params, mask_params)
//   extra       a pass's further pointer-stage checks: extra(-1) once the arrays are known to be there, extra(i) after
//               image i's size check (the codes passes: tables' alignment, the bytes of an image's codes)
// A pass's own scalar checks (curve_steps; channels, code_bits, table_stride) go in front of this call.
template <class Extra = NoExtraCheck>
int ragged_check_args(int steps, const void* const* in, void* const* ys, bool ys_optional, const int* hs, const int* ws,
                      int n, int dtype, uint64_t tap_mask, int tap_format, void* const* taps, bool arrays_ok,
                      bool steps_ok, bool* go, const Extra& extra = Extra()) {
  *go = false;
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (dtype != EXPO_F16 && dtype != EXPO_F32) return fail(EXPO_E_BADDTYPE, "dtype must be EXPO_F16 or EXPO_F32");
  if (steps < 0 || steps > 64) return fail(EXPO_E_BADARG, "steps must be in [0, 64]");
  if (ys_optional) {
    if (int rc = check_taps(steps, tap_mask, tap_format)) return rc;
    if (!ys && !tap_mask) return fail(EXPO_E_BADARG, "nothing to write (ys NULL and tap_mask 0)");
  }
  if (n == 0) return EXPO_OK;
  if (!in || !hs || !ws || (!ys_optional && !ys) || (tap_mask && !taps) || !arrays_ok || (steps > 0 && !steps_ok))
    return fail(EXPO_E_BADARG, "null pointer");
  if (int rc = extra(-1)) return rc;
  for (int i = 0; i < n; ++i) {
    if (int rc = check_common(1, hs[i], ws[i], dtype)) return rc;
    if (int rc = extra(i)) return rc;
    if (!in[i] || (ys && !ys[i])) return fail(EXPO_E_BADARG, "null image pointer");
    if (tap_mask && !taps[i]) return fail(EXPO_E_BADARG, "null tap pointer");
  }
  *go = true;
  return EXPO_OK;
}

// f(T(), std::integral_constant<int, FMT>()) for the call's storage dtype T (half_t | float) and FMT: kTapNone without
// taps (tap_mask == 0), the EXPO_TAP_* format otherwise.  dtype and tap_format have been checked.
template <class F>
int dispatch_dtype_tap(int dtype, uint64_t tap_mask, int tap_format, const F& f) {
  auto fmt = [&](auto t) {
    if (!tap_mask) return f(t, std::integral_constant<int, kTapNone>());
    if (tap_format == EXPO_TAP_U8) return f(t, std::integral_constant<int, EXPO_TAP_U8>());
    if (tap_format == EXPO_TAP_U16) return f(t, std::integral_constant<int, EXPO_TAP_U16>());
    return f(t, std::integral_constant<int, EXPO_TAP_STORAGE>());
  };
  return dtype == EXPO_F16 ? fmt(half_t()) : fmt(float());
}

// the members every table shares -- first, n, vec -- sit in the table itself or in its member t (RaggedTapTable)
template <class Tab, class = void>
struct RaggedCore { static Tab& of(Tab& tab) { return tab; } };
template <class Tab>
struct RaggedCore<Tab, std::void_t<decltype(std::declval<Tab&>().t)>> {
  static auto& of(Tab& tab) { return tab.t; }
};

inline uintptr_t ragged_addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// The launches of one call whose arguments have been checked: at most kRaggedMaxImages images each, in order.
//   fill(tab, j, i)  writes the pointers and sizes of image i into slot j of the zero-initialised table and returns the
//                    OR of the addresses that the vector path needs 4-byte aligned (ragged_addr; NULL counts as aligned)
//   launch(io, any_slow, grid, base, tab)  enqueues images [base, base + tab's n) and returns an EXPO_* code.  io is
//                    IoStream() when the whole call holds at least stream_min_bytes() bytes in the storage dtype (what
//                    one tensor of the same pixels would choose), IoCached() otherwise; any_slow is std::true_type()
//                    when some image of the launch takes the element-wise path; the launch's ids / params / ... rows
//                    start `base` images into the call's.
// The helper sets first[] (image j's first block; first[n] = the grid: one chunk per wave, ceil(groups / kThreads)
// blocks per image), n, and vec: bit j says image j has whole 12-byte vectors (hw % PPV == 0) and aligned addresses.
// The grid fits an int with room to spare: check_common holds one image under 2^31 bytes, so an image has at most
// 2^31 / 6 pixels (fp16; fp32: 2^31 / 12), 2^31 / 48 < 44 739 243 groups of PPL pixels and, at kThreads groups a block,
// under 174 763 blocks; 64 images stay below 11.2 million.  The check below is therefore dead, and stays as the one
// place that says so.
template <typename T, class Tab, class Fill, class Launch>
int ragged_launches(const int* hs, const int* ws, int n, const Fill& fill, const Launch& launch) {
  constexpr int PPL = PixTraits<T>::PPL;
  long bytes = 0;
  for (int i = 0; i < n; ++i) bytes += long(hs[i]) * ws[i] * 3L * long(sizeof(T));
  const bool stream = bytes >= stream_min_bytes();
  for (int base = 0; base < n; base += kRaggedMaxImages) {
    Tab tab = {};
    auto& core = RaggedCore<Tab>::of(tab);
    core.n = n - base < kRaggedMaxImages ? n - base : kRaggedMaxImages;
    long blocks = 0;
    bool any_slow = false;
    for (int j = 0; j < core.n; ++j) {
      const int hw = hs[base + j] * ws[base + j];
      core.first[j] = int(blocks);
      blocks += ((hw + PPL - 1) / PPL + kThreads - 1) / kThreads;
      const uintptr_t a = fill(tab, j, base + j);
      if (hw % VecTraits<T>::PPV == 0 && (a & 3) == 0) core.vec |= uint64_t(1) << j;
      else any_slow = true;
    }
    if (blocks > 0x7fffffffL) return fail(EXPO_E_BADARG, "too many blocks in one launch");
    core.first[core.n] = int(blocks);
    const dim3 grid(static_cast<unsigned>(blocks));
    const int rc = stream ? (any_slow ? launch(IoStream(), std::true_type(), grid, base, tab)
                                      : launch(IoStream(), std::false_type(), grid, base, tab))
                          : (any_slow ? launch(IoCached(), std::true_type(), grid, base, tab)
                                      : launch(IoCached(), std::false_type(), grid, base, tab));
    if (rc != EXPO_OK) return rc;
  }
  return EXPO_OK;
}

}  // namespace expo
