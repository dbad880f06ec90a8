// curves_run.h -- the step loop of the fused inference passes for ANY cfg.curve_steps L in [1, 16], shared by
// chain_fused_curves.hip and chain_fused_curves_codes.hip: the per-wave curve table for a
// runtime L and chain_fused_run for parameter rows of EXPO_MAX_PARAMS_CURVES.  Include it after chain_fused.hip
// (EXPO_CHAIN_FUSED_TEMPLATES_ONLY), whose chain_step, NoTap and PixTraits it uses; how the parameters and the table
// are held is described at the head of chain_fused_curves.hip.
#pragma once

namespace expo {

namespace {

constexpr int kCurvesMaxL = EXPO_CURVE_MAX_STEPS;
constexpr int kCurvesTabEntries = 3 * (kCurvesMaxL + 1) + 1;  // 51, padded to an even count
static_assert(EXPO_MAX_PARAMS_CURVES == 3 * kCurvesMaxL && EXPO_MAX_PARAMS_CURVES <= 64,
              "a row is three curves of kCurvesMaxL knots, one lane per entry");

// curve_lut_build for a runtime L: lane l < NC * L holds k[l] in klane (other lanes: anything -- masked to 0 here, an
// entry its filter does not use never enters arithmetic).  All 64 lanes of the wave must be active.
template <int NC>
__device__ __forceinline__ void curves_lut_build(float klane, int L, float2_lut* tab) {
  const int lane = threadIdx.x & 63;
  const int c = (lane >= L ? 1 : 0) + (lane >= 2 * L ? 1 : 0);  // the curve of this lane, j its segment
  const int j = lane - c * L;
  const bool mine = lane < NC * L;
  const float k = mine ? klane : 0.0f;
  float incl = k;  // inclusive scan inside each run of L lanes
#pragma unroll
  for (int d = 1; d < kCurvesMaxL; d <<= 1) {
    const float t = __shfl_up(incl, d);
    if (j >= d) incl += t;
  }
  const float inv_s = 1.0f / (__shfl(incl, c * L + L - 1) + 1e-30f);
  if (mine) {
    float2_lut e;
    e.x = float(L) * inv_s * k;
    e.y = inv_s * ((incl - k) - float(j) * k);
    const int slot = c * (L + 1) + j;
    tab[slot] = e;
    if (j == L - 1) tab[slot + 1] = e;
  }
  __builtin_amdgcn_wave_barrier();
}

template <int NC, int NPIX>
__device__ __forceinline__ void curves_lut_map(const float* in, float* out, int L, const float2_lut* tab) {
  const float lf = float(L);
#pragma unroll
  for (int k = 0; k < NPIX; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float xc = clamp01x(in[3 * k + c], 0.0f, 1.0f);
      const int seg = int(xc * lf);  // 0..L; entry L == entry L-1
      const float2_lut e = tab[(NC == 1 ? 0 : c * (L + 1)) + seg];
      out[3 * k + c] = fmaf(xc, e.x, e.y);
    }
  }
}

// chain_fused_run for rows of EXPO_MAX_PARAMS_CURVES: prn[steps][48], L the curve steps (uniform), `tab` this wave's
// kCurvesTabEntries of LDS, `plane` the row entry this lane mirrors.  The loop, the two alternating pixel arrays, the
// fetch one step ahead and the identity half-trip are chain_fused_run's; see there.
template <typename T, class Tap = NoTap>
__device__ inline void chain_fused_curves_run(const int32_t* idn, const float* prn, int steps, int L, float2_lut* tab,
                                              int plane, float* v, const Tap& tap = Tap()) {
  constexpr int PPL = PixTraits<T>::PPL;
  auto apply = [&](int id, const float* prm, float klane, const float* in, float* out) {
    if (id == 4) {
      curves_lut_build<1>(klane, L, tab);
      curves_lut_map<1, PPL>(in, out, L, tab);
      __builtin_amdgcn_wave_barrier();  // the next curve step of this wave rewrites the table
    } else if (id == 7) {
      curves_lut_build<3>(klane, L, tab);
      curves_lut_map<3, PPL>(in, out, L, tab);
      __builtin_amdgcn_wave_barrier();
    } else {
      chain_step<T>(id, prm, klane, tab, in, out);  // (its own cases 4 and 7 are never reached)
    }
  };
  float pa[3], pb[3];
  float ka = 0.f, kb = 0.f;
  int ia = 0, ib = 0;
  auto fetch = [&](int st, float* p, float& kl, int& id) {
    const bool live = st < steps;
    const int sn = live ? st : steps - 1;  // (past the end: any valid row)
    id = live ? idn[sn] : 0;
    kl = prn[sn * EXPO_MAX_PARAMS_CURVES + plane];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = prn[sn * EXPO_MAX_PARAMS_CURVES + j];
    if (!live) p[0] = 0.0f;
  };
  if (steps <= 0) return;
  float a[PPL * 3], w[PPL * 3];  // (locals, copied in and out: see chain_fused_run)
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

}  // namespace

}  // namespace expo
