// dispatch_curves.hip -- the agent's one-hot step (agent.py:58-77, 119-125) per image for ANY cfg.curve_steps, forward
// and backward, with the head regressors in front of it.
//
// expo_filter_dispatch_fwd / _bwd (exposure_hip.hip) are instantiated for 8-step curves and 24-float parameter rows.
// Here the rows are EXPO_MAX_PARAMS_CURVES wide and ids 4 (Tone) / 7 (Color) are the curves of expo_curve_fwd / _bwd
// with L = curve_steps (curve_segments.h); every other id runs the SAME body as the tuned dispatch (stream_bodies.h,
// same compiler flags, same launch geometry), so its image and image gradient have the same bits.
//
//   forward    one launch: block-uniform switch on ids[n]; light filters -> fwd_body, curves -> the segment form,
//              -1 -> zero fill; with `penalty` one record per block and the finish launch
//   backward   two streaming launches, as the tuned dispatch splits them for register budget:
//                light   dispatch_curves_bwd_light_kernel: bwd_body of ids 0-3, 5, 6, 8 and the zero fill of -1; blocks of
//                        a curve image exit at once; no dynamic LDS
//                curves  dispatch_curves_bwd_curve_kernel: ids 4 / 7 with PRIVATE LDS accumulator columns per thread
//                        (3 (2 L + 1) x 257 floats, sized from L at launch: 99.7 KB at L = 16, 9.3 KB at L = 1); blocks of
//                        any other image exit at once; cg_blocks(h w) blocks per image (two at 64x64)
//              plus ONE finish launch that adds an image's block records in a fixed order and writes its whole
//              48-float dparams row: no float atomics, no zero fill, bit-reproducible.
// Workspace: [light records n x bx x kWsSlots][curve records n x cg_blocks x 3 (2 L + 1)][one image tensor of scratch].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exposure_hip.h"
#include "filter_math.h"
#include "pixel_io.h"
#include "kernel_common.h"
#include "host_common.h"
#include "stream_bodies.h"
#include "curve_segments.h"

namespace expo {

static_assert(kCgThreads == kThreads, "the curve bodies run in the streaming kernels' blocks");
constexpr int kDcRow = EXPO_MAX_PARAMS_CURVES;
static_assert(kDcRow >= 3 * kCgMaxSteps && kDcRow >= EXPO_MAX_PARAMS, "a row holds a Color filter at the largest step count");

// ------------------------------------------------------------------------------------------ forward
template <typename T, bool PEN>
__device__ __forceinline__ void dc_curve_fwd(const T* __restrict__ xi, T* __restrict__ yi, const float* __restrict__ prm,
                                             float* __restrict__ rec, int hw, int curves, int L) {
  __shared__ CgCurve cv[3];
  cg_stage(prm, curves, L, cv);
  float pen = 0.f;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < hw; p += gridDim.x * kThreads) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int j;
      float o;
      const float v = cg_eval(cv[curves == 1 ? 0 : c], L, cg_load(xi, size_t(p) * 3 + c), &j, &o);
      cg_store(yi, size_t(p) * 3 + c, v);
      if constexpr (PEN) {
        const float e = fmaxf(v - 1.0f, 0.0f);
        pen = fmaf(e, e, pen);
      }
    }
  }
  if constexpr (PEN) {
    float a[1] = {pen};
    block_reduce_record<1>(a, rec);
  }
}

template <typename T, bool VEC, bool PEN, class IO>
__global__ __launch_bounds__(kThreads) void dispatch_curves_fwd_kernel(const int32_t* __restrict__ ids,
                                                                       const T* __restrict__ x, T* __restrict__ y,
                                                                       const float* __restrict__ params,
                                                                       float* __restrict__ records, int hw, int groups,
                                                                       int L) {
  const int n = blockIdx.y;
  const size_t off = size_t(n) * hw * 3;
  const float* prm = params + size_t(n) * kDcRow;
  float* rec = PEN ? records + size_t(n) * gridDim.x * kWsSlots : nullptr;
  const int id = ids[n];  // block-uniform
#define EXPO_CASE(ID, F) \
  case ID: fwd_body<F, T, VEC, PEN, IO>(x + off, y + off, prm, rec, hw, groups); break;
  switch (id) {
    EXPO_CASE(0, ExposureF)
    EXPO_CASE(1, GammaF)
    EXPO_CASE(2, WhiteBalanceF)
    EXPO_CASE(3, SatPlusF)
    EXPO_CASE(5, ContrastF)
    EXPO_CASE(6, WnbF)
    EXPO_CASE(8, LevelF)
    case 4: dc_curve_fwd<T, PEN>(x + off, y + off, prm, rec, hw, 1, L); break;
    case 7: dc_curve_fwd<T, PEN>(x + off, y + off, prm, rec, hw, 3, L); break;
    default:  // id -1 (and anything outside [0, 8]): y = 0, the finish launch writes penalty = 0 without reading records
      zero_image<T, VEC, IO>(y + off, hw, groups);
      break;
  }
#undef EXPO_CASE
}

// ------------------------------------------------------------------------------------------ backward
// (always the dx-storing instantiation of the bodies: compiled without the store, the Contrast, WNB and Level bodies round
// their parameter gradients differently -- in expo_filter_dispatch_bwd too -- and dparams must not depend on whether the
// caller wants dx; a caller without dx gets it written to a scratch slice of the workspace.  Likewise always the
// instantiation with the fused penalty: a caller without dpenalty runs it with a zero scale -- the same bits as a
// dpenalty of zeros, where the instantiation without the penalty rounds differently)
template <typename T, bool VEC, int MODE>
__global__ __launch_bounds__(kThreads) void dispatch_curves_bwd_light_kernel(const int32_t* __restrict__ ids,
                                                                             const T* __restrict__ x,
                                                                             const T* __restrict__ dy, T* __restrict__ dx,
                                                                             const float* __restrict__ params,
                                                                             float* __restrict__ records,
                                                                             const float* __restrict__ dpenalty, int hw,
                                                                             int groups, float inv_count) {
  const int n = blockIdx.y;
  const int id = ids[n];
  if (id == 4 || id == 7) return;  // the curve launch's image
  const size_t off = size_t(n) * hw * 3;
  const float* prm = params + size_t(n) * kDcRow;
  float* rec = records + size_t(n) * gridDim.x * kWsSlots;
  const float ps = dpenalty ? 2.0f * inv_count * dpenalty[n] : 0.f;
  T* dxi = dx + off;
#define EXPO_CASE(ID, F) \
  case ID: bwd_body<F, T, VEC, true, true, MODE, IoCached>(x + off, dy + off, dxi, prm, rec, hw, groups, ps); break;
  switch (id) {
    EXPO_CASE(0, ExposureF)
    EXPO_CASE(1, GammaF)
    EXPO_CASE(2, WhiteBalanceF)
    EXPO_CASE(3, SatPlusF)
    EXPO_CASE(5, ContrastF)
    EXPO_CASE(6, WnbF)
    EXPO_CASE(8, LevelF)
    default:  // id -1 selects nothing: dx = 0 (the finish launch writes the all-zero dparams row)
      zero_image<T, VEC, IoCached>(dxi, hw, groups);
      break;
  }
#undef EXPO_CASE
}

// record layout per block: [curve][H_0..H_{L-1} | R_0..R_{L-1} | B], 3 (2 L + 1) floats reserved whatever the id
// (curve_generic.hip has the derivation); with the fused penalty dy <- dy + ps max(y - 1, 0) first
template <typename T, bool HAS_DX>
__global__ __launch_bounds__(kThreads) void dispatch_curves_bwd_curve_kernel(const int32_t* __restrict__ ids,
                                                                             const T* __restrict__ x,
                                                                             const T* __restrict__ dy, T* __restrict__ dx,
                                                                             const float* __restrict__ params,
                                                                             float* __restrict__ records,
                                                                             const float* __restrict__ dpenalty, int hw,
                                                                             int L, float inv_count) {
  const int n = blockIdx.y;
  const int id = ids[n];
  if (id != 4 && id != 7) return;  // the light launch's image
  __shared__ CgCurve cv[3];
  extern __shared__ float acc[];  // 3 (2 L + 1) columns of kCgPad floats
  const int curves = id == 4 ? 1 : 3;
  cg_stage(params + size_t(n) * kDcRow, curves, L, cv);
  const int per_curve = 2 * L + 1, slots = curves * per_curve;
  for (int s = 0; s < slots; ++s) acc[s * kCgPad + threadIdx.x] = 0.f;
  const float ps = dpenalty ? 2.0f * inv_count * dpenalty[n] : 0.f;
  const size_t base = size_t(n) * hw * 3;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < hw; p += gridDim.x * kThreads) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cc = curves == 1 ? 0 : c;
      const CgCurve& cu = cv[cc];
      const float xv = cg_load(x, base + size_t(p) * 3 + c);
      float g = cg_load(dy, base + size_t(p) * 3 + c);
      int j;
      float o;
      const float yv = cg_eval(cu, L, xv, &j, &o);
      g = fmaf(fmaxf(yv - 1.0f, 0.0f), ps, g);
      float* a = acc + cc * per_curve * kCgPad + threadIdx.x;
      a[j * kCgPad] += g;
      a[(L + j) * kCgPad] = fmaf(g, o, a[(L + j) * kCgPad]);
      a[2 * L * kCgPad] = fmaf(g, yv, a[2 * L * kCgPad]);
      if constexpr (HAS_DX) {
        // tf.clip_by_value passes the gradient on 0 <= x - i/L <= 1/L: segment floor(u), plus segment u - 1 when
        // u = L x is an integer >= 1; nothing outside [0, 1]; -0.0 passes like +0.0; NaN gives 0
        const float u = xv * float(L);
        float sl = 0.f;
        if (u >= 0.0f && u <= float(L)) {
          const float jf = floorf(u);
          const int ju = int(jf);
          sl = ju < L ? cu.k[ju] : 0.0f;
          if (jf == u && ju >= 1) sl += cu.k[ju - 1];
        }
        cg_store(dx, base + size_t(p) * 3 + c, g * sl * cu.scale);
      }
    }
  }
  __syncthreads();
  // one thread per slot adds the 256 private columns in a fixed order
  float* rec = records + (size_t(n) * gridDim.x + blockIdx.x) * size_t(3 * per_curve);
  for (int s = threadIdx.x; s < slots; s += kThreads) {
    float t = 0.f;
    for (int i = 0; i < kThreads; ++i) t += acc[s * kCgPad + i];
    rec[s] = t;
  }
}

// One block per image writes its whole dparams row.  Light filters: the summation order of finish_kernel
// (exposure_hip.hip), so their parameter gradients have the tuned dispatch's bits; curves: curve_finish_kernel's.
constexpr int kDcFinishThreads = 256;
template <class F>
__device__ __forceinline__ void dc_finish_light(const float* prm, const float* tot, float* out, int lane) {
  if (lane < kDcRow) out[lane] = lane < F::NP ? F::finish_one(prm, tot, lane) : 0.0f;
}
__global__ __launch_bounds__(kDcFinishThreads) void dispatch_curves_finish_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ params, float* __restrict__ dparams,
    const float* __restrict__ light_records, int light_bx, const float* __restrict__ curve_records, int curve_bx, int L) {
  const int n = blockIdx.x, lane = threadIdx.x & 63;
  const int id = ids[n];
  const float* prm = params + size_t(n) * kDcRow;
  float* out = dparams + size_t(n) * kDcRow;
  if (id < 0 || id >= EXPO_NUM_FILTERS) {  // nothing selected: the image wrote no records
    if (threadIdx.x < kDcRow) out[threadIdx.x] = 0.0f;
    return;
  }
  if (id == 4 || id == 7) {
    const int curves = id == 4 ? 1 : 3, per_curve = 2 * L + 1, slots = curves * per_curve;
    __shared__ float ctot[3 * (2 * kCgMaxSteps + 1)];
    for (int s = threadIdx.x; s < slots; s += kDcFinishThreads) {
      float t = 0.f;
      for (int b = 0; b < curve_bx; ++b) t += curve_records[(size_t(n) * curve_bx + b) * size_t(3 * per_curve) + s];
      ctot[s] = t;
    }
    __syncthreads();
    if (threadIdx.x < kDcRow) {
      const int j = threadIdx.x;
      float g = 0.0f;
      if (j < curves * L) {
        const int c = j / L, i = j % L;
        const float* k = prm + c * L;
        float s = 0.f;
        for (int m = 0; m < L; ++m) s += k[m];
        s += 1e-30f;
        const float* t = ctot + c * per_curve;
        float above = 0.f;  // sum_{j > i} H_j
        for (int m = L - 1; m > i; --m) above += t[m];
        const float clip_sum = above / float(L) + t[L + i];
        g = (float(L) / s) * clip_sum - t[2 * L] / s;
      }
      out[j] = g;
    }
    return;
  }
  __shared__ float part[kDcFinishThreads / kWsSlots][kWsSlots];
  __shared__ float tot[kWsSlots];
  const int j = threadIdx.x & (kWsSlots - 1), g = threadIdx.x / kWsSlots;
  constexpr int kGroups = kDcFinishThreads / kWsSlots;
  float s = 0.f;
  {
    const float* r = light_records + (size_t(n) * light_bx) * kWsSlots + j;
    int b = g;
    for (; b + 3 * kGroups < light_bx; b += 4 * kGroups) {
      const float a0 = r[size_t(b) * kWsSlots], a1 = r[size_t(b + kGroups) * kWsSlots];
      const float a2 = r[size_t(b + 2 * kGroups) * kWsSlots], a3 = r[size_t(b + 3 * kGroups) * kWsSlots];
      s += a0;
      s += a1;
      s += a2;
      s += a3;
    }
    for (; b < light_bx; b += kGroups) s += r[size_t(b) * kWsSlots];
  }
  part[g][j] = s;
  __syncthreads();
  if (threadIdx.x >= 64) return;  // wave 0 finishes
  if (lane < kWsSlots) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < kGroups; ++k) v += part[k][lane];
    tot[lane] = v;
  }
  __builtin_amdgcn_wave_barrier();  // one wave: its LDS operations execute in order
  switch (id) {
    case 0: dc_finish_light<ExposureF>(prm, tot, out, lane); break;
    case 1: dc_finish_light<GammaF>(prm, tot, out, lane); break;
    case 2: dc_finish_light<WhiteBalanceF>(prm, tot, out, lane); break;
    case 3: dc_finish_light<SatPlusF>(prm, tot, out, lane); break;
    case 5: dc_finish_light<ContrastF>(prm, tot, out, lane); break;
    case 6: dc_finish_light<WnbF>(prm, tot, out, lane); break;
    case 8: dc_finish_light<LevelF>(prm, tot, out, lane); break;
    default: break;
  }
}

// the fused penalty of the forward: penalty[n] = (sum of the image's block records) * scale, 0 for id -1
__global__ __launch_bounds__(64) void dispatch_curves_penalty_kernel(const int32_t* __restrict__ ids,
                                                                     const float* __restrict__ records, int bx,
                                                                     float* __restrict__ penalty, float scale) {
  // one wave per image: lane l adds records l, l + 64, ... in order, then a fixed butterfly
  const int img = blockIdx.x;
  const int id = ids[img];
  float s = 0.f;
  if (id >= 0 && id < EXPO_NUM_FILTERS)
    for (int b = threadIdx.x; b < bx; b += 64) s += records[(size_t(img) * bx + b) * kWsSlots];
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  if (threadIdx.x == 0) penalty[img] = s * scale;
}

// ------------------------------------------------------------------------------------------ heads
// expo_heads_regress_fwd / _bwd (nn_ops.hip) with a Tone head of L and a Color head of 3 L values and 48-float rows
struct HeadsCurvesArgs {
  const float* raw[EXPO_MAX_HEADS];  // head j: [n][width_j] row-major (width_j >= P_j)
  float* draw[EXPO_MAX_HEADS];       // backward: same shapes
  int width[EXPO_MAX_HEADS];
  int abi[EXPO_MAX_HEADS];
  int heads, L;
  float exposure_range, log_gamma_range, tone_lo, tone_hi, tone_bias, color_lo, color_hi, color_bias, exposure_bias;
};
__host__ __device__ inline int dc_head_params(int fid, int L) {
  return fid == 4 ? L : fid == 7 ? 3 * L : (fid >= 0 && fid < EXPO_NUM_FILTERS) ? kNumParams[fid] : 0;
}
__device__ __forceinline__ float dc_tanh01(float x) { return tanhf(x) * 0.5f + 0.5f; }
__device__ __forceinline__ float dc_dtanh01(float x) { const float t = tanhf(x); return 0.5f * (1.0f - t * t); }
__device__ __forceinline__ float dc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void heads_regress_curves_fwd_kernel(const HeadsCurvesArgs a,
                                                                      const int32_t* __restrict__ sel,
                                                                      float* __restrict__ params, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kDcRow) return;
  const int img = t / kDcRow, k = t % kDcRow;
  const int j = sel[img];
  float out = 0.f;
  if (j >= 0 && j < a.heads) {
    const int fid = a.abi[j];
    if (k < dc_head_params(fid, a.L)) {
      const float* f = a.raw[j] + size_t(img) * a.width[j];
      const float x = f[k];
      switch (fid) {
        case 0: out = dc_tanh01(x + a.exposure_bias) * (2.0f * a.exposure_range) - a.exposure_range; break;
        case 1: out = expf(dc_tanh01(x) * (2.0f * a.log_gamma_range) - a.log_gamma_range); break;
        case 2: {  // features * (0, 1, 1); exp(tanh_range(-.5, .5)); normalised by the luminance of the scaling
          const float s0 = expf(dc_tanh01(0.0f) - 0.5f), s1 = expf(dc_tanh01(f[1]) - 0.5f), s2 = expf(dc_tanh01(f[2]) - 0.5f);
          const float inv = 1.0f / (1e-5f + 0.27f * s0 + 0.67f * s1 + 0.06f * s2);
          out = (k == 0 ? s0 : (k == 1 ? s1 : s2)) * inv;
        } break;
        case 3: case 6: case 8: out = dc_sigmoid(x); break;
        case 4: out = dc_tanh01(x + a.tone_bias) * (a.tone_hi - a.tone_lo) + a.tone_lo; break;
        case 5: out = tanhf(x); break;
        case 7: out = dc_tanh01(x + a.color_bias) * (a.color_hi - a.color_lo) + a.color_lo; break;
        default: break;
      }
    }
  }
  params[t] = out;
}

// d raw of EVERY head (zero outside the selected head's parameter slice, the mask columns included)
__global__ __launch_bounds__(256) void heads_regress_curves_bwd_kernel(const HeadsCurvesArgs a,
                                                                      const int32_t* __restrict__ sel,
                                                                      const float* __restrict__ dparams, int n,
                                                                      int total_width) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * total_width) return;
  const int img = t / total_width;
  int col = t % total_width, j = 0;
  while (col >= a.width[j]) col -= a.width[j++];
  float g = 0.f;
  if (j == sel[img]) {
    const int fid = a.abi[j];
    if (col < dc_head_params(fid, a.L)) {
      const float* f = a.raw[j] + size_t(img) * a.width[j];
      const float* dp = dparams + size_t(img) * kDcRow;
      const float x = f[col];
      switch (fid) {
        case 0: g = dp[col] * dc_dtanh01(x + a.exposure_bias) * (2.0f * a.exposure_range); break;
        case 1: {
          const float y = expf(dc_tanh01(x) * (2.0f * a.log_gamma_range) - a.log_gamma_range);
          g = dp[col] * y * dc_dtanh01(x) * (2.0f * a.log_gamma_range);
        } break;
        case 2:
          if (col > 0) {  // feature 0 is masked out (features * (0, 1, 1))
            const float s0 = expf(dc_tanh01(0.0f) - 0.5f), s1 = expf(dc_tanh01(f[1]) - 0.5f), s2 = expf(dc_tanh01(f[2]) - 0.5f);
            const float inv = 1.0f / (1e-5f + 0.27f * s0 + 0.67f * s1 + 0.06f * s2);
            const float sk = col == 1 ? s1 : s2, wk = col == 1 ? 0.67f : 0.06f;
            const float dsk = sk * dc_dtanh01(f[col]);  // d s_k / d f_k
            // out_c = s_c inv:  d out_c / d s_k = delta_ck inv - s_c inv^2 w_k
            const float dot = dp[0] * s0 + dp[1] * s1 + dp[2] * s2;
            g = dsk * (dp[col] * inv - dot * inv * inv * wk);
          }
          break;
        case 3: case 6: case 8: { const float y = dc_sigmoid(x); g = dp[col] * y * (1.0f - y); } break;
        case 4: g = dp[col] * dc_dtanh01(x + a.tone_bias) * (a.tone_hi - a.tone_lo); break;
        case 5: { const float y = tanhf(x); g = dp[col] * (1.0f - y * y); } break;
        case 7: g = dp[col] * dc_dtanh01(x + a.color_bias) * (a.color_hi - a.color_lo); break;
        default: break;
      }
    }
  }
  a.draw[j][size_t(img) * a.width[j] + col] = g;
}

// ------------------------------------------------------------------------------------------ host side
struct DcLayout {
  int light_bx;       // records per image of the light launches (the larger of the forward's and the backward's grids)
  int curve_bx;       // blocks per image of the curve backward
  size_t light_floats, curve_floats;
  size_t scratch_bytes;  // one image tensor: where the light backward launch writes dx when the caller wants none
};
static DcLayout dc_layout(int n, int h, int w, int dtype, int L) {
  DcLayout d;
  const int bf = dtype == EXPO_F16 ? make_geom<half_t>(n, h, w, {}, kGeomReduce).blocks_x
                                   : make_geom<float>(n, h, w, {}, kGeomReduce).blocks_x;
  const int bb = dtype == EXPO_F16 ? make_geom<half_t>(n, h, w, {}, kGeomDispatch).blocks_x
                                   : make_geom<float>(n, h, w, {}, kGeomDispatch).blocks_x;
  d.light_bx = bf > bb ? bf : bb;
  d.curve_bx = cg_blocks(h * w);
  d.light_floats = size_t(n) * d.light_bx * kWsSlots;
  d.curve_floats = size_t(n) * d.curve_bx * size_t(3 * (2 * L + 1));
  d.scratch_bytes = ((size_t(n) * h * w * 3 * (dtype == EXPO_F16 ? 2 : 4) + 3) / 4) * 4;
  return d;
}
static bool dc_steps_ok(int L) { return L >= 1 && L <= kCgMaxSteps; }

static int dc_check(int n, int h, int w, int dtype, int L) {
  if (int rc = check_common(n, h, w, dtype)) return rc;
  if (!dc_steps_ok(L)) return fail(EXPO_E_BADARG, "curve_steps must be in [1, EXPO_CURVE_MAX_STEPS]");
  return EXPO_OK;
}
static int dc_workspace(void* workspace, size_t workspace_bytes, int n, int h, int w, int dtype, int L) {
  if (!workspace) return fail(EXPO_E_BADARG, "workspace is NULL (size it with expo_filter_dispatch_curves_workspace_bytes)");
  if ((reinterpret_cast<uintptr_t>(workspace) & 3) != 0) return fail(EXPO_E_BADARG, "workspace must be 4-byte aligned");
  if (workspace_bytes < expo_filter_dispatch_curves_workspace_bytes(n, h, w, dtype, L))
    return fail(EXPO_E_BADARG, "workspace too small (expo_filter_dispatch_curves_workspace_bytes)");
  return EXPO_OK;
}

template <typename T>
static int dc_fwd_t(const int32_t* ids, const void* x, void* y, const float* params, int L, float* penalty, int n, int h,
                    int w, float* records, hipStream_t s) {
  // the geometry of expo_filter_dispatch_fwd: its light images then leave the same records
  const Geom g = make_geom<T>(n, h, w, {x, y}, kGeomReduce);
  const dim3 grid(g.blocks_x, n), block(kThreads);
#define EXPO_L(VEC, PEN, IO)                                                                                    \
  hipLaunchKernelGGL((dispatch_curves_fwd_kernel<T, VEC, PEN, IO>), grid, block, 0, s, ids, (const T*)x, (T*)y, \
                     params, records, g.hw, g.groups, L)
  if (g.stream) {
    if (penalty) EXPO_L(true, true, IoStream); else EXPO_L(true, false, IoStream);
  } else if (g.vec) {
    if (penalty) EXPO_L(true, true, IoCached); else EXPO_L(true, false, IoCached);
  } else {
    if (penalty) EXPO_L(false, true, IoCached); else EXPO_L(false, false, IoCached);
  }
#undef EXPO_L
  HIP_TRY(hipGetLastError(), "dispatch_curves_fwd launch");
  if (penalty) {
    hipLaunchKernelGGL(dispatch_curves_penalty_kernel, dim3(n), dim3(64), 0, s, ids, records, g.blocks_x, penalty,
                       1.0f / (float(g.hw) * 3.0f));
    HIP_TRY(hipGetLastError(), "dispatch_curves penalty finish launch");
  }
  return EXPO_OK;
}

template <typename T>
static int dc_bwd_t(const int32_t* ids, const void* x, const void* dy, void* dx, const float* params, float* dparams,
                    const float* dpenalty, int L, int n, int h, int w, int dtype, int mode, float* records,
                    hipStream_t s) {
  // the geometry of expo_filter_dispatch_bwd for the light launch (cached loads at every size: the step trains on
  // 64x64 proxies), cg_blocks for the curve launch
  const Geom g = make_geom<T>(n, h, w, {x, dy, dx}, kGeomDispatch);
  const DcLayout lay = dc_layout(n, h, w, dtype, L);
  float* curve_records = records + lay.light_floats;
  void* light_dx = dx ? dx : static_cast<void*>(curve_records + lay.curve_floats);
  const float inv_count = 1.0f / (float(g.hw) * 3.0f);
  const dim3 block(kThreads);
#define EXPO_L(VEC, MODE)                                                                                      \
  hipLaunchKernelGGL((dispatch_curves_bwd_light_kernel<T, VEC, MODE>), dim3(g.blocks_x, n), block, 0, s, ids,   \
                     (const T*)x, (const T*)dy, (T*)light_dx, params, records, dpenalty, g.hw, g.groups, inv_count)
  if (g.vec) { if (mode == 1) EXPO_L(true, 1); else EXPO_L(true, 0); }
  else { if (mode == 1) EXPO_L(false, 1); else EXPO_L(false, 0); }
#undef EXPO_L
  HIP_TRY(hipGetLastError(), "dispatch_curves_bwd light launch");
  const size_t lds = size_t(3 * (2 * L + 1)) * kCgPad * sizeof(float);
#define EXPO_C(HAS_DX)                                                                                               \
  do {                                                                                                               \
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&dispatch_curves_bwd_curve_kernel<T, HAS_DX>),          \
                                hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)), "dispatch_curves_bwd LDS size"); \
    hipLaunchKernelGGL((dispatch_curves_bwd_curve_kernel<T, HAS_DX>), dim3(lay.curve_bx, n), block, lds, s, ids,      \
                       (const T*)x, (const T*)dy, (T*)dx, params, curve_records, dpenalty, g.hw, L, inv_count);       \
  } while (0)
  if (dx) EXPO_C(true); else EXPO_C(false);
#undef EXPO_C
  HIP_TRY(hipGetLastError(), "dispatch_curves_bwd curve launch");
  hipLaunchKernelGGL(dispatch_curves_finish_kernel, dim3(n), dim3(kDcFinishThreads), 0, s, ids, params, dparams, records,
                     g.blocks_x, curve_records, lay.curve_bx, L);
  HIP_TRY(hipGetLastError(), "dispatch_curves_bwd finish launch");
  return EXPO_OK;
}

static int dc_heads_args(HeadsCurvesArgs* a, const float* const* raw, float* const* draw, const int* widths,
                         const int* abi_ids, int heads, const float* ranges, int L) {
  if (!dc_steps_ok(L)) return fail(EXPO_E_BADARG, "curve_steps must be in [1, EXPO_CURVE_MAX_STEPS]");
  if (heads < 1 || heads > EXPO_MAX_HEADS || !raw || !widths || !abi_ids || !ranges)
    return fail(EXPO_E_BADARG, "bad heads arguments");
  for (int j = 0; j < heads; ++j) {
    if (!raw[j] || (draw && !draw[j])) return fail(EXPO_E_BADARG, "null pointer");
    if (abi_ids[j] < 0 || abi_ids[j] >= EXPO_NUM_FILTERS) return fail(EXPO_E_BADARG, "filter_id out of range");
    if (widths[j] < dc_head_params(abi_ids[j], L)) return fail(EXPO_E_BADARG, "head narrower than its filter's parameter count");
    a->raw[j] = raw[j];
    a->draw[j] = draw ? draw[j] : nullptr;
    a->width[j] = widths[j];
    a->abi[j] = abi_ids[j];
  }
  a->heads = heads;
  a->L = L;
  a->exposure_range = ranges[0]; a->log_gamma_range = ranges[1];
  a->tone_lo = ranges[2]; a->tone_hi = ranges[3]; a->tone_bias = ranges[4];
  a->color_lo = ranges[5]; a->color_hi = ranges[6]; a->color_bias = ranges[7]; a->exposure_bias = ranges[8];
  return EXPO_OK;
}

}  // namespace expo

using namespace expo;

extern "C" {

size_t expo_filter_dispatch_curves_workspace_bytes(int n, int h, int w, int dtype, int curve_steps) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || (dtype != EXPO_F16 && dtype != EXPO_F32) || !dc_steps_ok(curve_steps)) return 0;
  const DcLayout lay = dc_layout(n, h, w, dtype, curve_steps);
  return (lay.light_floats + lay.curve_floats) * sizeof(float) + lay.scratch_bytes;
}

int expo_filter_dispatch_curves_fwd(const int32_t* filter_ids, const void* x, void* y, const float* params,
                                    int curve_steps, float* penalty, int n, int h, int w, int dtype, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (int rc = dc_check(n, h, w, dtype, curve_steps)) return rc;
  if (n == 0) return EXPO_OK;
  if (!filter_ids || !x || !y || !params) return fail(EXPO_E_BADARG, "null pointer");
  if (penalty)
    if (int rc = dc_workspace(workspace, workspace_bytes, n, h, w, dtype, curve_steps)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* records = static_cast<float*>(workspace);
  return dtype == EXPO_F16 ? dc_fwd_t<half_t>(filter_ids, x, y, params, curve_steps, penalty, n, h, w, records, s)
                           : dc_fwd_t<float>(filter_ids, x, y, params, curve_steps, penalty, n, h, w, records, s);
}

int expo_filter_dispatch_curves_bwd(const int32_t* filter_ids, const void* x, const void* dy, void* dx,
                                    const float* params, float* dparams, const float* dpenalty, int curve_steps, int n,
                                    int h, int w, int dtype, int hsv_grad_mode, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (int rc = dc_check(n, h, w, dtype, curve_steps)) return rc;
  if (hsv_grad_mode != 0 && hsv_grad_mode != 1) return fail(EXPO_E_BADARG, "hsv_grad_mode must be 0 or 1");
  if (n == 0) return EXPO_OK;
  if (!filter_ids || !x || !dy || !params || !dparams) return fail(EXPO_E_BADARG, "null pointer");
  if (int rc = dc_workspace(workspace, workspace_bytes, n, h, w, dtype, curve_steps)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* records = static_cast<float*>(workspace);
  return dtype == EXPO_F16 ? dc_bwd_t<half_t>(filter_ids, x, dy, dx, params, dparams, dpenalty, curve_steps, n, h, w,
                                              dtype, hsv_grad_mode, records, s)
                           : dc_bwd_t<float>(filter_ids, x, dy, dx, params, dparams, dpenalty, curve_steps, n, h, w, dtype,
                                             hsv_grad_mode, records, s);
}

int expo_heads_regress_curves_fwd(const float* const* raw, const int* widths, const int* abi_ids, int heads,
                                  const float* ranges, const int32_t* selected, float* params, int curve_steps, int n,
                                  void* stream) {
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  HeadsCurvesArgs a{};
  if (int rc = dc_heads_args(&a, raw, nullptr, widths, abi_ids, heads, ranges, curve_steps)) return rc;
  if (n == 0) return EXPO_OK;
  if (!selected || !params) return fail(EXPO_E_BADARG, "null pointer");
  const int total = n * kDcRow;
  hipLaunchKernelGGL(heads_regress_curves_fwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, selected, params, n);
  HIP_TRY(hipGetLastError(), "heads_regress_curves_fwd launch");
  return EXPO_OK;
}

int expo_heads_regress_curves_bwd(const float* const* raw, float* const* draw, const int* widths, const int* abi_ids,
                                  int heads, const float* ranges, const int32_t* selected, const float* dparams,
                                  int curve_steps, int n, void* stream) {
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  HeadsCurvesArgs a{};
  if (!draw) return fail(EXPO_E_BADARG, "null pointer");
  if (int rc = dc_heads_args(&a, raw, draw, widths, abi_ids, heads, ranges, curve_steps)) return rc;
  if (n == 0) return EXPO_OK;
  if (!selected || !dparams) return fail(EXPO_E_BADARG, "null pointer");
  int total_width = 0;
  for (int j = 0; j < heads; ++j) total_width += widths[j];
  const int total = n * total_width;
  hipLaunchKernelGGL(heads_regress_curves_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, selected, dparams, n, total_width);
  HIP_TRY(hipGetLastError(), "heads_regress_curves_bwd launch");
  return EXPO_OK;
}

}  // extern "C"
