// metric.hip -- the paper's evaluation metric on the device: the three statistics of every 64 x 64 patch and their
// histograms.  expo_patch_stats / expo_stat_hist; DESIGN.md §3.21.
//
//   patch_stats_kernel  one block per record: a C x C crop of one master image -> [mean lum, 2 std lum, mean sat].
//                       Thread t owns the pixels t, t + 256, ... of the crop (row-major) and sums them in that order in
//                       double; the 256 partials meet in a fixed LDS tree.  No atomics: a row is bit-identical run to
//                       run and whatever else the launch holds.  The luminance is summed relative to the crop's first
//                       pixel (the variance of l - l0 is the variance of l), so a constant crop has std exactly 0 and
//                       the subtraction mean(d^2) - mean(d)^2 loses nothing for flat crops.
//   stat_hist_kernel    one block: the 3 q statistics into [3][bins] counts held in LDS (integer atomics: the counts do
//                       not depend on the order), then written out whole.
#include "host_common.h"

namespace expo {

namespace {

constexpr int kHistMaxBins = 1024;

// every operation of the definition is rounded on its own, so that the crop's first pixel gives the same luminance in
// every thread as it does as a term of the sum, and the float64 restatement evaluates the same expressions
#pragma clang fp contract(off)
__device__ inline double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

__device__ inline double luminance(double r, double g, double b) { return r * 0.27 + g * 0.67 + b * 0.06; }

// the S channel of RGB -> HLS as metrics.hls_saturation has it: 0 where max == min (no epsilon)
__device__ inline double hls_saturation(double r, double g, double b) {
  const double mx = fmax(r, fmax(g, b)), mn = fmin(r, fmin(g, b));
  const double d = mx - mn;
  if (!(d > 0.0)) return 0.0;
  const double l = (mx + mn) * 0.5;
  const double den = l < 0.5 ? mx + mn : 2.0 - mx - mn;
  return d / (den > 1e-12 ? den : 1e-12);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void patch_stats_kernel(const T* __restrict__ master, int m, int S,
                                                               const int32_t* __restrict__ records, int C,
                                                               float* __restrict__ stats) {
  __shared__ double part[3][kThreads];
  const int r = blockIdx.x, t = threadIdx.x;
  // (a record out of range is the caller's error; it is clamped so that no read leaves the master)
  const int src = min(max(records[3 * r], 0), m - 1);
  const int oy = min(max(records[3 * r + 1], 0), S - C);
  const int ox = min(max(records[3 * r + 2], 0), S - C);
  const T* in = master + (long(src) * S + oy) * long(S) * 3 + long(ox) * 3;
  const long stride = long(S) * 3;
  const double l0 = luminance(clip01(double(float(in[0]))), clip01(double(float(in[1]))), clip01(double(float(in[2]))));
  double sd = 0.0, sdd = 0.0, ss = 0.0;
  const int total = C * C;
  for (int p = t; p < total; p += kThreads) {
    const int y = p / C, x = p - y * C;
    const T* px = in + y * stride + x * 3;
    const double cr = clip01(double(float(px[0]))), cg = clip01(double(float(px[1]))), cb = clip01(double(float(px[2])));
    const double d = luminance(cr, cg, cb) - l0;
    sd += d;
    sdd += d * d;
    ss += hls_saturation(cr, cg, cb);
  }
  part[0][t] = sd;
  part[1][t] = sdd;
  part[2][t] = ss;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (t < h) {
      part[0][t] += part[0][t + h];
      part[1][t] += part[1][t + h];
      part[2][t] += part[2][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double n = double(total);
    const double md = part[0][0] / n;
    const double var = part[1][0] / n - md * md;
    stats[3 * r] = float(l0 + md);
    stats[3 * r + 1] = float(2.0 * sqrt(var > 0.0 ? var : 0.0));
    stats[3 * r + 2] = float(part[2][0] / n);
  }
}
#pragma clang fp contract(on)

__global__ __launch_bounds__(kThreads) void stat_hist_kernel(const float* __restrict__ stats, int q, int bins,
                                                             int32_t* __restrict__ counts) {
  __shared__ int hist[3 * kHistMaxBins];
  for (int i = threadIdx.x; i < 3 * bins; i += kThreads) hist[i] = 0;
  __syncthreads();
  const long total = 3L * q;
  for (long e = threadIdx.x; e < total; e += kThreads) {
    const float v = stats[e];
    if (v >= 0.0f && v <= 1.0f) {  // (NaN fails both)
      const int b = min(int(v * float(bins)), bins - 1);
      atomicAdd(&hist[int(e % 3) * bins + b], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * bins; i += kThreads) counts[i] = hist[i];
}

}  // namespace

}  // namespace expo

using namespace expo;

extern "C" {

int expo_patch_stats(const void* master, int m, int S, const int32_t* records, int count, int C, float* stats,
                     int dtype, void* stream) {
  if (count < 0) return fail(EXPO_E_BADARG, "count >= 0 required");
  if (dtype != EXPO_F16 && dtype != EXPO_F32) return fail(EXPO_E_BADDTYPE, "dtype must be EXPO_F16 or EXPO_F32");
  if (S < 1 || C < 1 || C > S) return fail(EXPO_E_BADARG, "1 <= C <= S required");
  if (long(S) * S * 3 * (dtype == EXPO_F16 ? 2L : 4L) > (1L << 31))
    return fail(EXPO_E_BADARG, "one master image must be <= 2 GiB");
  if (count == 0) return EXPO_OK;
  if (m < 1) return fail(EXPO_E_BADARG, "m >= 1 required");
  if (!master || !records || !stats) return fail(EXPO_E_BADARG, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == EXPO_F32)
    hipLaunchKernelGGL(patch_stats_kernel<float>, dim3(unsigned(count)), dim3(kThreads), 0, s,
                       static_cast<const float*>(master), m, S, records, C, stats);
  else
    hipLaunchKernelGGL(patch_stats_kernel<half_t>, dim3(unsigned(count)), dim3(kThreads), 0, s,
                       static_cast<const half_t*>(master), m, S, records, C, stats);
  HIP_TRY(hipGetLastError(), "patch_stats launch");
  return EXPO_OK;
}

int expo_stat_hist(const float* stats, int q, int bins, int32_t* counts, void* stream) {
  if (q < 0) return fail(EXPO_E_BADARG, "q >= 0 required");
  if (bins < 1 || bins > kHistMaxBins) return fail(EXPO_E_BADARG, "1 <= bins <= 1024 required");
  if (!counts || (q > 0 && !stats)) return fail(EXPO_E_BADARG, "null pointer");
  hipLaunchKernelGGL(stat_hist_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), stats, q, bins,
                     counts);
  HIP_TRY(hipGetLastError(), "stat_hist launch");
  return EXPO_OK;
}

}  // extern "C"
