/*
 * exposure_hip.h -- C-ABI of libexposure_hip.so: the MI355X (gfx950) implementation
 * of Exposure's differentiable per-pixel filter stack.
 *
 * The reference (yuanming-hu/exposure, TF-1 Python) has NO FFI for this path: the
 * filters are Python classes composed of TF elementwise ops.  This header is the
 * boundary a native replacement of that path binds; each entry point cites the
 * reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - Images are contiguous NHWC, C = 3, dtype EXPO_F16 (default) or EXPO_F32.
 *   - Every pointer is a caller-owned DEVICE pointer that must stay valid until the
 *     work enqueued on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) has completed.  No allocation, no ownership transfer, no host sync.
 *   - Stateless and re-entrant; ordering only through `stream`.
 *   - Reduction workspace.  Every entry point that produces per-image sums (parameter
 *     gradients, penalty, statistics) takes `workspace` / `workspace_bytes`: a caller-owned,
 *     4-byte aligned device scratch buffer of at least expo_workspace_bytes(n, h, w, dtype)
 *     bytes (expo_chain_bwd: that many bytes PER STEP).  It needs no initialisation and
 *     carries nothing from call to call: the streaming kernel leaves one record of partial
 *     sums per block in it and a small finish launch enqueued behind it adds an image's
 *     records in a fixed order -- no float atomics, no zero-fill launch, bit-reproducible
 *     results.  One workspace serves one stream at a time (calls that may run concurrently on
 *     different streams need their own).
 *   - Filter ids follow cfg.filters (config_example.py:22-25):
 *       0 E  ExposureFilter              P = 1   params[n][0] = EV stops
 *       1 G  GammaFilter                 P = 1   gamma
 *       2 W  ImprovedWhiteBalanceFilter  P = 3   per-channel scale
 *       3 S+ SaturationPlusFilter        P = 1   blend in [0,1]
 *       4 T  ToneFilter                  P = 8   curve slopes k_0..k_7
 *       5 Ct ContrastFilter              P = 1   blend in [-1,1]
 *       6 BW WNBFilter                   P = 1   blend in [0,1]
 *       7 C  ColorFilter                 P = 24  k[channel*8 + knot]
 *       8 Le LevelFilter                 P = 2   lower, upper-1   (not in cfg.filters)
 *     `params` are the outputs of Filter.filter_param_regressor (filters.py:177-179,
 *     201-203, 224-235, 481-482, 306-310, 411-413, 435-436, 256-262) flattened to
 *     float32 [N][P].
 *   - All functions return EXPO_OK (0) or a negative EXPO_E_* code; the message of
 *     the last failure on the calling thread is available from expo_last_error().
 */
#ifndef EXPOSURE_HIP_H_
#define EXPOSURE_HIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXPO_ABI_VERSION 9 /* 2: caller-owned reduction workspace (no float atomics, no fills); 3: derivatives of the
                              critic statistics and of the penalty, VignetFilter, bias + lrelu, masked per-image dispatch;
                              4: Tone / Color curves of any cfg.curve_steps (expo_curve_*); 5: the convnets' convolution
                              (expo_conv4x4s2_*); 6: its mask / bias variants, the hand-scheduled critic update's
                              kernels, expo_build_info; 7: expo_net_inputs, the first FC layer with its K dimension split
                              (expo_fc_*; expo_critic_head_fwd / _bwd take the partial sums); 8: expo_chain_plan;
                              9: expo_chain_fused_fwd_ragged; added exports: the taps, expo_decode_ragged,
                              expo_area_resize_ragged, expo_pack_recut, expo_bilinear_resize_ragged,
                              expo_patch_stats, expo_stat_hist, expo_chain_fused_masked_fwd_ragged,
                              expo_decode_tables, expo_bilinear_resize_ragged_codes,
                              expo_chain_fused_fwd_ragged_codes, expo_codes_max_ragged,
                              expo_codes_lut_ragged, expo_chain_fused_curves_fwd_ragged,
                              expo_chain_fused_curves_fwd_ragged_codes, expo_png_segment_bytes,
                              expo_png_encode_bound, expo_png_encode_workspace_bytes, expo_png_encode_ragged,
                              expo_jpeg_restart_mcus, expo_jpeg_encode_bound, expo_jpeg_encode_workspace_bytes,
                              expo_jpeg_encode_ragged, expo_jpeg_decode_plan_bytes, expo_jpeg_decode_workspace_bytes,
                              expo_jpeg_decode_ragged, expo_jpeg_decode_sync_workspace_bytes,
                              expo_jpeg_decode_sync_ragged */

#define EXPO_OK 0
#define EXPO_E_BADARG (-1)
#define EXPO_E_BADDTYPE (-2)
#define EXPO_E_HIP (-3)

#define EXPO_F16 0
#define EXPO_F32 1

#define EXPO_NUM_FILTERS 9
#define EXPO_MAX_PARAMS 24
#define EXPO_MAX_HEADS 16 /* FC heads one expo_heads_regress_* call serves (cfg.filters has 8) */
#define EXPO_CURVE_MAX_STEPS 16 /* largest cfg.curve_steps of expo_curve_fwd / _bwd */
#define EXPO_MAX_PARAMS_CURVES 48 /* a parameter row of expo_chain_fused_curves_fwd_ragged: 3 x EXPO_CURVE_MAX_STEPS */

#define EXPO_FILTER_EXPOSURE 0
#define EXPO_FILTER_GAMMA 1
#define EXPO_FILTER_WB 2
#define EXPO_FILTER_SATPLUS 3
#define EXPO_FILTER_TONE 4
#define EXPO_FILTER_CONTRAST 5
#define EXPO_FILTER_WNB 6
#define EXPO_FILTER_COLOR 7
#define EXPO_FILTER_LEVEL 8 /* LevelFilter (filters.py:449-466): defined by the reference, not in cfg.filters */

/* hsv_grad_mode for SaturationPlus backward: 0 = TF-1.x faithful (RGBToHSV / HSVToRGB
 * are registered NotDifferentiable, so no gradient flows through full_color);
 * 1 = analytic gradient through the HSV round trip. */
#define EXPO_HSV_GRAD_TF1 0
#define EXPO_HSV_GRAD_ANALYTIC 1

/* Library / ABI version (EXPO_ABI_VERSION of the built library). */
int expo_version(void);

/* Message of the last error raised on the calling thread ("" if none). */
const char* expo_last_error(void);

/* (ABI 6) The sha256 (hex) of the sources this binary was built from -- csrc/build.sh hashes include/exposure_hip.h and
 * the .hip / .h files and build.sh of csrc/ (byte order of their names) and passes the digest to the compiler.  The
 * Python binding recomputes it from the tree and refuses a stale binary (EXPO_ALLOW_STALE_LIB=1 overrides); "unknown"
 * for a build that bypassed build.sh. */
const char* expo_build_info(void);

/* Replaces Filter.get_num_filter_parameters() (filters.py:24-26); -1 on bad id. */
int expo_num_filter_params(int filter_id);

/*
 * Bytes of reduction workspace ONE reducing call needs for images of this shape (the maximum
 * over the entry points; expo_chain_bwd needs `steps` times as much).  0 on invalid arguments.
 * New with ABI 2; the reference has no counterpart (TF allocates its reduction scratch itself).
 */
size_t expo_workspace_bytes(int n, int h, int w, int dtype);

/*
 * y = <Filter>.process(x, params)      replaces filters.py:181-182 (E), 205-206 (G),
 * 237-238 (W), 484-498 (S+), 312-322 (T), 415-419 (Ct), 438-440 (BW), 264-273 (C).
 * With cfg.masking = False (config_example.py:36) this is also Filter.apply's
 * lerp(img, process(img, p), ones) (filters.py:88, 111-113).
 * x, y: [N][H][W][3] of dtype; y may alias x.  params: float32 [N][P].
 * Any H, W >= 1 (the same parameters may be applied to the 64x64 proxy and to the
 * full-resolution image: filters.py:89-96).
 */
int expo_filter_fwd(int filter_id, const void* x, void* y, const float* params,
                    int n, int h, int w, int dtype, void* stream);

/*
 * Backward of expo_filter_fwd: what tf.gradients produces for process() in the
 * reference graph (net.py:222-251 via ly.optimize_loss).
 *   dx      [N][H][W][3] dtype, may be NULL (parameter gradient only), may alias dy.
 *   dparams float32 [N][P], OVERWRITTEN with sum_{h,w,c} dy * d y/d param.
 * y is recomputed from x (never read).
 */
int expo_filter_bwd(int filter_id, const void* x, const void* dy, void* dx,
                    const float* params, float* dparams, int n, int h, int w,
                    int dtype, int hsv_grad_mode, void* workspace, size_t workspace_bytes,
                    void* stream);

/*
 * Same as expo_filter_bwd but dparams is ACCUMULATED into (dparams += ...): the caller owns
 * the initial value.  This is gradient accumulation over several
 * backward calls that share a parameter tensor (e.g. the low-resolution and the high-resolution
 * application of one filter, filters.py:88-96, or micro-batches).
 */
int expo_filter_bwd_accumulate(int filter_id, const void* x, const void* dy, void* dx,
                               const float* params, float* dparams, int n, int h, int w,
                               int dtype, int hsv_grad_mode, void* workspace,
                               size_t workspace_bytes, void* stream);

/*
 * Filter.apply with the spatial mask enabled (cfg.masking = True; filters.py:62-99, 110-148):
 *   out = (1 - mask) * x + mask * process(x, params)
 *   mask = sigmoid((gx*m0 + gy*m1 + m2*(lum(x) - .5) + 2*m3) * maximum_sharpness * m4 / 5)
 *          * (m5/5 * .5 + .5) * (1 - minimum_strength) + minimum_strength
 * mask_params: float32 [N][6] = tanh_range(-5, 5)(raw mask parameters) -- the range squashing
 * (filters.py:121-123) stays with the caller so its gradient is handled by the host autograd.
 * gx, gy: the constant coordinate grid of filters.py:124-133.  cfg.maximum_sharpness and
 * cfg.minimum_strength are config_example.py:37-38.
 */
int expo_filter_apply_fwd(int filter_id, const void* x, void* y, const float* params,
                          const float* mask_params, float maximum_sharpness, float minimum_strength,
                          int n, int h, int w, int dtype, void* stream);

/* Backward of expo_filter_apply_fwd; dparams [N][P] and dmask_params [N][6] are overwritten. */
int expo_filter_apply_bwd(int filter_id, const void* x, const void* dy, void* dx,
                          const float* params, float* dparams, const float* mask_params,
                          float* dmask_params, float maximum_sharpness, float minimum_strength,
                          int n, int h, int w, int dtype, int hsv_grad_mode, void* workspace,
                          size_t workspace_bytes, void* stream);

/*
 * The agent's step with cfg.masking = True (agent.py:58-77, 119-125 around filters.py:62-99, 110-148): the reference runs
 * EVERY filter's masked apply on the whole batch, stacks the 8 results and reduces with one_hot(selected_filter_id).
 * The one-hot zeroes the seven others (values and gradients), so per image only the selected filter's masked apply runs:
 *   y[n] = expo_filter_apply_fwd(filter_ids[n], x[n], params[n], mask_params[n])      filter_ids[n] = -1 -> y[n] = 0
 * params / dparams: float32 [N][EXPO_MAX_PARAMS] (row = packed parameters of filter filter_ids[n], rest ignored / 0);
 * mask_params / dmask_params: float32 [N][6] = tanh_range(-5, 5)(raw mask parameters of THAT filter).
 */
int expo_filter_apply_dispatch_fwd(const int32_t* filter_ids, const void* x, void* y, const float* params,
                                   const float* mask_params, float maximum_sharpness, float minimum_strength,
                                   int n, int h, int w, int dtype, void* stream);
int expo_filter_apply_dispatch_bwd(const int32_t* filter_ids, const void* x, const void* dy, void* dx,
                                   const float* params, float* dparams, const float* mask_params,
                                   float* dmask_params, float maximum_sharpness, float minimum_strength, int n,
                                   int h, int w, int dtype, int hsv_grad_mode, void* workspace,
                                   size_t workspace_bytes, void* stream);

/*
 * Per-image filter choice == the reference's "compute all 8 filters, stack, multiply
 * by one_hot(selected_filter_id), reduce_sum" (agent.py:58-77, 119-125) without the
 * 7 discarded outputs.  filter_ids: int32 [N] in [-1, 8]; -1 (pdf_sample with noise
 * 0, pdf_sample_layer.py:5-10) selects nothing: y = 0, all gradients 0.
 * params / dparams: float32 [N][EXPO_MAX_PARAMS]; row n holds the P values of filter
 * filter_ids[n] in its first P slots (remaining slots ignored / written as 0).
 * penalty (nullable): float32 [N], overwritten with mean_{h,w,c} max(y - 1, 0)^2,
 * the over-exposure term of agent.py:249-251, fused into the same pass (workspace needed
 * only when penalty != NULL).
 */
int expo_filter_dispatch_fwd(const int32_t* filter_ids, const void* x, void* y,
                             const float* params, float* penalty, int n, int h, int w,
                             int dtype, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Backward of expo_filter_dispatch_fwd.  dpenalty (nullable): float32 [N], upstream
 * gradient of the fused penalty; its contribution 2*max(y-1,0)/(H*W*3)*dpenalty[n]
 * is added to dy before back-propagating through the selected filter.
 */
int expo_filter_dispatch_bwd(const int32_t* filter_ids, const void* x, const void* dy,
                             void* dx, const float* params, float* dparams,
                             const float* dpenalty, int n, int h, int w, int dtype,
                             int hsv_grad_mode, void* workspace, size_t workspace_bytes,
                             void* stream);

/*
 * The two halves of expo_filter_bwd, for callers that finish several passes with one launch
 * (expo_chain_bwd is exactly: the records pass of every step, then one expo_finish_bwd) and for
 * per-kernel timing.  expo_filter_bwd_records runs the streaming pass alone: dx is written, the
 * per-block partial sums stay in `records` (>= expo_workspace_bytes(n, h, w, dtype) bytes), dparams
 * is not touched.  expo_finish_bwd turns `steps` record slices -- slice k at byte offset
 * k * expo_workspace_bytes(...) of `workspace` -- into the parameter gradients dparams[k] of the
 * filters filter_ids[k] (host arrays, as in expo_chain_bwd).  No reference counterpart: TF fuses
 * nothing here (net.py:222-251 builds one reduction per parameter tensor).
 */
int expo_filter_bwd_records(int filter_id, const void* x, const void* dy, void* dx,
                            const float* params, int n, int h, int w, int dtype,
                            int hsv_grad_mode, void* records, size_t records_bytes, void* stream);
int expo_finish_bwd(const int* filter_ids, int steps, const float* const* params,
                    float* const* dparams, int n, int h, int w, int dtype, void* workspace,
                    size_t workspace_bytes, void* stream);

/*
 * The benchmark construct of SURVEY.md section 8(d): `steps` filters applied
 * sequentially, enqueued by a single call.  The forward runs up to 8 consecutive steps of a
 * chunk of the plan in ONE launch (csrc/chain_steps.hip): a pixel group is loaded once, and after
 * every step it is rounded to the storage type, stored to acts[k+1] and carried on in registers,
 * so every acts[k+1] holds the very bits a per-step expo_filter_fwd would have written.
 * EXPO_CHAIN_FUSE_STEPS=<k> in the environment (read once per process) caps the steps per launch;
 * 1 is one kernel per step.  Shapes off the 12-byte vector path (odd fp16 pixel counts, unaligned
 * bases) and the reversed walk (below) keep one kernel per step.  The backward is one kernel per step.
 *   filter_ids  host int [steps]
 *   acts        host array of steps+1 device image pointers: acts[0] = input,
 *               acts[i+1] = output of step i (kept: the backward reads them)
 *   params      host array of `steps` device pointers, float32 [N][P_i]
 *
 * Images are independent, so for batches whose tensors are between 40 and 256 MiB the chain entry points split the
 * batch in two halves and run them on two streams -- `stream` and a library-owned helper stream, forked and joined
 * with events INSIDE the call (one half's kernels fill the ramp / tail bubbles of the other's 17 dependent launches:
 * -3.5 % per step at 64x512x512).  Nothing changes for the caller: all work is ordered after what `stream` held
 * before the call and before what it receives afterwards, and the pattern is capturable into a hipGraph.
 * expo_chain_streams() returns the number of streams (1 or 2) a shape gets (EXPO_CHAIN_STREAMS=1|2 overrides).
 * A tensor of 256 MiB or more (EXPO_CHAIN_TILE_MIN_MIB) runs TILE-MAJOR instead: every step on one tile of images
 * (EXPO_CHAIN_TILE_MIB per tensor, balanced: tile sizes differ by at most one image) before the next, each tile split
 * over the two streams when a tile of the smaller size would be.  Consecutive launches walk the images in alternating
 * order for an untiled tensor of 256 MiB or more (EXPO_CHAIN_SNAKE=0|1 overrides; EXPO_CHAIN_SNAKE is IGNORED when the
 * batch is tiled).
 *
 * (ABI 8) expo_chain_plan() reports the plan expo_chain_fwd / _bwd run for a shape, read-only (it launches nothing and
 * touches no stream): the return value is the number of chunks C (0 for n == 0; a negative EXPO_E_* on invalid
 * arguments), the first min(C, max_chunks) chunks are written to chunks[3 k .. 3 k + 2] = (first image, image count,
 * lane: 0 = `stream`, 1 = the helper) in launch order, *lanes = 1 or 2, *snake = 1 when alternate launches walk the
 * images in reverse.  chunks may be NULL when max_chunks is 0; lanes and snake may be NULL.
 *
 * The helper is chosen per (device, caller stream) and must sit on another hardware queue than `stream`: the pairing
 * is probed ONCE per caller stream (two one-wave kernels, < 0.1 ms; a rejected helper costs 0.5 ms -- the kernel on
 * `stream` waits that long for the helper's -- at most 4 candidates; both streams are synchronised), see
 * exposure_hip.hip.  By default the first EAGER two-stream chain call of a caller stream does that; an integrator who
 * does not want a stall inside a data-path call runs it at set-up time with expo_chain_prepare(stream) (idempotent;
 * nothing to do under stream capture, where the graph executor assigns the queues).  EXPO_CHAIN_HELPER_PROBE=0 in the
 * environment switches the probe off altogether (the first helper stream is taken as it comes).  Only callers on the
 * SAME stream wait for a probe.  expo_chain_release(stream) forgets a pairing and destroys its helper stream -- call it
 * before hipStreamDestroy of a stream that made chain calls (where the runtime has hipStreamGetId -- HIP >= 7.1 -- a destroyed
 * stream whose handle is reused is recognised and probed again either way).  Rejected helper streams stay parked (at most 8 per process) so
 * that their hardware queue is not handed out again.  expo_chain_helper_stats() reports how many pairings this
 * process probed and how many helpers it rejected (diagnostics; either pointer may be NULL).
 */
int expo_chain_streams(int n, int h, int w, int dtype);
int expo_chain_plan(int n, int h, int w, int dtype, int* chunks, int max_chunks, int* lanes, int* snake);
int expo_chain_helper_stats(int* probed, int* rejected);
int expo_chain_prepare(void* stream);
int expo_chain_release(void* stream);
int expo_chain_fwd(const int* filter_ids, int steps, void* const* acts,
                   const float* const* params, int n, int h, int w, int dtype,
                   void* stream);

/*
 * Backward of expo_chain_fwd.
 *   grads    host array of steps+1 device image pointers: grads[steps] = upstream
 *            dy (read), grads[i] = gradient w.r.t. acts[i] (written).  Entries may
 *            ping-pong between two buffers as long as grads[i] != grads[i+1] is not
 *            required (dx may alias dy).
 *   dparams  host array of `steps` device pointers, float32 [N][P_i], overwritten.
 *   workspace_bytes >= steps * expo_workspace_bytes(n, h, w, dtype): every step keeps its block
 *   records until the ONE finish launch at the end of the chain has produced all dparams.
 *   acts     must be what the forward made: acts[i + 1] = filter filter_ids[i] with params[i] applied to
 *            acts[i], as expo_chain_fwd (or expo_filter_fwd step by step) leaves them.  Consecutive
 *            element-wise steps run as one launch that loads only the LOWEST step's activation and
 *            recomputes the ones above it in registers, bit for bit, so the interior
 *            acts[i] of such a run are NOT read.  A caller that edits activations between the forward
 *            and the backward sets EXPO_CHAIN_BWD_RECOMPUTE=0 in the environment (read once per
 *            process): every step then reads its acts[i], with the same results for unedited ones.
 *
 * A run whose filter ids, storage type and hsv_grad_mode are in the library's table of compiled sequences (the
 * reference's filter order: Saturation+, White balance, Gamma, Exposure from the run's head down)
 * goes to a kernel compiled for exactly that sequence, with the same launch count and bit-identical results.
 * EXPO_CHAIN_BWD_SEQ=0 in the environment (read once per process) keeps the general kernels for every run.
 * expo_chain_bwd_seq_launches() returns how many run launches of this process went to a compiled sequence (one per
 * run and lane; diagnostics -- nothing else tells the two kernels apart).
 */
int expo_chain_bwd(const int* filter_ids, int steps, void* const* acts,
                   void* const* grads, const float* const* params,
                   float* const* dparams, int n, int h, int w, int dtype,
                   int hsv_grad_mode, void* workspace, size_t workspace_bytes, void* stream);
long long expo_chain_bwd_seq_launches(void);

/*
 * Fused multi-step forward for the high-resolution inference path (net.py:796-821, evaluate.py:8-31):
 * the agent regresses every step's parameters on the 64x64 proxy, so the per-image sequence
 * (filter id, parameters) x steps is known before the full-resolution image is touched.  All
 * `steps` filters are applied while a pixel group sits in registers (fp32 between steps): one
 * read and one write of the image instead of `steps` of each.
 *   filter_ids  device int32 [N][steps] in [-1, 8]   (-1: the image becomes 0 from that step on)
 *   params      device float32 [N][steps][EXPO_MAX_PARAMS], row = packed params of that step's filter
 */
int expo_chain_fused_fwd(const int32_t* filter_ids, const float* params, int steps,
                         const void* x, void* y, int n, int h, int w, int dtype, void* stream);

/*
 * (ABI 9) expo_chain_fused_fwd over a LIST of n images of any sizes, in one launch (several for n > 64: the table of
 * images travels in the kernel arguments, 64 per launch, all on `stream` in order).  Every output is bit-identical to
 * expo_chain_fused_fwd on that image alone (same step loop; only cache bits and addressing differ).
 *   filter_ids  device int32 [n][steps] in [-1, 8], params device float32 [n][steps][EXPO_MAX_PARAMS]: as above
 *   xs, ys      HOST arrays of n device image pointers (NHWC, 3 channels, `dtype` storage; as the pointer arrays of
 *               expo_chain_bwd); image i has hs[i] x ws[i] pixels (host arrays).  Outputs must not overlap any image
 *               of the call but their own input.
 * Everything is validated before anything is enqueued: every image as expo_chain_fused_fwd's one (h, w >= 1, smaller
 * than 2 GiB), steps in [0, 64], no null pointer; n == 0 is a no-op.  Per image the dwordx3 path is taken when its
 * pixel count is whole 12-byte vectors and both bases are 4-byte aligned (else element-wise); the streaming cache
 * policy when the whole call moves at least EXPO_STREAM_MIN_BYTES.
 */
int expo_chain_fused_fwd_ragged(const int32_t* filter_ids, const float* params, int steps,
                                const void* const* xs, void* const* ys, const int* hs, const int* ws,
                                int n, int dtype, void* stream);

/*
 * Taps: expo_chain_fused_fwd / _ragged that also write the running image after chosen steps (the step-by-step
 * pictures of net.py:820-823, evaluate.py:31), from the same pass -- the image between steps is never read back.
 * Added exports of ABI 9 (the version is unchanged).
 *   tap_mask    bit k set: write the image after step k (k < steps).  Tap j is the j-th set bit, T = popcount.
 *   tap_format  EXPO_TAP_STORAGE: the storage dtype, bit-identical to what expo_chain_fused_fwd writes for the
 *               truncated sequence filter_ids[:, :k+1].
 *               EXPO_TAP_U8: uint8 = saturate_[0,255](round_half_even(float(s) * 255.0f)), s the value rounded to the
 *               storage dtype first: the reference's 8-bit PNG value (cv2.imwrite(img * 255), net.py:769-772).  A NaN
 *               pixel gives an unspecified byte, as everywhere on the inference path.
 *               EXPO_TAP_U16: uint16 = saturate_[0,65535](round_half_even(float(s) * 65535.0f)), s as for U8: one IEEE
 *               fp32 multiply, then the rounding, then the clamp.  Little-endian, 6 B/px: a plane is byte for byte the
 *               payload of an uncompressed 16-bit RGB TIFF.  With EXPO_F16 storage s has fp16's 11 significant bits, so
 *               the picture has them too; the full 16-bit depth needs EXPO_F32 storage.
 *   taps        dense: ONE device buffer [T][N][H][W][3], tap-major; ragged: a HOST array of n device buffers,
 *               image i's [T][hs[i]][ws[i]][3].  A uint8 plane may start at any byte, a uint16 plane at any 2-byte
 *               boundary (EXPO_F16 storage: a plane that is not 4-byte aligned sends its image down the element-wise
 *               path, as an unaligned x or y does).
 *   y / ys      may be NULL (only taps are written: the 8-bit preview writes 3 B/px instead of the image's 6 B/px);
 *               ys may be NULL as a whole array, not per image.
 * Validated before anything is enqueued: as the calls without taps, plus tap_mask bits < steps, tap_format one of the
 * three, taps (and every taps[i]) non-NULL when tap_mask != 0, and y / ys NULL with tap_mask == 0 is EXPO_E_BADARG
 * ("nothing to write").  tap_mask == 0 with y / ys given is exactly the call without taps.
 */
#define EXPO_TAP_STORAGE 0
#define EXPO_TAP_U8 1
#define EXPO_TAP_U16 3
int expo_chain_fused_fwd_taps(const int32_t* filter_ids, const float* params, int steps, const void* x, void* y,
                              int n, int h, int w, int dtype, uint64_t tap_mask, int tap_format, void* taps,
                              void* stream);
int expo_chain_fused_fwd_ragged_taps(const int32_t* filter_ids, const float* params, int steps,
                                     const void* const* xs, void* const* ys, const int* hs, const int* ws, int n,
                                     int dtype, uint64_t tap_mask, int tap_format, void* const* taps, void* stream);

/*
 * The fused inference pass with the reference's spatial masks (cfg.masking, filters.py:110-148): an added export of
 * ABI 9 (the version is unchanged), modelled on expo_chain_fused_fwd_ragged_taps.  For image i, v_0 = float(x_i) and
 * for k = 0 .. steps-1, per pixel (row, col):
 *   id -1:      v_{k+1} = +0
 *   otherwise:  m = the mask of expo_filter_apply_dispatch_fwd for mask_params[i][k] at (row, col) with the luminance
 *               of v_k, on the grid of an hs[i] x ws[i] image;  v_{k+1} = fma(m, process_id(v_k) - v_k, v_k) per channel
 * fp32 between steps, one rounding to storage at the end (the per-step schedule rounds after every step).
 *   mask_params  device float32 [n][steps][6]: tanh_range(-5, 5)(raw) of the step's selected filter, as
 *                expo_filter_apply_dispatch_fwd takes them; maximum_sharpness / minimum_strength as there
 *   tap_mask, tap_format, taps, ys NULL: exactly as expo_chain_fused_fwd_ragged_taps (tap_mask 0: no taps, taps may
 *                be NULL)
 * Launches, the per-image choice of the dwordx3 path, the cache policy and the validation are those of
 * expo_chain_fused_fwd_ragged_taps, plus mask_params non-NULL when steps > 0.  Every output is bit-identical to the
 * same image passed alone.
 */
int expo_chain_fused_masked_fwd_ragged(const int32_t* filter_ids, const float* params, const float* mask_params,
                                       int steps, float maximum_sharpness, float minimum_strength,
                                       const void* const* xs, void* const* ys, const int* hs, const int* ws, int n,
                                       int dtype, uint64_t tap_mask, int tap_format, void* const* taps, void* stream);

/*
 * The fused inference pass for any cfg.curve_steps: an added export of ABI 9 (the version is unchanged).  It replaces
 * the high-resolution loop of net.py:796-823 with the curves of filters.py:264-273, 312-322 for any L, where
 * expo_chain_fused_fwd_ragged_taps is built for L = 8.
 *   filter_ids   device int32 [n][steps] in [-1, 8]
 *   params       device float32 [n][steps][EXPO_MAX_PARAMS_CURVES].  Ids 0, 1, 2, 3, 5, 6, 8 keep their packing at the
 *                front of the row (at most 3 values); Tone (4) holds k_0 .. k_{L-1}; Color (7) holds channel * L + knot
 *                (ColorFilter.pack for that L).  Entries a filter does not use never enter arithmetic.
 *   curve_steps  L in [1, EXPO_CURVE_MAX_STEPS], one value for the call.  Ids 4 and 7 evaluate, per channel value x,
 *                  y = (L/S) sum_i clip(x - i/L, 0, 1/L) k_i,  S = sum_i k_i + 1e-30
 *                through the segment form of expo_curve_fwd: x^ = clamp(x, 0, 1), j = min(int(x^ L), L - 1).
 *                L = 8 is allowed (the curve steps then differ from expo_chain_fused_fwd_ragged_taps in rounding only).
 * Everything else -- fp32 between steps and one rounding to storage at the end, id -1 -> +0, steps == 0 -> the input's
 * bits, xs / ys / hs / ws, the launches of up to 64 images, the per-image choice of the dwordx3 path, the cache policy
 * from the call's total bytes, tap_mask / tap_format / taps, ys NULL with taps, and the validation -- is exactly
 * expo_chain_fused_fwd_ragged_taps; a sequence without ids 4 and 7 gives that entry point's bits.  curve_steps outside
 * its range is EXPO_E_BADARG; n == 0 is EXPO_OK.  No backward.
 */
int expo_chain_fused_curves_fwd_ragged(const int32_t* filter_ids, const float* params, int steps, int curve_steps,
                                       const void* const* xs, void* const* ys, const int* hs, const int* ws, int n,
                                       int dtype, uint64_t tap_mask, int tap_format, void* const* taps, void* stream);

/*
 * The fused inference pass for any cfg.curve_steps straight from the integer codes: an added export of ABI 9 (the
 * version is unchanged).  It replaces expo_decode_ragged followed by expo_chain_fused_curves_fwd_ragged -- and with them
 * the decoded float input, which is never written or re-read -- as expo_chain_fused_fwd_ragged_codes replaces
 * expo_decode_ragged + expo_chain_fused_fwd_ragged_taps for L = 8.  Every result is bit-identical to that pair.
 *   filter_ids, params, steps, curve_steps        as expo_chain_fused_curves_fwd_ragged: params is device float32
 *                                                 [n][steps][EXPO_MAX_PARAMS_CURVES], curve_steps = L one value per call
 *   codes, channels, code_bits, tables, table_stride   as expo_chain_fused_fwd_ragged_codes (below): image i's input is
 *                                                 codes[i] plus its table at entry i * table_stride, in `dtype`; a
 *                                                 pixel value enters the step loop as float(cast table value)
 *   ys, hs, ws, n, dtype, tap_mask, tap_format, taps   as both: tap_mask == 0 is allowed (taps may be NULL), ys NULL is
 *                                                 allowed with taps, ys NULL with tap_mask == 0 is EXPO_E_BADARG
 * 64 images per launch by value in the kernel arguments, more as further launches on `stream`; per image the vector path
 * under the rule of expo_chain_fused_fwd_ragged_codes; the cache policy from the call's total bytes.  Validated before
 * anything is enqueued (EXPO_E_BADARG / EXPO_E_BADDTYPE), the union of the two: curve_steps in [1, EXPO_CURVE_MAX_STEPS],
 * channels 1, 3 or 4, code_bits 8 or 16, table_stride 0 or >= 2^code_bits, tables non-NULL and 4-byte aligned, steps in
 * [0, 64], the taps' arguments, no null pointer and no null per-image pointer, the codes of one image smaller than
 * 2 GiB; n == 0 is a no-op.  No backward, no spatial masks.
 */
int expo_chain_fused_curves_fwd_ragged_codes(const int32_t* filter_ids, const float* params, int steps, int curve_steps,
                                             const void* const* codes, int channels, int code_bits, const void* tables,
                                             int table_stride, void* const* ys, const int* hs, const int* ws, int n,
                                             int dtype, uint64_t tap_mask, int tap_format, void* const* taps,
                                             void* stream);

/*
 * Decode: the integer codes of n input images, as the file holds them, to the linear storage tensors that
 * evaluate.load_image + .to(dtype) gives (net.py:726-747).  Added exports of ABI 9 (the version is unchanged).
 *   codes      HOST array of n device pointers; image i is hs[i] x ws[i] x channels codes, uint8 (code_bits 8) or
 *              uint16 (16), NHWC.  channels 1, 3 or 4; a pointer may start at any byte (uint8) / element (uint16).
 *   table      device float32 [2^code_bits], non-decreasing (the caller's contract): the linearisation of every code.
 *   outs       HOST array of n device pointers, image i's [hs[i]][ws[i]][3] in `dtype`.  With k the code of output
 *              channel c (channel 0 when channels == 1, channel c otherwise: the alpha channel is ignored):
 *                normalize 0:  out = cast(table[k])
 *                normalize 1:  out = cast(fl32(table[k] / fl32(2 table[m_i]))), m_i the largest code of image i over
 *                              the channels that reach the output; an image of all-zero codes gives NaN everywhere.
 *              cast rounds to nearest even; the division is the IEEE float32 one.
 *   workspace  normalize 1 only: caller-owned, 4-byte aligned device scratch of at least expo_decode_workspace_bytes
 *              (n, hs, ws, channels, code_bits) bytes, no initialisation, nothing carried between calls (one record of
 *              the largest code per block, then a finish launch writes every image's normalised table into it).
 *              Ignored with normalize 0.
 * Three launches per 64 images with normalize 1, one without; larger n is split into launches of 64 on `stream`.
 * Everything is validated before anything is enqueued (EXPO_E_BADARG / EXPO_E_BADDTYPE): no null pointer, channels,
 * code_bits and normalize in range, h, w >= 1, an output and the codes of one image smaller than 2 GiB, the
 * workspace; n == 0 is a no-op.  expo_decode_workspace_bytes is 0 for invalid arguments.
 */
size_t expo_decode_workspace_bytes(int n, const int* hs, const int* ws, int channels, int code_bits);
int expo_decode_ragged(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                       const float* table, int normalize, void* const* outs, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);

/*
 * Inference straight from the integer codes: the decode is a table gather, so its consumers can gather at load time
 * and the decoded float tensor need not exist.  Added exports of ABI 9 (the version is unchanged); every result is
 * bit-identical to expo_decode_ragged followed by the export that takes tensors.
 *
 * expo_decode_tables: the tables expo_decode_ragged uses internally, written into a caller-owned buffer in `dtype`.
 *   codes, hs, ws, n, channels, code_bits, table, normalize, workspace, workspace_bytes: as expo_decode_ragged
 *   (normalize 0 reads no codes: codes, hs and ws may be NULL; the workspace is sized by expo_decode_workspace_bytes).
 *   tables     device buffer, 4-byte aligned, of at least expo_decode_tables_bytes(n, code_bits, normalize, dtype) bytes:
 *                normalize 1:  n tables, image i's at entry i * 2^code_bits: cast(fl32(table[k] / fl32(2 table[m_i]))),
 *                              the records, the division and the cast of expo_decode_ragged (alpha not counted).  An image
 *                              of all-zero codes (2 table[m_i] == 0) gives a table of NaN in every entry: the entries
 *                              its codes read are 0 / 0 as there, and the others, which no code of the image reads,
 *                              are NaN too instead of table[k] / 0;
 *                normalize 0:  ONE shared table cast(table[k]).
 * Returns the stride between consecutive images' tables in ENTRIES (2^code_bits; 0 = one shared table, and for n == 0,
 * a no-op), or a negative EXPO_E_* code.  Everything is validated before anything is enqueued, as expo_decode_ragged
 * does, plus the tables buffer.  expo_decode_tables_bytes is 0 for invalid arguments.
 *
 * expo_bilinear_resize_ragged_codes: expo_bilinear_resize_ragged with the windows read from codes: the same windows, S
 * and individually rounded float32 arithmetic; a tap is float(tables_i[code]), tables in table_dtype.  channels 1 (the
 * grey channel is replicated), 3 or 4 (alpha is dropped); a code pointer may sit at any byte (uint8) / element (uint16).
 *   tables, table_stride  what expo_decode_tables wrote and returned: image i's table at entry i * table_stride.
 * Validated as expo_bilinear_resize_ragged, plus channels, code_bits, table_stride (0 or >= 2^code_bits) and tables.
 *
 * expo_chain_fused_fwd_ragged_codes: expo_chain_fused_fwd_ragged_taps with image i's input given as codes[i] plus its
 * table (in `dtype`, the storage dtype of ys and of storage taps): a pixel value enters the step loop as
 * float(cast table value), what the decoded tensor would hold.  tap_mask == 0 is allowed (no taps; taps may be NULL);
 * ys NULL is allowed with taps; ys NULL with tap_mask == 0 is EXPO_E_BADARG.  Every tap_format of the sibling.  64
 * images per launch by value in the kernel arguments, more as further launches on `stream`.  Per image the vector path is
 * taken when the codes, y and a vector-stored tap plane are 4-byte aligned and the pixel count is whole 12-byte vectors
 * (else element-wise).  Validated before anything is enqueued: as the sibling, plus channels, code_bits, table_stride,
 * tables non-NULL and 4-byte aligned, and the codes of one image smaller than 2 GiB; n == 0 is a no-op.
 */
size_t expo_decode_tables_bytes(int n, int code_bits, int normalize, int dtype);
int expo_decode_tables(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                       const float* table, int normalize, void* tables, size_t tables_bytes, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);
int expo_bilinear_resize_ragged_codes(const void* const* codes, const int* hs, const int* ws, int n, int channels,
                                      int code_bits, const void* tables, int table_stride, int table_dtype,
                                      const int32_t* windows, int q, int S, void* out, int out_dtype, void* stream);
int expo_chain_fused_fwd_ragged_codes(const int32_t* filter_ids, const float* params, int steps,
                                      const void* const* codes, int channels, int code_bits, const void* tables,
                                      int table_stride, void* const* ys, const int* hs, const int* ws, int n, int dtype,
                                      uint64_t tap_mask, int tap_format, void* const* taps, void* stream);

/*
 * The input pictures from the integer codes.  Added exports of ABI 9 (the version is unchanged).
 *
 * expo_codes_max_ragged: maxima[i] (device int32 [n]) = the largest code of image i over the channels that reach the
 * output (alpha ignored; the one channel when channels == 1): the m_i expo_decode_ragged normalises by.
 *   workspace  caller-owned, 4-byte aligned device scratch of at least expo_decode_workspace_bytes(...) bytes.
 * Validated before anything is enqueued, as expo_decode_ragged with normalize 1; n == 0 is a no-op.
 *
 * expo_codes_lut_ragged: outs[i][p][c] = luts[i * lut_stride + code_i(p, c)] for the 3 output channels (grey is
 * replicated, alpha is dropped).
 *   luts       device array of uint8 (out_bits 8) or uint16 (out_bits 16) entries; with out_bits 16, 2-byte aligned.
 *   lut_stride 0 (one shared table) or at least 2^code_bits entries between consecutive images' tables.
 *   outs       HOST array of n device pointers to [hs[i]][ws[i]][3] integers of out_bits.
 * A code pointer may start at any byte (uint8) or element (uint16), and so may an output pointer.  Per image the vector
 * path is taken when codes and output are 4-byte aligned and the pixel count is a multiple of 4 (else element-wise).
 * 8-bit tables are staged in LDS.  16-bit codes with uint8 entries and 16-byte aligned tables stage their 64 KiB table
 * in LDS too; every other 16-bit case reads the table through the caches.  The environment variable
 * EXPO_CODES_LUT_LDS16, read at every call, set to 0 makes all 16-bit codes read through the caches (1 or unset: the
 * default above); the values written are the same.  64 images
 * per launch, more as further launches on `stream`.  Everything is validated before anything is enqueued; n == 0 is a no-op.
 */
int expo_codes_max_ragged(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                          int32_t* maxima, void* workspace, size_t workspace_bytes, void* stream);
int expo_codes_lut_ragged(const void* const* codes, const int* hs, const int* ws, int n, int channels, int code_bits,
                          const void* luts, int lut_stride, int out_bits, void* const* outs, void* stream);

/*
 * 8-bit PNG files made on the device (png_encode.hip): the file show_and_save writes with cv2.imwrite
 * (net.py:769-772), without a host compressor.  Added exports of ABI 9 (the version is unchanged).
 *
 * The file: signature; IHDR (bit depth 8, colour type 2, no interlace); one IDAT with the zlib header 78 01; one IDAT
 * per segment of SEG bytes of the filtered stream (row r: one type byte, then its 3 w filtered bytes, bpp = 3); one
 * IDAT with the stream's Adler-32; IEND.  A segment is deflated on its own and ends on a byte boundary: one dynamic
 * Huffman block of literals only (HLIT 0, HDIST 0 with the unused distance code of length 1, HCLEN 15 with the fixed
 * code-length code "0..15 have length 4", so a header of 1106 bits; lengths from a Huffman construction over the
 * segment's bytes and one end-of-block, limited to 15 bits, canonical codes), followed by an empty stored block (zlib's
 * sync flush) unless it is the last, which sets BFINAL; or one stored block, exactly when the dynamic form is not
 * smaller.  No LZ77 matches.  The bytes depend on the picture and `filter` alone.
 *
 * expo_png_segment_bytes (net.py:769-772): SEG, a compile-time constant, 16384 <= SEG <= 65535.
 * expo_png_encode_bound (net.py:769-772): the largest file of an h x w picture, 75 + 17 ceil(S / SEG) + S with
 *   S = h (1 + 3 w); reached exactly by incompressible pictures.  -1 (with a message) when h or w is below 1 or
 *   S >= 2^31.
 * expo_png_encode_workspace_bytes (net.py:769-772): the scratch a call on these n pictures needs (0 for invalid
 *   arguments): per picture of a launch group its row types, a slot of SEG + 32 bytes and 24 bytes per segment.
 * expo_png_encode_ragged (net.py:769-772):
 *   pics         HOST array of n device pointers, picture i is contiguous [hs[i]][ws[i]][3] uint8, any alignment.
 *   filter       0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth for every row; 5 adaptive: per row the type with the smallest
 *                sum of min(b, 256 - b) over its filtered bytes (libpng's heuristic), ties to the lowest type.
 *   outs         HOST array of n device pointers to byte buffers, any alignment; out_capacity HOST [n], each at least
 *                expo_png_encode_bound(hs[i], ws[i]).  File i is outs[i][0 .. sizes[i]).
 *   sizes        DEVICE int64 [n]: the files' lengths.
 *   workspace    caller-owned, 16-byte aligned device scratch of at least expo_png_encode_workspace_bytes(...) bytes;
 *                needs no initialisation and carries no state.
 * Allocates nothing, does not synchronise with the host, can be captured.  64 pictures per launch group (four launches,
 * three with a fixed filter), more as further groups on `stream`.  Everything is validated before anything is enqueued
 * (EXPO_E_BADARG: n < 0, filter outside 0..5, h or w below 1, S >= 2^31, a capacity below the bound, a workspace that
 * is too small, null pointers); n == 0 is a no-op.
 */
int expo_png_segment_bytes(void);
int64_t expo_png_encode_bound(int h, int w);
size_t expo_png_encode_workspace_bytes(const int* hs, const int* ws, int n);
int expo_png_encode_ragged(const void* const* pics, const int* hs, const int* ws, int n, int filter, void* const* outs,
                           const int64_t* out_capacity, int64_t* sizes, void* workspace, size_t workspace_bytes,
                           void* stream);

/*
 * Baseline JPEG files made on the device (jpeg_encode.hip): the photographer's deliverable of the
 * pictures show_and_save writes (net.py:769-772), without a host encoder.  Added exports of ABI 9 (the version is
 * unchanged).
 *
 * The file (DESIGN.md §3.34 fixes every byte): SOI; APP0 JFIF 1.01, density 1 x 1; DQT 0 and 1 (T.81 Annex K.1 / K.2
 * scaled by `quality` as libjpeg does, 8-bit, zigzag order); SOF0 (precision 8, three components, Y sampled 1 x 1 for
 * subsampling 0 and 2 x 2 for subsampling 2); the four DHT of Annex K.3 - K.6; DRI; SOS; the restart intervals; EOI.
 * The header is 629 bytes.  Colour: the JFIF integer matrix in 16-bit fixed point; planes extended to whole MCUs by
 * edge replication; 4:2:0 chroma is the rounded mean of 2 x 2.  Transform: two 8-point passes with the 13-bit cosine
 * table of csrc/jpeg_codec.h, everything in int32.  An interval is Ri MCUs in raster order, coded on its own with the
 * DC predictors at 0, padded to a byte with 1-bits, 0xFF stuffed, followed by RSTm (m = k mod 8) unless it is the last.
 * The bytes depend on the picture, `quality` and `subsampling` alone.
 *
 * expo_jpeg_restart_mcus (net.py:769-772): Ri of a sampling, a compile-time constant (16 and 8: 48 blocks either way); -1 (with a message)
 *   for a subsampling other than 0 (4:4:4) and 2 (4:2:0).
 * expo_jpeg_encode_bound (net.py:769-772): a proved upper bound of the file's length: 629 + per interval of m MCUs of
 *   B blocks (3 or 6) 2 ceil(1660 m B / 8) + 2 -- a block is at most 22 + 63 * 26 = 1660 bits, stuffing at most doubles
 *   the padded bytes, and two bytes of marker follow.  -1 (with a message) when h or w is outside 1..65535.
 * expo_jpeg_encode_workspace_bytes (net.py:769-772): the scratch a call on these n pictures needs (0 for invalid
 *   arguments): per picture of a launch group 16 bytes, and 4 + 8 bytes per interval, each piece rounded up to 16.
 * expo_jpeg_encode_ragged (net.py:769-772):
 *   pics         HOST array of n device pointers, picture i is contiguous [hs[i]][ws[i]][3] uint8 RGB, any alignment.
 *   quality      1..100; subsampling 0 (4:4:4) or 2 (4:2:0).
 *   outs         HOST array of n device pointers to byte buffers, any alignment; out_capacity HOST [n], each >= 0.
 *                File i is written iff sizes[i] <= out_capacity[i], as outs[i][0 .. sizes[i]); otherwise not one byte
 *                of outs[i] is written.  A capacity of expo_jpeg_encode_bound makes that impossible.
 *   sizes        DEVICE int64 [n]: the files' true lengths, whatever the capacities.
 *   workspace    caller-owned, 16-byte aligned device scratch of at least expo_jpeg_encode_workspace_bytes(...) bytes;
 *                needs no initialisation and carries no state.
 * Allocates nothing, does not synchronise with the host, can be captured.  64 pictures per launch group (three
 * launches), more as further groups on `stream`.  Everything is validated before anything is enqueued (EXPO_E_BADARG:
 * n < 0, quality outside 1..100, a subsampling other than 0 and 2, h or w outside 1..65535, a negative capacity, a
 * workspace that is too small or misaligned, null pointers); n == 0 is a no-op.
 */
int expo_jpeg_restart_mcus(int subsampling);
int64_t expo_jpeg_encode_bound(int h, int w, int subsampling);
size_t expo_jpeg_encode_workspace_bytes(const int* hs, const int* ws, int n, int subsampling);
int expo_jpeg_encode_ragged(const void* const* pics, const int* hs, const int* ws, int n, int quality, int subsampling,
                            void* const* outs, const int64_t* out_capacity, int64_t* sizes, void* workspace,
                            size_t workspace_bytes, void* stream);

/*
 * Baseline JPEG input files decoded on the device (jpeg_decode.hip): the (H, W, 3) uint8 codes that the
 * reference's readers hand to the network (net.py:739; folder_data_provider.py's cv2.imread), bit for bit what PIL's
 * open + convert('RGB') makes of the file, without a host codec.  Added exports of ABI 9 (the version is unchanged).
 *
 * The picture (DESIGN.md §3.35 fixes every value): T.81 §F.2.2 entropy decoding with any table of up to 256 symbols and
 * code lengths 1..16, DC predictors 0 at the start of every restart interval; d = coefficient * Q; libjpeg's "islow"
 * inverse transform with 13-bit constants (columns with descale shift 11, rows with 18, + 128, clamped), in wrapping
 * int32; component planes of their real samples; libjpeg's triangle-filter chroma upsampling with indices clamped to
 * the real plane; the JFIF integer colour matrix in 16-bit fixed point.  sampling is PIL's number: 0 = 4:4:4 (Y 1 x 1),
 * 1 = 4:2:2 (Y 2 x 1), 2 = 4:2:0 (Y 2 x 2), Cb and Cr 1 x 1; ncomps 1 (grey, sampling 0, Y replicated) or 3.  A segment
 * is a restart interval (a file without DRI is one segment).
 *
 * The plan of a picture is a device blob the host builds from the file's header (exposure_amd/jpeg_decode.py: parse),
 * little endian, 16-byte aligned:
 *   0     int32 ri            MCUs per restart interval, 0 without DRI
 *   4     uint8 tq[4], 8 uint8 td[4], 12 uint8 ta[4]   per component its quantiser, DC and AC table
 *   16    uint8 q[4][64]      the quantiser tables, natural order
 *   272   4 x 384 bytes       the Huffman tables DC 0, DC 1, AC 0, AC 1, each uint32 limit[16] (limit[l - 1] =
 *                             (MAXCODE(l) + 1) << (16 - l); for a length without codes the limit before it, 0 before the
 *                             first), int32 offs[16] (VALPTR(l) - MINCODE(l)), uint8 vals[256] (HUFFVAL)
 *   1808  int32 seg[nsegs][2] the byte range [begin, end) of every segment's stuffed bytes in the file
 * The kernels trust none of it for addressing: every read is clamped to the file's length, every write to the lane's
 * own blocks, every loop is bounded by the geometry given here on the host.
 *
 * expo_jpeg_decode_plan_bytes (net.py:739; folder_data_provider.py's cv2.imread): 1808 + 8 nsegs rounded up to 16; 0
 *   for nsegs < 1.
 * expo_jpeg_decode_workspace_bytes (net.py:739; folder_data_provider.py's cv2.imread): the scratch a call on these n
 *   pictures needs (0 for invalid arguments): per picture of a launch group 128 bytes per block and its component planes
 *   (real rows of whole blocks across), each piece rounded up to 16; the largest launch group's sum.
 * expo_jpeg_decode_ragged (net.py:739; folder_data_provider.py's cv2.imread):
 *   files        HOST array of n device pointers to the files' bytes, any alignment; file_bytes HOST [n], 0..2^31-1.
 *   plans        HOST array of n device pointers to the plans, 16-byte aligned, expo_jpeg_decode_plan_bytes(nsegs[i]) bytes.
 *   hs, ws, samplings, ncomps, nsegs   HOST [n]: the geometry from the file's header; nsegs[i] = ceil(mcus / Ri).
 *   outs         HOST array of n device pointers, picture i contiguous [hs[i]][ws[i]][3] uint8 RGB, any alignment.
 *   status       DEVICE int32 [n], written for every picture: 0, or an OR of 1 (TRUNCATED: a segment consumed more bits
 *                than it has), 2 (BAD_CODE: 16 bits matched no code, or a DC category above 15) and 4 (BAD_RUN: a run
 *                stepped past coefficient 63).  On an error the lane stops and the rest of its segment's blocks are
 *                all-zero coefficients; the picture's pixels are unspecified; its other segments still decode.
 *   workspace    caller-owned, 16-byte aligned device scratch of at least expo_jpeg_decode_workspace_bytes(...) bytes;
 *                needs no initialisation and carries no state.
 * Allocates nothing, does not synchronise with the host, can be captured.  One memset node for `status`, then three
 * launches per group of 64 pictures, more as further groups on `stream`.  Everything is validated before anything is
 * enqueued (EXPO_E_BADARG: n < 0, h or w outside 1..65535, a sampling other than 0, 1 and 2, ncomps other than 1 and 3
 * or grey with a sampling other than 0, nsegs that is ceil(mcus / Ri) for no Ri >= 1, file_bytes outside 0..2^31-1, a
 * misaligned plan, a workspace that is too small or misaligned, null pointers); n == 0 is a no-op.
 */
size_t expo_jpeg_decode_plan_bytes(int nsegs);
size_t expo_jpeg_decode_workspace_bytes(const int* hs, const int* ws, const int* samplings, const int* ncomps, int n);
int expo_jpeg_decode_ragged(const void* const* files, const int64_t* file_bytes, const void* const* plans, const int* hs,
                            const int* ws, const int* samplings, const int* ncomps, const int* nsegs, int n,
                            void* const* outs, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Baseline JPEG files without restart markers decoded in parallel on the device (jpeg_decode_sync.hip):
 * the pictures and status words of expo_jpeg_decode_ragged, for every input, with the entropy walk of a one-segment
 * file spread over a lane per subsequence.  Added exports of ABI 9 (the version is unchanged).
 *
 * Subsequence i of the segment [begin, end) of a file without DRI is its bytes [begin + i sub_bytes, min(begin + (i + 1)
 * sub_bytes, end)).  Every subsequence is walked from a speculative entry state (bit offset, block in the MCU,
 * coefficient index); the lanes then take the exit of the subsequence before them as their entry and walk again until
 * nothing changes (rounds inside a workgroup of 256 subsequences, then grid_rounds further launches that carry the last
 * exit of a workgroup to the next).  The chain in[0] = the exact start, in[i] = out[i - 1] is verified on the device;
 * a verified picture's coefficients are stored by a second walk, a picture whose chain is not verified is decoded by the
 * one-lane walk of expo_jpeg_decode_ragged inside the same call.
 *
 * expo_jpeg_decode_sync_workspace_bytes (net.py:739; folder_data_provider.py's cv2.imread): the scratch a call on these n
 *   pictures needs (0 for invalid arguments): expo_jpeg_decode_workspace_bytes' layout per launch group, then per
 *   picture with nsegs 1 and nsubs > 1 two state words, a 16-byte payload and 16 bytes of first block and predictors per
 *   subsequence, two boundary words per 256 subsequences and 16 bytes of results, each piece rounded up to 16.
 * expo_jpeg_decode_sync_ragged (net.py:739; folder_data_provider.py's cv2.imread): the arguments of
 *   expo_jpeg_decode_ragged, and
 *   nsubs        HOST [n]: max(1, ceil(bytes of the segment / sub_bytes)) of a picture with nsegs 1, and 1 for the others.
 *                The device clamps to the segment: a wrong count addresses nothing outside the file or the workspace, and
 *                its picture is decoded by the one-lane walk.
 *   sub_bytes    a multiple of 16 in 32..65536.
 *   grid_rounds  0..16: the settle launch runs once and then grid_rounds times more.
 *   info         DEVICE int32 [n] or null, written for every picture: 0 a lane per segment (restart intervals, or one
 *                subsequence), 1 decoded through verified subsequences, 2 the chain was not verified and the serial lane
 *                decoded it.
 * outs and status are expo_jpeg_decode_ragged's for every file whose segment has a 00 behind every FF (every plan the
 * host parser makes).  Allocates nothing, does not synchronise with the host, can be captured.  A memset node each for
 * `status` and `info`, then per group of 64 pictures 1 + grid_rounds settle launches, the scan, a memset node over the
 * sync pictures' coefficients, the emit, the serial launch and the two reconstruction launches.  The workspace needs no
 * initialisation and carries no state.  Everything is validated before anything is enqueued (EXPO_E_BADARG: the cases of
 * expo_jpeg_decode_ragged, sub_bytes that is no multiple of 16 in 32..65536, grid_rounds outside 0..16, nsubs outside
 * 1..2^26, nsubs other than 1 for a picture with nsegs > 1); n == 0 is a no-op.
 */
size_t expo_jpeg_decode_sync_workspace_bytes(const int* hs, const int* ws, const int* samplings, const int* ncomps,
                                             const int* nsegs, const int* nsubs, int n);
int expo_jpeg_decode_sync_ragged(const void* const* files, const int64_t* file_bytes, const void* const* plans, const int* hs,
                                 const int* ws, const int* samplings, const int* ncomps, const int* nsegs, const int* nsubs,
                                 int n, int sub_bytes, int grid_rounds, void* const* outs, int32_t* status, int32_t* info,
                                 void* workspace, size_t workspace_bytes, void* stream);

/*
 * Training sets (datasets.hip): the master pack of a folder of photos and its per-epoch re-cut.  Added exports of
 * ABI 9 (the version is unchanged).
 *
 * expo_area_resize_ragged: q square windows of n linear NHWC images, each resampled to S x S x 3 with OpenCV's
 * INTER_AREA weights (computeResizeAreaTab, per axis, scale = side / S in double; the 2-D weight is the product).
 *   xs         HOST array of n device pointers, image i is [hs[i]][ws[i]][3] in in_dtype (EXPO_F16 / EXPO_F32).
 *   windows    HOST int32 array [q][4]: (image, y0, x0, side); the window is rows y0 .. y0 + side - 1 and columns
 *              x0 .. x0 + side - 1 of its image.
 *   out        device [q][S][S][3] in out_dtype, window k at out[k]; cast from the double sum through float32 with
 *              round-to-nearest-even (fp16 = the fp32 result rounded once more).
 * Every sum runs in a fixed order (no atomics): a window's result is bit-identical run to run and whatever else the
 * call holds.  side == S is the identity; side < S (upscaling) is refused.  64 windows per launch, more as further
 * launches on `stream`.  Validated before anything is enqueued (EXPO_E_BADARG / EXPO_E_BADDTYPE): n, q >= 0, dtypes,
 * no null pointer, h, w >= 1 and one image < 2 GiB, every window inside its image with side >= S and side / S small
 * enough for one LDS tile (side <= 4094 S); q == 0 is a no-op.
 *
 * expo_pack_recut: out[r] = flip_r(master[src_r][oy_r : oy_r + C, ox_r : ox_r + C]) for r < count, a copy in one
 * dtype.  master device [m][S][S][3]; records DEVICE int32 [count][4] = (src, oy, ox, flip != 0); out device
 * [count][C][C][3].  S, C (1 <= C <= S), count, the dtype and the pointers are validated on the host; records out of
 * range are the caller's contract (clamped on the device, so no read leaves the master).  count == 0 is a no-op.
 */
int expo_area_resize_ragged(const void* const* xs, const int* hs, const int* ws, int n, int in_dtype,
                            const int32_t* windows, int q, int S, void* out, int out_dtype, void* stream);
int expo_pack_recut(const void* master, int m, int S, const int32_t* records, int count, int C, void* out, int dtype,
                    void* stream);

/*
 * Proxies (proxy.hip): the agent's low-resolution view of a ragged batch.  An added export of ABI 9 (the version is
 * unchanged).
 *
 * expo_bilinear_resize_ragged: q square windows of n linear NHWC images, each resampled to S x S x 3 with plain
 * bilinear interpolation at half-pixel centres, no antialiasing -- net.py:779 (cv2.resize(get_image_center(hi),
 * (64, 64)), the proxy the agent decides on) and data_provider.py:97, 137 (cv2.resize(img, output_size) without
 * augmentation); the arithmetic is torch's upsample_bilinear2d(align_corners=False, antialias=False), every operation
 * an individually rounded float32 operation, nothing contracted:
 *     scale  = (float)side / (float)S
 *     src(d) = max(scale * ((float)d + 0.5f) - 0.5f, 0.0f)
 *     i0 = (int)src;  i1 = i0 + (i0 < side - 1);  l1 = src - (float)i0;  l0 = 1.0f - l1
 *     v = hl0 * (wl0 * a + wl1 * b) + hl1 * (wl0 * c + wl1 * d)     a, b = row i0 at columns j0, j1; c, d = row i1
 *     out = cast(v), round to nearest even; the taps are widened to float32 first.
 *   xs, hs, ws, windows as for expo_area_resize_ragged (HOST arrays; windows [q][4] = (image, y0, x0, side)).
 *   out        device [q][S][S][3] in out_dtype, window k at out[k].
 * side < S (upscaling) is allowed and side == S is the identity up to the cast.  The call reads 4 S^2 pixels of a
 * window whatever its side.  No atomics, no workspace: a window's result is bit-identical run to run and whatever
 * else the call holds.  64 windows per launch, more as further launches on `stream`.  Validated before anything is
 * enqueued (EXPO_E_BADARG / EXPO_E_BADDTYPE): n, q >= 0, dtypes, no null pointer, h, w >= 1 and one image < 2 GiB,
 * every window inside its image with side >= 1, 1 <= S <= 4096; q == 0 is a no-op.
 */
int expo_bilinear_resize_ragged(const void* const* xs, const int* hs, const int* ws, int n, int in_dtype,
                                const int32_t* windows, int q, int S, void* out, int out_dtype, void* stream);

/*
 * The evaluation metric (metric.hip): histogram_intersection.py's statistics of patches and their histograms.  Added
 * exports of ABI 9 (the version is unchanged).
 *
 * expo_patch_stats: stats[r] = the three statistics of the crop master[src_r][oy_r : oy_r + C, ox_r : ox_r + C].
 *   master     device [m][S][S][3] in dtype (EXPO_F16 / EXPO_F32).
 *   records    DEVICE int32 [count][3] = (src, oy, ox); out of range is the caller's contract (clamped on the device,
 *              so no read leaves the master).
 *   stats      device float32 [count][3], fully overwritten.  Every value is widened to double and clipped to [0, 1];
 *              with l = .27 R + .67 G + .06 B in double:
 *                stats[r][0] = mean(l)
 *                stats[r][1] = 2 sqrt(max(mean(l^2) - mean(l)^2, 0))        (the population std)
 *                stats[r][2] = mean(s),  s = 0 where max == min, else (max - min) / max(den, 1e-12) with
 *                              den = (max + min) / 2 < 0.5 ? max + min : 2 - max - min      (HLS saturation)
 *              each rounded once to float32.  The two luminance sums are taken of l - l0, l0 the crop's first pixel
 *              (the same mean and variance): a constant crop has std exactly 0.
 * One block per record; every sum runs in a fixed order in double (per-thread partials over a fixed pixel assignment,
 * then a fixed LDS tree), no atomics: a row is bit-identical run to run and whatever else the call holds.
 *
 * expo_stat_hist: counts[k][b] = the number of stats[.][k] in bin b of `bins` equal bins over [0, 1], as
 * np.histogram(range=(0, 1)): a float32 v with 0 <= v <= 1 goes to bin min((int)(v * bins), bins - 1) (the product in
 * float32: exact for bins a power of two), anything else (v < 0, v > 1, NaN) is dropped.
 *   stats      device float32 [q][3];  counts  device int32 [3][bins], fully overwritten (q == 0 writes zeros).
 * One block, integer LDS atomics (the counts do not depend on the order).
 *
 * Both validate before anything is enqueued (EXPO_E_BADARG / EXPO_E_BADDTYPE): count, q >= 0, the dtype, 1 <= C <= S,
 * m >= 1, 1 <= bins <= 1024, no null pointer; expo_patch_stats with count == 0 is a no-op.
 */
int expo_patch_stats(const void* master, int m, int S, const int32_t* records, int count, int C, float* stats,
                     int dtype, void* stream);
int expo_stat_hist(const float* stats, int q, int bins, int32_t* counts, void* stream);

/*
 * One-pass backward of the same fixed per-image sequence: dx = d(loss)/dx and every step's parameter
 * gradients from x and dy = d(loss)/dy alone -- ONE read of x and dy, ONE write of dx (18 B/pixel
 * whatever the number of steps); the activations are recomputed in registers and no intermediate
 * image exists.  A benchmark construct (bench.py --workload chain_fused): the reference has no caller
 * for it, because there the parameters of step k+1 depend on the image after step k through the CNN
 * (agent.py:30-125) and the backward has to be step by step (expo_chain_bwd / expo_filter_bwd).
 * Each step is linearised at its input rounded to the storage dtype (exact for fp32 storage; for fp16
 * storage the value the per-step chain stores between its launches); the gradient travels between the
 * steps in fp32.  Tie conventions, hsv_grad_mode and id -1 (the image becomes 0: no gradient reaches
 * the input or the earlier steps, that step's dparams row is 0) as in expo_filter_bwd / the dispatch.
 *   filter_ids  device int32 [N][steps] in [-1, 8],  steps <= EXPO_FUSED_BWD_MAX_STEPS
 *   params      device float32 [N][steps][EXPO_MAX_PARAMS]
 *   dparams     device float32 [N][steps][EXPO_MAX_PARAMS], fully overwritten (unused tail of a row = 0)
 *   dx may alias dy (not x).  workspace: expo_workspace_bytes(...) * steps, as for expo_chain_bwd.
 */
#define EXPO_FUSED_BWD_MAX_STEPS 8
int expo_chain_fused_bwd(const int32_t* filter_ids, const float* params, int steps, const void* x,
                         const void* dy, void* dx, float* dparams, int n, int h, int w, int dtype,
                         int hsv_grad_mode, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Per-image statistics the critic appends as constant feature planes
 * (critics.py:48-62): stats[n] = { mean(lum), variance(lum), mean(sat) } with
 * lum = .27R + .67G + .06B + 1e-5 and
 * sat = (max - min) / (min(max + min, 2 - max - min) + 1e-2) on the [0,1]-clipped image.
 * stats: float32 [N][3], overwritten.
 */
int expo_critic_stats(const void* x, float* stats, int n, int h, int w, int dtype,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * mean_{h,w,c} max(y - 1, 0)^2 per image (agent.py:249-251). penalty: float32 [N].
 */
int expo_overexposure_penalty(const void* y, float* penalty, int n, int h, int w,
                              int dtype, void* workspace, size_t workspace_bytes, void* stream);

/*
 * VignetFilter.apply (filters.py:341-396; defined by the reference, in no cfg.filters).  process() is img * 0
 * (filters.py:351-352), so the filter IS its mask:  y = x * (1 - mask),
 *   mask = sigmoid(((gx*m0)^2 + (gy*m1)^2 + m2 - 5) * maximum_sharpness * m3 / 5) * (m4/5 * .5 + .5)
 * with gx, gy the constant coordinate grid of filters.py:371-380 (the one expo_filter_apply_fwd uses).
 * mask_params: float32 [N][5] = tanh_range(-5, 5)(raw mask parameters) (the squashing stays with the caller, as
 * for expo_filter_apply_fwd).  masking = 0 reproduces cfg.masking = False: mask forced to 1 (filters.py:390-392),
 * i.e. y = 0, dx = 0, dmask_params = 0.  The backward overwrites dx (nullable) and dmask_params [N][5].
 */
int expo_vignet_apply_fwd(const void* x, void* y, const float* mask_params, float maximum_sharpness, int masking,
                          int n, int h, int w, int dtype, void* stream);
int expo_vignet_apply_bwd(const void* x, const void* dy, void* dx, const float* mask_params,
                          float* dmask_params, float maximum_sharpness, int masking, int n, int h, int w,
                          int dtype, void* workspace, size_t workspace_bytes, void* stream);

/*
 * d penalty / d y of expo_overexposure_penalty (what tf.gradients produces for agent.py:249-251 when the
 * penalty is NOT taken from the fused dispatch pass -- cfg.masking or cfg.clamp, agent.py:240-241):
 *   dy[n] = 2 * max(y[n] - 1, 0) * dpenalty[n] / (H*W*3).      dy: [N][H][W][3] dtype, overwritten.
 */
int expo_overexposure_penalty_bwd(const void* y, const float* dpenalty, void* dy, int n, int h, int w,
                                  int dtype, void* stream);

/*
 * Derivatives of expo_critic_stats.  The statistics sit inside the training graph of the reference: the
 * generator's reward flows through critic(fake_output) (net.py:68-90) and the WGAN-GP term takes
 * tf.gradients(inte_logit, [interpolated]) and then differentiates THAT with respect to the critic's weights
 * (net.py:174-194), i.e. a double backward through critics.py:48-73.  With S = the three statistics of one
 * image and J = dS/dx (3 x H*W*3):
 *   expo_critic_stats_bwd   dx  = J^T dstats              first derivative (tf.gradients of critics.py:48-62)
 *   expo_critic_stats_jvp   jv  = J v                     d <dx, v> / d dstats: the path of the double backward
 *                                                         that reaches the critic's weights
 *   expo_critic_stats_hvp   out = d <J^T dstats, v> / dx  the second-order term in the image itself
 * stats: float32 [N][3] as written by expo_critic_stats for the SAME x (the mean luminance is read from it);
 * dstats, jv: float32 [N][3]; v, dx, out: images of x's dtype (the gradients are O(1/(H*W)): use EXPO_F32 images
 * when the values matter -- exposure_amd/critics.py always does).  TF conventions: population variance
 * (tf.nn.moments), reduce_max / reduce_min split the gradient evenly between tied channels, clip_by_value
 * passes on 0 <= x <= 1 inclusive, tf.minimum(x, y) sends ties to x.
 */
int expo_critic_stats_bwd(const void* x, const float* stats, const float* dstats, void* dx, int n, int h,
                          int w, int dtype, void* stream);
int expo_critic_stats_jvp(const void* x, const float* stats, const void* v, float* jv, int n, int h, int w,
                          int dtype, void* workspace, size_t workspace_bytes, void* stream);
int expo_critic_stats_hvp(const void* x, const float* dstats, const float* jv, const void* v, void* out,
                          int n, int h, int w, int dtype, void* stream);

/*
 * The activation of the convnets around the filter path -- lrelu(x) = f1*x + f2*|x| with leak 0.2 (util.py:225-229),
 * used after every ly.conv2d / ly.fully_connected of feature_extractor (agent.py:21-32), cnn (critics.py:13-35) and
 * the FC heads (filters.py:31-42, agent.py:87-99, critics.py:94-97) -- fused with the bias add in front of it.
 *   expo_bias_lrelu_fwd   z[i] = lrelu(y[i] + bias[i % channels])     bias may be NULL (then channels is ignored)
 *   expo_lrelu_bwd        dy[i] = dz[i] * (z[i] > 0 ? 1 : z[i] < 0 ? leak : (1 + leak) / 2)
 * float32, `count` contiguous elements, the channel is the fastest dimension (NHWC conv outputs, (N, C) FC
 * outputs); z may alias y, dy may alias dz.  The slope is taken from the OUTPUT z (lrelu keeps sign and zero);
 * exactly at 0 it is TF's sub-gradient f1 (tf.abs has gradient 0 at 0).  expo_lrelu_bwd is linear in dz and
 * therefore its own double backward (net.py:174-194).
 */
int expo_bias_lrelu_fwd(const float* y, const float* bias, float* z, size_t count, int channels, float leak,
                        void* stream);
int expo_lrelu_bwd(const float* z, const float* dz, float* dy, size_t count, float leak, void* stream);
/* (ABI 4) The same backward WITH the layer's bias gradient: dy as above and dbias[c] = sum over rows of dy[row][c]
 * (what tf.gradients returns for the biases of ly.conv2d / ly.fully_connected: agent.py:21-32, critics.py:13-35) in one
 * pass over dz instead of a second reduction pass over dy.  channels: a power of two in [4, 256]; count a multiple of
 * channels; 16-byte aligned pointers; dbias [channels] is overwritten; workspace >= expo_lrelu_bwd_bias_workspace_bytes(
 * channels) bytes, 16-byte aligned, uninitialised.  No atomics; bit-reproducible. */
size_t expo_lrelu_bwd_bias_workspace_bytes(int channels);
int expo_lrelu_bwd_bias(const float* z, const float* dz, float* dy, float* dbias, size_t count, int channels,
                        float leak, void* workspace, size_t workspace_bytes, void* stream);

/*
 * (ABI 4) The tail of the agent's FC heads: every filter's `filter_param_regressor` (filters.py:177-179 E, 201-203 G,
 * 224-235 W, 481-482 S+, 306-310 T, 411-413 Ct, 435-436 BW, 256-262 C, 457-458 Le) followed by the one-hot selection of
 * the chosen filter's parameters (agent.py:58-77, 119-125), per image, in one launch:
 *   params[n][0..P) = regressor_{abi_ids[j]}(raw[j][n][0..P)),  j = selected[n];  the rest of the row, and the whole row
 *   for j = -1, is 0.
 * raw: HOST array of `heads` device pointers, head j holding float32 [n][widths[j]] (its second FC's output: P_j filter
 * features followed by the mask features); abi_ids[j]: the C-ABI filter id of head j; selected: device int32 [n]
 * (position in cfg.filters, -1 = none); params / dparams: float32 [n][EXPO_MAX_PARAMS]; ranges: HOST float[9] =
 * {exposure_range, log(gamma_range), tone lo, tone hi, tone bias, colour lo, colour hi, colour bias, exposure bias}
 * (cfg.exposure_range, cfg.gamma_range, cfg.tone_curve_range, cfg.color_curve_range; the biases are util.py:281-294's
 * atanh(2 (initial - l) / (r - l) - 1), 0 for every shipped range).  The white-balance log range is the reference's
 * constant 0.5.  expo_heads_regress_bwd writes d raw[j] for EVERY head (zeros outside the selected head's slice).
 * 8-step curves only (cfg.curve_steps = 8: the rows hold EXPO_MAX_PARAMS values).
 */
int expo_heads_regress_fwd(const float* const* raw, const int* widths, const int* abi_ids, int heads,
                           const float* ranges, const int32_t* selected, float* params, int n, void* stream);
int expo_heads_regress_bwd(const float* const* raw, float* const* draw, const int* widths, const int* abi_ids,
                           int heads, const float* ranges, const int32_t* selected, const float* dparams, int n,
                           void* stream);

/*
 * (ABI 4) Action selection, state update and the image-independent part of the penalty (agent.py:87-125, 207-252;
 * pdf_sample_layer.py:5-10), per image, one launch:
 *   pdf = softmax(logits) + 1e-37;  pdf = pdf (1 - exploration) + exploration / K;  pdf /= sum(pdf) + 1e-30
 *   entropy = -sum pdf log pdf;  random id = #(exclusive cumsum(pdf / (rowsum(pdf) + 1e-36)) < noise) - 1 with the
 *   explicit association orders of the reference's CPU kernels (K = 8: ((p0+p4)+(p2+p6))+((p1+p5)+(p3+p7)); the scan
 *   left to right) -- noise 0 gives -1;  selected = is_train ? random id : argmax(pdf);  onehot;
 *   surrogate = log(pdf[selected] + 1e-10) (0 for -1);  new_states = [submitted, submitted, step + 1, max(usage, onehot)],
 *   submitted = |step + 1 - test_steps| < 1e-4;  penalty_base = (1 - progress) c_e (log K - entropy) + <usage, onehot> c_u
 *   + (1 - submitted) submitted c_s.
 * logits [n][k]; noise: element n * noise_stride (column 0 of z); states / new_states [n][state_dim] = [reward, stopped,
 * step, usage x k, ...], state_dim >= 3 + k: columns c >= 3 + k are copied through, new_states[n][c] = states[n][c]
 * (every element of new_states is written); progress: DEVICE float[1] (a graph input); consts: HOST float[5] = {cfg.exploration,
 * cfg.exploration_penalty, cfg.filter_usage_penalty, cfg.early_stop_penalty, cfg.test_steps}; outputs pdf / onehot
 * [n][k], entropy / surrogate / penalty_base [n], selected int32 [n].  expo_agent_select_bwd: d logits from the
 * gradients of surrogate and penalty_base (through the entropy); k <= 16.
 */
int expo_agent_select_fwd(const float* logits, const float* noise, int noise_stride, const float* states,
                          const float* progress, const float* consts, int k, int state_dim, int is_train, float* pdf,
                          float* entropy, int32_t* selected, float* onehot, float* surrogate, float* new_states,
                          float* penalty_base, int n, void* stream);
int expo_agent_select_bwd(const float* logits, const int32_t* selected, const float* progress, const float* consts,
                          int k, int state_dim, const float* d_surrogate, const float* d_penalty_base, float* d_logits,
                          int n, void* stream);

/*
 * (ABI 4) The critic step's loss glue (net.py:126-194) -- the callers of the critic around the filter path:
 *   expo_gp_inputs         cat[0:n] = real, cat[n:2n] = fake (float32) and the gradient penalty's interpolation
 *                          interp = real + alpha[n] (fake - real) (net.py:170-172) in one pass; real / fake of `dtype`,
 *                          elems_per_image = H*W*3; interp (and alpha) may be NULL: conversion + concatenation only
 *                          (the generator step's image pairs, exposure_amd/generator_direct.py)
 *   expo_gp_inputs_rows    the same with the batch's images named by ROW: image i is row real_rows[i] of `real` / row
 *                          fake_rows[i] of `fake` (device int64[n]; NULL: row i) -- the replayed records are read straight
 *                          out of the replay memory's pool and the resident data set (replay_memory.py:168-185 builds
 *                          that batch on the host), no gather launch in front
 *   expo_grad_penalty_fwd  per image: norm = sqrt(1e-6 + sum g^2), term = max(norm - 1, 0)^2 (net.py:185-187; the
 *                          penalty is lambda * mean(term)); g float32 [n][elems_per_image]
 *   expo_grad_penalty_bwd  dg = g * dterm[n] * 2 max(norm - 1, 0) / norm   (the gradient TF takes of that term with
 *                          respect to `gradients`; it then flows on into the critic's double backward)
 * No workspace; one block per image for the reduction (fixed order).
 */
int expo_gp_inputs(const void* real, const void* fake, const float* alpha, float* cat_out, float* interp, int n,
                   size_t elems_per_image, int dtype, void* stream);
int expo_gp_inputs_rows(const void* real, const int64_t* real_rows, const void* fake, const int64_t* fake_rows,
                        const float* alpha, float* cat_out, float* interp, int n, size_t elems_per_image, int dtype,
                        void* stream);
int expo_grad_penalty_fwd(const float* g, float* norm, float* term, int n, size_t elems_per_image, void* stream);
int expo_grad_penalty_bwd(const float* g, const float* norm, const float* dterm, float* dg, int n,
                          size_t elems_per_image, void* stream);

/*
 * ToneFilter / ColorFilter with ANY number of curve steps L = cfg.curve_steps (config_example.py:27; the reference
 * loops `for i in range(self.cfg.curve_steps)`, filters.py:264-273, 312-322):
 *     y = (L / S) sum_{i<L} clip(x - i/L, 0, 1/L) k_i,   S = sum_i k_i + 1e-30
 * `curves` = 1 (Tone: one curve for the three channels, params float32 [N][L]) or 3 (Color: one per channel,
 * params [N][3][L], channel-major like filter 7).  1 <= L <= EXPO_CURVE_MAX_STEPS.  Filters 4 and 7 of the entry
 * points above ARE these with L = 8, on kernels tuned for that count; other counts run here (one element-wise
 * pass per direction, O(1) work per element).  Gradient conventions as everywhere (tf.clip_by_value passes on both
 * inclusive bounds; x exactly on a knot receives both neighbouring slopes).  expo_curve_bwd: dx nullable, may alias
 * dy; dparams [N][curves * L] is overwritten; `workspace` >= expo_curve_workspace_bytes(n, h, w, curves, steps)
 * bytes, uninitialised, no atomics, bit-reproducible (block records + a finish launch, like expo_filter_bwd).
 */
size_t expo_curve_workspace_bytes(int n, int h, int w, int curves, int steps);
int expo_curve_fwd(const void* x, void* y, const float* params, int n, int h, int w, int dtype, int curves,
                   int steps, void* stream);
int expo_curve_bwd(const void* x, const void* dy, void* dx, const float* params, float* dparams, int n, int h,
                   int w, int dtype, int curves, int steps, void* workspace, size_t workspace_bytes, void* stream);

/*
 * (added exports, ABI 9) The per-image dispatch and the heads' tail for ANY cfg.curve_steps: what
 * expo_filter_dispatch_fwd / _bwd and expo_heads_regress_fwd / _bwd are at 8 steps, with
 *   params / dparams  float32 [N][EXPO_MAX_PARAMS_CURVES];
 *   curve_steps       L in [1, EXPO_CURVE_MAX_STEPS], one value for the call;
 *   ids 4 and 7       the curves of expo_curve_fwd / _bwd with `steps` = L: a Tone row holds k_0..k_{L-1}, a Color row
 *                     channel * L + knot -- the layout expo_chain_fused_curves_fwd_ragged takes;
 *   every other id    (0-3, 5, 6, 8, and -1 = nothing selected) exactly as in expo_filter_dispatch_*, on the first
 *                     slots of the row: the same kernel bodies, the same image and image-gradient bits.
 * Nothing behind a filter's parameters is read.  An id outside [-1, 8] selects nothing, like -1 (the ids live on the
 * device: they are not validated on the host).
 * expo_filter_dispatch_curves_fwd: one streaming launch; `penalty` (nullable, float32 [N]) is the fused over-exposure
 *   term mean max(y - 1, 0)^2 and costs one finish launch and the workspace.
 * expo_filter_dispatch_curves_bwd: dparams is fully overwritten (zeros behind a filter's parameters and in rows with
 *   id -1); dx nullable; dpenalty nullable (the same bits as a dpenalty of zeros: the kernels with the fused penalty
 *   run with a zero scale, so without it the light rows need not have expo_filter_dispatch_bwd's bits, which come from
 *   other instantiations of the bodies), its share 2 max(y - 1, 0) / (H W 3) dpenalty[n] is added to dy first.  Curve
 *   gradients follow expo_curve_bwd (both clip bounds inclusive, both neighbouring slopes on a knot).  Two streaming
 *   launches -- light filters, curves; an image outside a launch's set costs that launch one early exit per block --
 *   and one finish launch.  No float atomics: block records and a fixed-order finish, bit-reproducible.  The curve
 *   launch keeps 3 (2 L + 1) private accumulator columns per thread in dynamic LDS, sized from L.
 * expo_filter_dispatch_curves_workspace_bytes: bytes both directions need (0 for invalid arguments); grows with L, and
 *   holds one image tensor of scratch: dparams has the same bits with and without dx, so the light launch always
 *   stores dx -- compiled without the store three of the tuned bodies round their parameter gradients differently.
 * expo_heads_regress_curves_fwd / _bwd: a Tone head regresses L values, a Color head 3 L; ranges, biases, the -1
 *   convention and "d raw is zero outside the selected head's parameter slice" as in expo_heads_regress_*.
 * Validated before anything is enqueued (EXPO_E_BADARG / EXPO_E_BADDTYPE): curve_steps, shapes, dtype, null pointers,
 * a null / misaligned / short workspace, hsv_grad_mode, the heads' count, widths and filter ids; n == 0 is a no-op.
 */
size_t expo_filter_dispatch_curves_workspace_bytes(int n, int h, int w, int dtype, int curve_steps);
int expo_filter_dispatch_curves_fwd(const int32_t* filter_ids, const void* x, void* y, const float* params,
                                    int curve_steps, float* penalty, int n, int h, int w, int dtype, void* workspace,
                                    size_t workspace_bytes, void* stream);
int expo_filter_dispatch_curves_bwd(const int32_t* filter_ids, const void* x, const void* dy, void* dx,
                                    const float* params, float* dparams, const float* dpenalty, int curve_steps, int n,
                                    int h, int w, int dtype, int hsv_grad_mode, void* workspace, size_t workspace_bytes,
                                    void* stream);
int expo_heads_regress_curves_fwd(const float* const* raw, const int* widths, const int* abi_ids, int heads,
                                  const float* ranges, const int32_t* selected, float* params, int curve_steps, int n,
                                  void* stream);
int expo_heads_regress_curves_bwd(const float* const* raw, float* const* draw, const int* widths, const int* abi_ids,
                                  int heads, const float* ranges, const int32_t* selected, const float* dparams,
                                  int curve_steps, int n, void* stream);

/*
 * One Adam update of a LIST of fp32 tensors in one launch -- the three optimisers of a training iteration
 * (net.py:222-251 `ly.optimize_loss(..., optimizer=cfg.optimizer)`; config_example.py:158
 * `tf.train.AdamOptimizer(learning_rate=lr, beta1=0.5, beta2=0.9)`), replacing torch's fused multi-tensor Adam
 * (one block per 65 536 elements: 43 us for the 1-5 M parameters of one network).
 *   params / grads / exp_avg / exp_avg_sq   host arrays of `count` device pointers; tensor j has numel[j] floats,
 *                                           all four in the same element order (tables of EXPO_ADAM_MAX_TENSORS
 *                                           tensors per launch; more tensors -> more launches)
 *   lr     device float        (a captured launch reads the learning rate of the replay)
 *   step   device float        t - 1 on entry; the update computes with t = step + 1 and a one-thread launch behind it
 *                              stores t (capturable, no host involvement; ABI 4-5 let the update's last block do it,
 *                              found through a ticket atomic per block -- most of the update's time)
 *   ticket device uint32, owned by the optimiser; accepted for ABI compatibility, not touched since ABI 6
 *   step_advanced  (ABI 7) 0: as above.  1: `step` already holds t -- a kernel the caller launched in front of this
 *                              update moved the counter (expo_critic_report's / expo_generator_losses' adam_step
 *                              pointers): the update computes with t = step and launches nothing behind it
 * Update rule (torch.optim.Adam without weight decay / amsgrad; TF-1's differs only in where epsilon sits:
 * sqrt(v) + eps' with eps' = eps sqrt(1 - beta2^t)):
 *   m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 */
#define EXPO_ADAM_MAX_TENSORS 64
int expo_adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const size_t* numel, const float* lr, float* step, void* ticket,
                   float beta1, float beta2, float eps, int step_advanced, void* stream);

/*
 * The input tensor of a convnet: image channels + per-image values broadcast as constant planes, minus `offset` --
 * critics.py:64-76 (`tf.concat([images, state planes, statistics planes], axis=3) - 0.5` in front of `cnn`) and
 * agent.py:17-19, 47-53 (`enrich_image_input`, then `net - 0.5` in feature_extractor): dtype conversion,
 * concatenation and subtraction in one launch.
 *   images  device [N][pixels][3] in `dtype` (NULL: zeros -- the adjoint's own adjoint has no image part)
 *   vec     device float32 [N][V] (0 <= V <= 61)
 *   out     device float32 [N][pixels][3 + V] = (c < 3 ? images : vec[n][c - 3]) - offset
 * Linear, so its derivative is slicing / a per-image sum (the host side leaves those to autograd).
 */
int expo_planes_concat(const void* images, const float* vec, float* out, int n, size_t pixels_per_image, int v,
                       int dtype, float offset, void* stream);

/*
 * The whole input side of a critic / value-net pass as ONE launch (critics.py:42-76 in front of `cnn`; net.py:170-172):
 * what expo_gp_inputs_rows + expo_critic_stats + expo_planes_concat compute in four, for images of at most 4096 pixels
 * (a block holds its image in LDS; EXPO_E_BADARG beyond -- the callers then run the separate launches).
 *   a, b        device [.][H][W][3] in `dtype`; a_rows / b_rows (nullable, int64 [n]): image j of the block is row rows[j]
 *   alpha       nullable float32 [n]: a third block of rows a + alpha (b - a) (the gradient penalty's interpolation)
 *   vec_a/_b    nullable float32 [n][v0]: per-image values of the two blocks (the states critics.py:64-70 broadcasts)
 *   planes      float32 [m][H][W][3 + v0 + 3] = concat(image, values, statistics) - offset,  m = 2 n (3 n with alpha)
 *   stats       float32 [m][3] = {mean luminance, luminance variance, mean saturation} (critics.py:48-62)
 *   x_out       nullable float32 [x_count][H][W][3]: the images of rows x_first .. x_first + x_count as float32 (the rows
 *               whose backward needs them: expo_critic_penalty_tangent, expo_critic_stats_bwd)
 */
int expo_net_inputs(const void* a, const int64_t* a_rows, const void* b, const int64_t* b_rows, const float* alpha,
                    const float* vec_a, const float* vec_b, int v0, float* planes, float* stats, float* x_out, int x_first,
                    int x_count, int n, int h, int w, int dtype, float offset, void* stream);

/*
 * The generator step's loss glue (net.py:92-160 with cfg.gan == 'w'; util.py:13-16 state columns): per image
 *   stopped = new_states[1], step = new_states[2];  nv = new_value * [step <= max_len];  gate = a + (1 - a) stopped
 *   reward = gate (fake_logit - fake_input_logit) m - penalty;  q = reward + (1 - stopped) gamma nv;  adv = q - old_value
 *   use_td:  g term = -q plm - surrogate adv      (net.py:135-140, 152-157)
 *   else:    g term = -reward - surrogate reward
 *   losses[0] = g_loss = mean g term,  losses[1] = v_loss = mean adv^2
 * consts = host float[5] {a = all_reward, m = critic_logit_multiplier, gamma = discount_factor,
 * plm = parameter_lr_mul, max_len = maximum_trajectory_length}; penalty may be NULL (cfg.use_penalty off).
 * All vectors float32 [N]; new_states [N][state_dim].  reward / q_value [N] are reported values;
 * coef float32 [5][N] receives d g_loss / d {fake_logit, new_value, surrogate, penalty} and d v_loss / d old_value
 * (stop-gradients of the reference applied: the weight of the surrogate and q inside adv are constants), so the
 * backward pass is coef times the upstream scalar.  One block; N is a minibatch.
 * adam_step_a / adam_step_b (ABI 7; nullable device floats) += 1: the step counters of the generator's and the value net's
 * updates behind this launch (expo_adam_step with step_advanced = 1).
 */
int expo_generator_losses(const float* fake_logit, const float* fake_input_logit, const float* new_value,
                          const float* old_value, const float* new_states, int state_dim, const float* penalty,
                          const float* surrogate, const float* consts, int use_td, float* losses, float* reward,
                          float* q_value, float* coef, int n, float* adam_step_a, float* adam_step_b, void* stream);

/* ---- the convnets' convolution (round 5) ------------------------------------------------------------------------
 * `ly.conv2d(net, C_out, kernel_size=4, stride=2)` (SAME padding; agent.py:21-32, critics.py:13-35) on NHWC float32
 * tensors as implicit-GEMM kernels on the f32 matrix cores (csrc/conv_ops.hip), with the layer's bias + lrelu
 * (util.py:225-229) in the epilogue:
 *   y[n][oh][ow][co] = f(bias[co] + sum_{kh,kw,ci} x[n][2 oh - 1 + kh][2 ow - 1 + kw][ci] w[co][kh][kw][ci])
 *   x     float32 [n][h][w][cin] (h, w even)      w     float32 [cout][4][4][cin] (16-byte aligned: the channels_last
 *   y     float32 [n][h/2][w/2][cout]                    memory order of an nn.Conv2d weight (cout, cin, 4, 4))
 *   bias  float32 [cout] or NULL                  act   0: f = identity, 1: f = lrelu(., leak)
 * Deterministic (fixed summation order, no atomics), no workspace.  Replaces aten::miopen_convolution +
 * expo_bias_lrelu_fwd for these layers. */
int expo_conv4x4s2_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int cin,
                       int cout, int act, float leak, void* stream);
/* The data gradient of the same convolution (the transposed convolution of dy): four dense GEMMs, one per parity
 * class of the input pixel.  Replaces aten::convolution_backward(input gradient only) and the zero fill in front of
 * MIOpen's split-K kernel.
 *   dy  float32 [n][h/2][w/2][cout] (cout % 4 == 0)     dx  float32 [n][h][w][cin], every element written */
int expo_conv4x4s2_bwd_data(const float* dy, const float* w, float* dx, int n, int h, int wd, int cin, int cout,
                            void* stream);
/* The weight gradient: dw[co][kh][kw][ci] = sum over the batch's output pixels of dy[.][co] x[.][kh][kw][ci], written in
 * the weight's own memory order, every element (dw 16-byte aligned).  The pixel sum of a 32 x 128 tile of dw is spread
 * over P blocks; for P > 1 the blocks write P full-size copies of dw into `workspace` (caller-owned scratch, no
 * initialisation needed, at least expo_conv4x4s2_wrw_workspace_bytes(...) bytes, 16-byte aligned) and a second,
 * element-wise launch adds them in block order: deterministic, no atomics, no zero fill of dw.  w / 2 must be even.
 * Replaces aten::convolution_backward(weight gradient only) + the zero fill in front of MIOpen's split-K kernel. */
size_t expo_conv4x4s2_wrw_workspace_bytes(int n, int h, int wd, int cin, int cout);
int expo_conv4x4s2_wrw(const float* x, const float* dy, float* dw, int n, int h, int wd, int cin, int cout,
                       void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 6) The same three primitives with the ACTIVATION'S gradient and the BIAS gradient folded in -- what a layer
 * `z = lrelu(conv(x, w) + b)` (agent.py:21-32, critics.py:13-35; util.py:225-229) needs around its convolutions in the
 * backward and in the gradient penalty's double backward (net.py:174-194), without launches of their own:
 *   slope(z) = 1 (z > 0), leak (z < 0), (1 + leak) / 2 (z == 0: TF's sub-gradient of f1 x + f2 |x|)
 *   expo_conv4x4s2_bwd_data_mask   dx = D(dy, w) * slope(zmask):  zmask float32 [n][h][w][cin] = the activation of the
 *                                  layer BELOW -- its lrelu backward in this kernel's epilogue
 *   expo_conv4x4s2_fwd_mask        y = F(x, w) * slope(zmask):    zmask float32 [n][h/2][w/2][cout]; y MAY ALIAS zmask --
 *                                  the tangent of the double backward, t_l = F(t_{l-1}, w_l) slope(z_l), written over z_l
 *   expo_conv4x4s2_wrw_bias        expo_conv4x4s2_wrw and dbias[co] = sum of dy[.][co] over the output pixels of the
 *                                  first `bias_images` images (0 <= bias_images <= n; cout % 4 == 0, dbias 16-byte
 *                                  aligned): the column sums come from the values the kernel feeds to the matrix cores
 *                                  anyway.  Same workspace as expo_conv4x4s2_wrw (the bias copies are part of it).
 * The data gradient of the layers with 6 or 17 input planes (critic, value net) runs on the vector ALUs with the weights
 * in scalar registers (conv_bwd_small_kernel: a 32-wide matrix-core tile would be 81 % / 47 % padding). */
int expo_conv4x4s2_bwd_data_mask(const float* dy, const float* w, const float* zmask, float* dx, int n, int h, int wd,
                                 int cin, int cout, float leak, void* stream);
int expo_conv4x4s2_fwd_mask(const float* x, const float* w, const float* zmask, float* y, int n, int h, int wd, int cin,
                            int cout, float leak, void* stream);
int expo_conv4x4s2_wrw_bias(const float* x, const float* dy, float* dw, float* dbias, int bias_images, int n, int h,
                            int wd, int cin, int cout, void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 7) Two problems of ONE geometry as one grid: the forward (bias + activation) and the data gradient (activation
 * gradient of the layer below in the epilogue) of two independent layers -- the agent's filter and selector extractors read
 * the same input through different weights (agent.py:47-56), the critic's and the value net's pair passes of a G / V step run
 * side by side -- at batch 64 / 128, where one of them alone leaves CUs idle.  The decomposition is chosen for the grid that
 * runs (twice the blocks), so the results equal the two separate calls up to the order in which the K slices are added
 * (float32 rounding); a pair call is bit-reproducible. */
int expo_conv4x4s2_fwd_pair(const float* x_a, const float* w_a, const float* bias_a, float* y_a, const float* x_b,
                            const float* w_b, const float* bias_b, float* y_b, int n, int h, int wd, int cin, int cout, int act,
                            float leak, void* stream);
/* (ABI 7) expo_conv4x4s2_fwd (zmask NULL) / expo_conv4x4s2_fwd_mask (zmask given, bias NULL, act 0) of a FIRST layer whose input
 * comes from expo_planes_concat / expo_net_inputs / expo_critic_penalty_tangent: channels 3 .. cin - 1 of x are per-image
 * CONSTANTS (the states and statistics critics.py:64-76 / agent.py:17-19 broadcast as planes; the kernel reads their values
 * from the image's first pixel).  The convolution is linear, so the constant planes contribute one value per image, channel
 * and border class (which of the 4 x 4 taps fall inside the image): K shrinks from 16 cin to 48.  Same sum in another order
 * (float32 rounding).  64-wide inputs of 4 .. 20 planes and at most 32 output channels; EXPO_E_BADARG otherwise (take
 * expo_conv4x4s2_fwd).  The caller vouches for the planes being constant. */
int expo_conv4x4s2_fwd_planes(const float* x, const float* w, const float* bias, const float* zmask, float* y, int n, int h,
                              int wd, int cin, int cout, int act, float leak, void* stream);
int expo_conv4x4s2_fwd_planes_pair(const float* x_a, const float* w_a, const float* bias_a, float* y_a, const float* x_b,
                                   const float* w_b, const float* bias_b, float* y_b, int n, int h, int wd, int cin, int cout,
                                   int act, float leak, void* stream);
int expo_conv4x4s2_bwd_data_mask_pair(const float* dy_a, const float* w_a, const float* zmask_a, float* dx_a, const float* dy_b,
                                      const float* w_b, const float* zmask_b, float* dx_b, int n, int h, int wd, int cin,
                                      int cout, float leak, void* stream);
/* The weight (and bias) gradients of up to 8 layers -- a whole stack -- with ONE reduce launch for all of them: per layer the
 * arguments of expo_conv4x4s2_wrw_bias (arrays of `count` entries; dbias[l] may be NULL: no bias gradient for that
 * layer), each layer with its own workspace of expo_conv4x4s2_wrw_workspace_bytes(...) bytes.  Same results, bit for
 * bit, as `count` separate calls. */
int expo_conv4x4s2_wrw_group(int count, const float* const* x, const float* const* dy, float* const* dw,
                             float* const* dbias, const int* bias_images, const int* n, const int* h, const int* wd,
                             const int* cin, const int* cout, void* const* workspace, const size_t* workspace_bytes,
                             void* stream);
/* Probes and tests: waves per block (1 .. 4) and blocks per tile of the weight-gradient kernel (negative = leave as
 * is, 0 = the library's choice; initial values from EXPO_CONV_WRW_SLICES / EXPO_CONV_PARTS).  Independent of
 * expo_conv_tuning's `slices`. */
int expo_conv_wrw_tuning(int slices, int parts);
/* Probes and tests: override how the forward / data-gradient kernels decompose a problem (process-wide; negative = leave as is,
 * 0 = the library's own choice).  tile 1-4: an LDS-tiled forward shape, 5: the flat kernel, 6: the
 * first layers' row-staged kernel where it applies; nt 1 | 2: column tiles per
 * wave; slices 1, 2, 4, 8 or 16: K slices per tile (any other value is rejected: the kernels cut K into 4 S2 segments).
 * The initial values come from EXPO_CONV_TILE / _NT / _SLICES, read once. */
int expo_conv_tuning(int tile, int nt, int slices);

/* ---- the hand-scheduled critic update (round 6; csrc/critic_step.hip, exposure_amd/critic_direct.py) ------------------
 * net.py:126-199, 245-251: c_loss = mean(D(fake) - D(real)) + lambda mean(max(||grad_x^ D(x^)|| - 1, 0)^2).  The real,
 * fake and interpolated images run as ONE batch [real | fake | interpolated] through critics.py:42-98; the kernels
 * below are the per-row / per-image reductions between its convolutions and GEMMs.  Fixed summation orders.
 *   expo_critic_head_fwd  hpre float32 [slabs][M][hidden]: fc1's pre-activation (critics.py:94-96) as `slabs` partial sums
 *                         (expo_fc_fwd_slabs; 1 = the finished GEMM) added here in slab order, + b1 (nullable: already
 *                         inside), M = n_real + n_fake + n_interp rows.  h = lrelu(hpre); logits[m] = h[m] . w2 + b2 (critics.py:97);
 *                         dh[m] = dlogit[m] w2 slope(h[m]) with dlogit = -inv_n (real), +inv_n (fake), 1 (interpolated:
 *                         the inner gradient starts from ones, net.py:174-183)
 *   expo_critic_report    out[0..4] = {c_loss = mean fake - mean real + lambda mean term, emd = mean real - mean fake, mean
 *                         norm, lambda mean term, c_average = (mean fake + mean real) / 2} (net.py:188-199) from the logits
 *                         [real | fake | interpolated] and the per-image norm / term; ema (nullable, device float) advances
 *                         as ema += (1 - decay) (c_average - ema) (update_average, net.py:165-168, 267-268); adam_step
 *                         (nullable, device float) += 1: the step counter of the update behind this launch
 *                         (expo_adam_step with step_advanced = 1)
 *   expo_critic_head_bwd  gb1 = sum over the real + fake rows of dh;  gw2 = sum over those rows of dlogit h + sum over
 *                         the interpolated rows of thpre slope(h) (thpre float32 [th_slabs][n_interp][hidden]: the penalty's
 *                         tangent in front of fc1's activation, as partial sums like hpre);  gb2 = sum of dlogit.
 *                         n_real == n_fake: gb1 adds dh[m] + dh[n_real + m] first and sums those pairs, so a unit whose
 *                         real / fake pairs have equal slopes (dh exact negatives) gets gb1 == 0.0 exactly, for every
 *                         row count; unequal counts: the rows in index order
 *   expo_plane_sums       sums[n][c - first] = sum over the pixels of x[n][.][c], first <= c < channels (<= 16 planes):
 *                         the gradient reaching the per-image values planes_concat broadcast (critics.py:64-76)
 *   expo_gp_direct        g = u[..., 0:3] + ds (u float32 [n][pixels][u_channels], ds [n][pixels][3]);
 *                         norm = sqrt(1e-6 + sum g^2), term = max(norm - 1, 0)^2 (net.py:185-187) and
 *                         v = scale 2 max(norm - 1, 0) / norm g  (the gradient of scale sum(term)) in one launch
 *   expo_critic_penalty_tangent  everything between the first layer's data gradient and the tangent pass as ONE launch (a
 *                         block per image): u float32 [n][h w][6] (image + statistics planes), x float32 [n][h w][3] the
 *                         interpolated images, stats [n][3] their statistics ->  gs = plane sums of u[..., 3:6];
 *                         g = u[..., 0:3] + J^T gs (expo_critic_stats_bwd);  norm, term as expo_gp_direct;
 *                         v = scale 2 max(norm - 1, 0) / norm g;  t0 [n][h w][6] = [v | J v broadcast]
 *                         (expo_critic_stats_jvp + expo_planes_concat with offset 0): the tangent's input */
int expo_critic_head_fwd(const float* hpre, const float* b1, int slabs, const float* w2, const float* b2, int n_real, int n_fake,
                         int n_interp, int hidden, float inv_n, float leak, float* logits, float* h, float* dh, void* stream);
int expo_critic_report(const float* logits, const float* norm, const float* term, int n_real, int n_fake, int n_interp,
                       float lambda, float decay, float* out, float* ema, float* adam_step, void* stream);
int expo_critic_head_bwd(const float* dh, const float* h, const float* thpre, int th_slabs, int n_real, int n_fake,
                         int n_interp, int hidden, float inv_n, float leak, float* gb1, float* gw2, float* gb2, void* stream);

/* ---- the first FC layer behind a convnet (critics.py:27-31 / agent.py:33-35: ly.fully_connected(flat, 128)) in the
 * hand-scheduled passes: the library GEMM takes ~10 us for it whatever the batch is (one workgroup per 16 x 16 tile walks
 * K = 4096), 14 calls per training iteration.
 *   expo_fc_fwd_slabs_count  S = the number of partial sums expo_fc_fwd_slabs writes for M rows of K features (0: K is not
 *                         a multiple of 128 -- use the library GEMM)
 *   expo_fc_fwd_slabs     slabs float32 [S][M][N]: slab s = x[:, K_s] w[:, K_s]^T over the s-th of S ranges of K (x float32
 *                         [M][K], w float32 [N][K] = nn.Linear's weight).  Their sum in slab order (+ bias) is the
 *                         pre-activation; expo_critic_head_fwd / _bwd add them while they read it.  Fixed summation order.
 *   expo_fc_bwd_data_mask gy float32 [M][C] = (dh w) slope(z): the layer's data gradient (dh float32 [M][J], w float32
 *                         [J][C], J % 16 == 0, C % 128 == 0) times the activation gradient of the feature map z [M][C] below
 *                         it (util.py:225-229; TF's sub-gradient at 0) -- torch.mm + expo_lrelu_bwd in one launch */
int expo_fc_fwd_slabs_count(int m, int k);
int expo_fc_fwd_slabs(const float* x, const float* w, float* slabs, int m, int n, int k, void* stream);
int expo_fc_bwd_data_mask(const float* dh, const float* w, const float* z, float* gy, int m, int j, int c, float leak,
                          void* stream);
/*   expo_fc_wrw           dw float32 [J][C] = dh^T x (dh float32 [M][J], x float32 [M][C]): the layer's weight gradient over M
 *                         rows -- a GEMM whose K dimension is the batch; OVERWRITTEN, fixed summation order */
int expo_fc_wrw(const float* dh, const float* x, float* dw, int m, int j, int c, void* stream);
int expo_plane_sums(const float* x, float* sums, int n, size_t pixels_per_image, int channels, int first, void* stream);
int expo_gp_direct(const float* u, int u_channels, const float* ds, float scale, float* v, float* norm, float* term, int n,
                   size_t pixels_per_image, void* stream);
int expo_critic_penalty_tangent(const float* u, const float* x, const float* stats, float scale, float* t0, float* norm,
                                float* term, int n, int h, int w, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* EXPOSURE_HIP_H_ */
