#!/bin/bash
# Build libexposure_hip.so for gfx950 in-tree (the .so is git-ignored but travels with gpurun).
# Fifteen translation units plus chain_fused_curves.hip, the sixteenth, dispatch_curves.hip, the seventeenth, and
# chain_fused_curves_codes.hip, the eighteenth, and chain_steps_bwd.hip, the nineteenth, and png_encode.hip, the twentieth, and chain_steps_bwd_rc.hip, the twenty-first, and chain_steps_bwd_seq.hip, the twenty-second, and jpeg_encode.hip, the twenty-third, and jpeg_decode.hip, the twenty-fourth, and jpeg_decode_sync.hip, the twenty-fifth;
# extra arguments go to every compile step.
#   exposure_hip.hip     the streaming kernels and the C-ABI (default flags)
#   chain_steps.hip      several forward steps of expo_chain_fwd in one launch (the flags of exposure_hip.hip: it
#                        must reproduce the per-step kernels bit for bit)
#   chain_steps_bwd.hip  runs of element-wise backward steps of expo_chain_bwd in one launch (the flags of
#                        exposure_hip.hip: it must reproduce the per-step kernels bit for bit)
#   chain_steps_bwd_rc.hip  the same runs with their interior activations recomputed from the run's lowest one
#                        instead of loaded (the flags of exposure_hip.hip: its forward sweep must reproduce the
#                        per-step forward kernels bit for bit, its backward steps the per-step backward kernels)
#   chain_steps_bwd_seq.hip  the runs whose filter sequence is known at build time (the reference's filter order) as
#                        straight-line kernels, one per sequence (the flags of exposure_hip.hip: every step must
#                        reproduce the per-step kernels bit for bit)
#   chain_fused.hip      the VALU-bound fused inference kernel (-fno-slp-vectorize -fno-honor-nans, see the file)
#   chain_fused_codes.hip  the fused inference pass reading the files' integer codes (exactly chain_fused.hip's flags:
#                        it includes that file for the step loop and the stores and must reproduce its outputs bit for bit)
#   chain_fused_curves.hip  the fused inference pass for any cfg.curve_steps (exactly chain_fused.hip's flags: it
#                        includes that file and must reproduce its bits for every step that is no curve)
#   chain_fused_bwd.hip  the one-pass backward of a fixed sequence (-fno-slp-vectorize: the packed-fp32 pairs cost it
#                        ~100 VGPRs)
#   nn_ops.hip           the convnets' activation and glue
#   curve_generic.hip    Tone / Color for cfg.curve_steps other than 8
#   conv_ops.hip         the convnets' 4x4 / stride-2 convolution on the f32 matrix cores
#   critic_step.hip      the reductions of the hand-scheduled critic update
#   decode.hip           the integer codes of an input image to the linear storage tensor (default flags: its
#                        normalising division must stay IEEE)
#   datasets.hip         the training sets' INTER_AREA master pack and its per-epoch re-cut (default flags)
#   proxy.hip            the agent's bilinear 64x64 proxies of a ragged batch (-ffp-contract=off: every operation of
#                        its definition is rounded on its own, so the host restatement matches bit for bit)
#   proxy_codes.hip      the same proxies read from the files' integer codes (exactly proxy.hip's flags: it includes that file
#                        for the arithmetic)
#   codes_lut.hip        integer pictures gathered from the files' integer codes through caller-built tables (default flags)
#   metric.hip           the evaluation metric's patch statistics and their histograms (default flags)
#   dispatch_curves.hip  the agent's per-image dispatch step and its head regressors for any cfg.curve_steps (the flags
#                        of exposure_hip.hip: the light filters' bodies must give that unit's bits)
#   chain_fused_curves_codes.hip  the fused inference pass for any cfg.curve_steps reading the files' integer codes
#                        (exactly chain_fused.hip's flags: the step loop of chain_fused_curves.hip behind the loader of
#                        chain_fused_codes.hip, bit for bit decode + that pass)
#   png_encode.hip      8-bit PNG files made on the device: the row filter and a Huffman-only deflate in independent
#                        segments (default flags: integer code; png_deflate.h holds its serial routines, which
#                        tools/png_rehearse.cpp runs on the host)
#   jpeg_encode.hip     baseline JPEG files made on the device: colour conversion, 8 x 8 transform, quantisation and the
#                        fixed Huffman code in independent restart intervals (default flags: integer code; jpeg_codec.h
#                        holds its serial routines, which tools/jpeg_rehearse.cpp runs on the host)
#   jpeg_decode.hip     baseline JPEG files decoded on the device: entropy decoding a lane per restart interval, the
#                        inverse transform, chroma upsampling and colour (default flags: integer code; jpeg_decode.h
#                        holds its serial routines, which tools/jpeg_decode_rehearse.cpp runs on the host)
#   jpeg_decode_sync.hip  files without restart markers decoded in parallel: speculative walks a lane per subsequence,
#                        their settling, its verification and the stores (default flags: integer code;
#                        jpeg_decode_sync.h holds its serial routines, which tools/jpeg_sync_rehearse.cpp runs on the host)
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${EXPO_LIB_OUT:-$HERE/../libexposure_hip.so}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
TMP="$(mktemp -d)"
trap 'rm -rf "$TMP"' EXIT
# the digest of the sources, baked into the binary (expo_build_info): _cabi.load() recomputes it and refuses a stale .so
DIGEST="$(cd "$HERE" && LC_ALL=C ls *.hip *.h build.sh | LC_ALL=C sort | xargs cat ../../include/exposure_hip.h | sha256sum | cut -d' ' -f1)"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC "-DEXPO_SOURCE_DIGEST=\"$DIGEST\"")
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/exposure_hip.hip" -o "$TMP/exposure_hip.o" &
p1=$!
"$HIPCC" "${FLAGS[@]}" -fno-slp-vectorize -fno-honor-nans "$@" -c "$HERE/chain_fused.hip" -o "$TMP/chain_fused.o" &
p2=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/nn_ops.hip" -o "$TMP/nn_ops.o" &
p3=$!
"$HIPCC" "${FLAGS[@]}" -fno-slp-vectorize "$@" -c "$HERE/chain_fused_bwd.hip" -o "$TMP/chain_fused_bwd.o" &
p4=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/curve_generic.hip" -o "$TMP/curve_generic.o" &
p5=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/conv_ops.hip" -o "$TMP/conv_ops.o" &
p6=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/critic_step.hip" -o "$TMP/critic_step.o" &
p7=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/decode.hip" -o "$TMP/decode.o" &
p8=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/datasets.hip" -o "$TMP/datasets.o" &
p9=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/chain_steps.hip" -o "$TMP/chain_steps.o" &
p10=$!
"$HIPCC" "${FLAGS[@]}" -ffp-contract=off "$@" -c "$HERE/proxy.hip" -o "$TMP/proxy.o" &
p11=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/metric.hip" -o "$TMP/metric.o" &
p12=$!
# (a bare `wait` returns 0 whatever the jobs did: wait for each PID so a failed compile stops the script here)
"$HIPCC" "${FLAGS[@]}" -fno-slp-vectorize -fno-honor-nans "$@" -c "$HERE/chain_fused_codes.hip" -o "$TMP/chain_fused_codes.o" &
p13=$!
"$HIPCC" "${FLAGS[@]}" -ffp-contract=off "$@" -c "$HERE/proxy_codes.hip" -o "$TMP/proxy_codes.o" &
p14=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/codes_lut.hip" -o "$TMP/codes_lut.o" &
p15=$!
"$HIPCC" "${FLAGS[@]}" -fno-slp-vectorize -fno-honor-nans "$@" -c "$HERE/chain_fused_curves.hip" -o "$TMP/chain_fused_curves.o" &
p16=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/dispatch_curves.hip" -o "$TMP/dispatch_curves.o" &
p17=$!
"$HIPCC" "${FLAGS[@]}" -fno-slp-vectorize -fno-honor-nans "$@" -c "$HERE/chain_fused_curves_codes.hip" -o "$TMP/chain_fused_curves_codes.o" &
p18=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/chain_steps_bwd.hip" -o "$TMP/chain_steps_bwd.o" &
p19=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/png_encode.hip" -o "$TMP/png_encode.o" &
p20=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/chain_steps_bwd_rc.hip" -o "$TMP/chain_steps_bwd_rc.o" &
p21=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/chain_steps_bwd_seq.hip" -o "$TMP/chain_steps_bwd_seq.o" &
p22=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/jpeg_encode.hip" -o "$TMP/jpeg_encode.o" &
p23=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/jpeg_decode.hip" -o "$TMP/jpeg_decode.o" &
p24=$!
"$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/jpeg_decode_sync.hip" -o "$TMP/jpeg_decode_sync.o" &
p25=$!
wait $p1
wait $p2
wait $p3
wait $p4
wait $p5
wait $p6
wait $p7
wait $p8
wait $p9
wait $p10
wait $p11
wait $p12
wait $p13
wait $p14
wait $p15
wait $p16
wait $p17
wait $p18
wait $p19
wait $p20
wait $p21
wait $p22
wait $p23
wait $p24
wait $p25
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "$TMP/exposure_hip.o" "$TMP/chain_fused.o" "$TMP/nn_ops.o" "$TMP/chain_fused_bwd.o" "$TMP/curve_generic.o" "$TMP/conv_ops.o" "$TMP/critic_step.o" "$TMP/decode.o" "$TMP/datasets.o" "$TMP/chain_steps.o" "$TMP/proxy.o" "$TMP/metric.o" "$TMP/chain_fused_codes.o" "$TMP/proxy_codes.o" "$TMP/codes_lut.o" "$TMP/chain_fused_curves.o" "$TMP/dispatch_curves.o" "$TMP/chain_fused_curves_codes.o" "$TMP/chain_steps_bwd.o" "$TMP/png_encode.o" "$TMP/chain_steps_bwd_rc.o" "$TMP/chain_steps_bwd_seq.o" "$TMP/jpeg_encode.o" "$TMP/jpeg_decode.o" "$TMP/jpeg_decode_sync.o" -o "$OUT"
echo "built $OUT (sources $DIGEST)"
