// png_encode.hip -- 8-bit RGB PNG files made on the device (expo_png_encode_ragged): the row filter of
// the PNG specification and a Huffman-only deflate, cut into segments of SEG stream bytes that are compressed on their
// own and end on a byte boundary, one IDAT chunk each, so that no workgroup waits for another and no CRC spans two of
// them.  What show_and_save hands to cv2.imwrite (net.py:769-772) is then written without a host compressor.
// Default flags (csrc/build.sh).  Integer code only: no float, no global atomic, no zero-filled state; the bytes depend
// on the picture and the filter alone.  Four launches per group of up to 64 pictures, in stream order:
//   png_row_types_kernel  filter 5 only: a wave per row sums min(b, 256 - b) of the row under the five filters and
//                         keeps the smallest (ties to the lowest type)
//   png_segment_kernel    a workgroup per segment: filters its SEG stream bytes from the picture into LDS (the filtered
//                         stream is never stored), counts them, builds the code (lengths serially in one lane, the rest
//                         in parallel), decides dynamic against stored, packs the bits in LDS, adds the chunk's length,
//                         type and CRC-32 and writes the finished chunk to its slot with the Adler pair of its bytes
//   png_scan_kernel       a workgroup per picture: the chunks' offsets in the file, the Adler-32 of the stream, the
//                         file's length
//   png_gather_kernel     a workgroup per chunk copies it to its place; one more per picture writes the signature,
//                         IHDR, the zlib header, the Adler chunk and IEND
// The serial routines are png_deflate.h's, which tools/png_rehearse.cpp runs on the host.
#include <limits.h>

#include "host_common.h"
#include "png_deflate.h"

namespace expo {

namespace {

using namespace png;

constexpr int kPngMaxImages = 64;
constexpr int kSegWords = kSeg / 4;
constexpr int kChunkBytes = kSeg / kThreads;  // stream bytes a thread packs: a contiguous run
constexpr int kChunkWords = kChunkBytes / 4;
static_assert(kChunkBytes % 4 == 0 && kChunkWords == 16, "the LDS padding below is one word per 16");

// up to 64 pictures by value in the kernel arguments (2.6 KB)
struct PngTable {
  const uint8_t* pic[kPngMaxImages];
  uint8_t* out[kPngMaxImages];
  int64_t base[kPngMaxImages];  // the picture's part of the workspace (png::layout)
  int h[kPngMaxImages];
  int w[kPngMaxImages];
  int first_row[kPngMaxImages + 1];  // first block of png_row_types_kernel
  int first_seg[kPngMaxImages + 1];  // first segment
  int n;
};
static_assert(sizeof(PngTable) + 32 <= 4096, "the table must fit the 4 KB kernarg block");

// a picture's record in the workspace, at its base
struct ImageRec {
  int64_t total;
  uint32_t adler;
  uint32_t pad;
};
constexpr int kImageRec = 16;
static_assert(sizeof(ImageRec) == kImageRec, "ImageRec");

__host__ __device__ inline Layout image_layout(int64_t base, int h, int64_t nseg) { return layout(base + kImageRec, h, nseg); }

// the last image whose first block is <= b
__device__ __forceinline__ int find_image(const int* first, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t lo = __shfl_xor(uint32_t(v), m, 64), hi = __shfl_xor(uint32_t(v >> 32), m, 64);
    v += (uint64_t(hi) << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void png_row_types_kernel(const PngTable tab, uint8_t* __restrict__ ws) {
  const int b = blockIdx.x;
  const int i = find_image(tab.first_row, tab.n, b);
  const int h = tab.h[i], w3 = 3 * tab.w[i];
  const int r = (b - tab.first_row[i]) * kWaves + int(threadIdx.x >> 6);
  if (r >= h) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint8_t* cur = tab.pic[i] + size_t(r) * size_t(w3);
  const uint8_t* prev = cur - w3;  // read only when r > 0
  uint64_t sum[5] = {0, 0, 0, 0, 0};
  for (int x = lane; x < w3; x += 64) {
    const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, up = r ? prev[x] : 0, c = (r && x >= 3) ? prev[x - 3] : 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) sum[t] += uint32_t(filter_cost(filter_byte(t, v, a, up, c)));
  }
  int best = 0;
  uint64_t least = wave_sum(sum[0]);
#pragma unroll
  for (int t = 1; t < 5; ++t) {
    const uint64_t s = wave_sum(sum[t]);
    if (s < least) {
      least = s;
      best = t;
    }
  }
  if (lane == 0) {
    const Layout l = image_layout(tab.base[i], h, 0);
    ws[l.types + r] = uint8_t(best);
  }
}

// `n` bits (at most 32) of `v` into the zeroed LDS words at bit `pos`
__device__ __forceinline__ void put_bits(uint32_t* words, uint32_t pos, uint32_t v, int n) {
  if (n <= 0) return;
  const uint64_t x = uint64_t(v) << (pos & 31);
  atomicOr(&words[pos >> 5], uint32_t(x));
  if (uint32_t(x >> 32)) atomicOr(&words[(pos >> 5) + 1], uint32_t(x >> 32));
}

// stream word q of the segment in LDS: a thread's 16 words sit 17 apart from its neighbour's, off each other's banks
__device__ __forceinline__ int seg_index(int q) { return q + (q >> 4); }

__global__ __launch_bounds__(kThreads) void png_segment_kernel(const PngTable tab, uint8_t* __restrict__ ws, int filter) {
  __shared__ uint32_t seg[kSegWords + kSegWords / 16];
  __shared__ __attribute__((aligned(16))) uint32_t obuf[kSlot / 4];  // the chunk: length, type, deflate data, CRC
  __shared__ uint32_t hist[kSyms];
  __shared__ int sorted_f[kSyms];
  __shared__ int sorted_len[kSyms];
  __shared__ uint16_t rank_of[kSyms];
  __shared__ uint16_t codes[kSyms];
  __shared__ uint8_t lens[kSyms + 3];
  __shared__ uint32_t crc_tab[256];
  __shared__ uint32_t scan[kThreads];
  __shared__ uint32_t len_count[16];
  __shared__ uint32_t crc_pw[8];
  __shared__ uint32_t sh_sum_d, sh_sum_w, sh_nsym, sh_crc;

  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int i = find_image(tab.first_seg, tab.n, b);
  const int k = b - tab.first_seg[i];
  const int h = tab.h[i], w3 = 3 * tab.w[i];
  const uint32_t L = 1u + uint32_t(w3);
  const int64_t S = int64_t(h) * L;
  const int64_t nseg = segments(S);
  const Layout lay = image_layout(tab.base[i], h, nseg);
  const uint32_t j_first = uint32_t(k) * uint32_t(kSeg);  // S < 2^31
  const int len = S - j_first < kSeg ? int(S - j_first) : kSeg;
  const bool final = k == nseg - 1;
  const uint8_t* pic = tab.pic[i];
  const uint8_t* types = ws + lay.types;
  uint8_t* ob8 = reinterpret_cast<uint8_t*>(obuf);

  for (int e = t; e < kSlot / 4; e += kThreads) obuf[e] = 0;
  for (int s = t; s < kSyms; s += kThreads) hist[s] = s == 256 ? 1u : 0u;  // end-of-block is counted once
  crc_tab[t] = crc_table_entry(uint32_t(t));
  if (t < 16) len_count[t] = 0;
  if (t == 0) sh_sum_d = sh_sum_w = sh_nsym = sh_crc = 0;
  __syncthreads();

  // the segment's stream bytes: filtered as they load, counted, and summed for the Adler pair
  uint32_t sum_d = 0, sum_w = 0;  // at most 64 * 255 and 64 * 16384 * 255
  for (int q = t; q < (len + 3) / 4; q += kThreads) {
    const uint32_t j0 = j_first + 4u * uint32_t(q);
    uint32_t r = j0 / L, x = j0 - r * L;  // x == 0 is the row's type byte
    int ty = filter == 5 ? types[r] : filter;
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * q + e;
      if (j < len) {
        int v;
        if (x == 0) {
          v = ty;
        } else {
          const uint32_t px = x - 1;
          const uint8_t* cur = pic + size_t(r) * size_t(w3);
          const int val = cur[px], a = px >= 3 ? cur[px - 3] : 0;
          const int up = r ? cur[ptrdiff_t(px) - w3] : 0, c = (r && px >= 3) ? cur[ptrdiff_t(px) - 3 - w3] : 0;
          v = filter_byte(ty, val, a, up, c);
        }
        word |= uint32_t(v) << (8 * e);
        atomicAdd(&hist[v], 1u);
        sum_d += uint32_t(v);
        sum_w += uint32_t(len - j) * uint32_t(v);
        if (++x == L) {
          x = 0;
          ++r;
          if (j + 1 < len && filter == 5) ty = types[r];
        }
      }
    }
    seg[seg_index(q)] = word;
  }
  atomicAdd(&sh_sum_d, sum_d % kAdlerMod);
  atomicAdd(&sh_sum_w, sum_w % kAdlerMod);
  __syncthreads();

  // the symbols in use in the order of (count, value): every thread ranks its own
  for (int s = t; s < kSyms; s += kThreads) {
    const uint32_t f = hist[s];
    if (f) {
      const uint32_t key = (f << 9) | uint32_t(s);
      int rank = 0;
      for (int o = 0; o < kSyms; ++o) {
        const uint32_t fo = hist[o];
        rank += (fo && ((fo << 9) | uint32_t(o)) < key) ? 1 : 0;
      }
      rank_of[s] = uint16_t(rank);
      sorted_f[rank] = int(f);
      atomicAdd(&sh_nsym, 1u);
    }
  }
  __syncthreads();
  if (t == 0) huffman_lengths_limited(sorted_f, sorted_len, int(sh_nsym));  // at least two symbols: a byte and end-of-block
  __syncthreads();
  for (int s = t; s < kSyms; s += kThreads) {
    const int l = hist[s] ? sorted_len[rank_of[s]] : 0;
    lens[s] = uint8_t(l);
    if (l) atomicAdd(&len_count[l], 1u);
  }
  __syncthreads();
  {
    int count[16], first[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) count[l] = int(len_count[l]);
    canonical_first_codes(count, first);
    for (int s = t; s < kSyms; s += kThreads) {
      const int l = lens[s];
      int code = 0;
      if (l) {
        code = first[l];
        for (int o = 0; o < s; ++o) code += lens[o] == l ? 1 : 0;
      }
      codes[s] = uint16_t(reverse_bits(uint32_t(code), l));
    }
  }
  __syncthreads();

  // bits of every thread's run, and where they start
  uint32_t my_bits = 0;
  const int j_lo = t * kChunkBytes;
  for (int q = 0; q < kChunkWords; ++q) {
    const int j = j_lo + 4 * q;
    if (j >= len) break;
    const uint32_t word = seg[seg_index(t * kChunkWords + q)];
#pragma unroll
    for (int e = 0; e < 4; ++e) my_bits += (j + e < len) ? lens[(word >> (8 * e)) & 255u] : 0u;
  }
  scan[t] = my_bits;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    const uint32_t add = t >= d ? scan[t - d] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const uint32_t data_bits = scan[kThreads - 1];
  const uint32_t my_first = scan[t] - my_bits;
  const int64_t bits = kHeaderBits + int64_t(data_bits) + lens[256];
  const int dyn = dynamic_bytes(bits, final), sto = stored_bytes(len);
  const bool stored = dyn >= sto;
  const int P = stored ? sto : dyn;  // the chunk's data bytes, at ob8[8]

  if (t < 8) crc_pw[t] = crc_xpow((8ull * uint64_t((4 + P + kThreads - 1) / kThreads)) << t);
  if (t == 0) {
    ob8[0] = uint8_t(uint32_t(P) >> 24);
    ob8[1] = uint8_t(uint32_t(P) >> 16);
    ob8[2] = uint8_t(uint32_t(P) >> 8);
    ob8[3] = uint8_t(P);
    ob8[4] = 'I';
    ob8[5] = 'D';
    ob8[6] = 'A';
    ob8[7] = 'T';
  }
  if (stored) {  // block-uniform
    if (t == 0) {
      ob8[8] = final ? 1 : 0;
      ob8[9] = uint8_t(len);
      ob8[10] = uint8_t(len >> 8);
      ob8[11] = uint8_t(~len);
      ob8[12] = uint8_t(~len >> 8);
    }
    for (int j = t; j < len; j += kThreads) ob8[13 + j] = uint8_t(seg[seg_index(j >> 2)] >> (8 * (j & 3)));
  } else {
    constexpr uint32_t at = 64;  // the data's first bit
    if (t == 0) {
      // BFINAL, BTYPE 10, HLIT 0, HDIST 0, HCLEN 15; then the 19 lengths of the code-length code in the order
      // 16 17 18 0 8 7 ...: three zeros and sixteen fours
      put_bits(obuf, at, (final ? 1u : 0u) | (2u << 1) | (15u << 13), 17);
      for (int c = 3; c < 19; ++c) put_bits(obuf, at + 17 + 3 * c, 4u, 3);
      put_bits(obuf, at + 74 + 4 * 257, reverse_bits(1u, 4), 4);  // the one distance code, never used
      put_bits(obuf, at + kHeaderBits + data_bits, codes[256], lens[256]);
      if (!final) put_bits(obuf, at + 8u * uint32_t(((bits + 3 + 7) >> 3) + 2), 0xFFFFu, 16);  // 00 00 FF FF
    }
    for (int s = t; s < kSyms; s += kThreads) put_bits(obuf, at + 74 + 4 * s, reverse_bits(lens[s], 4), 4);
    uint32_t pos = at + kHeaderBits + my_first;
    uint32_t wi = pos >> 5;
    int nb = int(pos & 31);
    uint64_t acc = 0;
    for (int q = 0; q < kChunkWords; ++q) {
      const int j = j_lo + 4 * q;
      if (j >= len) break;
      const uint32_t word = seg[seg_index(t * kChunkWords + q)];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (j + e < len) {
          const uint32_t sym = (word >> (8 * e)) & 255u;
          acc |= uint64_t(codes[sym]) << nb;
          nb += lens[sym];
          if (nb >= 32) {
            atomicOr(&obuf[wi++], uint32_t(acc));
            acc >>= 32;
            nb -= 32;
          }
        }
      }
    }
    if (nb > 0 && uint32_t(acc)) atomicOr(&obuf[wi], uint32_t(acc));
  }
  __syncthreads();

  // CRC-32 of type + data: slices of K bytes that END at the chunk's end, so slice t is followed by (255 - t) K bytes
  {
    const int N = 4 + P, K = (N + kThreads - 1) / kThreads;
    const int start = N - (kThreads - t) * K, end = start + K;
    if (end > 0) {
      uint32_t reg = start <= 0 ? 0xFFFFFFFFu : 0u;
      for (int j = start < 0 ? 0 : start; j < end; ++j) reg = crc_tab[(reg ^ ob8[4 + j]) & 255u] ^ (reg >> 8);
      uint32_t m = 0x80000000u;  // x^0
      const int after = kThreads - 1 - t;
      for (int bit = 0; bit < 8; ++bit)
        if ((after >> bit) & 1) m = crc_mul(m, crc_pw[bit]);
      atomicXor(&sh_crc, crc_mul(reg, m));
    }
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t crc = sh_crc ^ 0xFFFFFFFFu;
    ob8[8 + P] = uint8_t(crc >> 24);
    ob8[9 + P] = uint8_t(crc >> 16);
    ob8[10 + P] = uint8_t(crc >> 8);
    ob8[11 + P] = uint8_t(crc);
    uint32_t* rec = reinterpret_cast<uint32_t*>(ws + lay.recs) + 4 * size_t(k);
    rec[0] = uint32_t(12 + P);
    rec[1] = (1u + sh_sum_d) % kAdlerMod;
    rec[2] = (uint32_t(len) + sh_sum_w) % kAdlerMod;
    rec[3] = uint32_t(len);
  }
  __syncthreads();
  uint32_t* slot = reinterpret_cast<uint32_t*>(ws + lay.slots + int64_t(k) * kSlot);
  for (int e = t; e < (12 + P + 3) / 4; e += kThreads) slot[e] = obuf[e];
}

// a workgroup per picture: every thread walks a run of consecutive segments, lane 0 joins the 256 runs
__global__ __launch_bounds__(kThreads) void png_scan_kernel(const PngTable tab, uint8_t* __restrict__ ws,
                                                            int64_t* __restrict__ sizes) {
  __shared__ int64_t run_bytes[kThreads];
  __shared__ uint32_t run_a[kThreads], run_b[kThreads], run_len[kThreads];
  const int t = threadIdx.x, i = blockIdx.x;
  const int h = tab.h[i];
  const int64_t nseg = segments(int64_t(h) * (1 + 3 * int64_t(tab.w[i])));
  const Layout lay = image_layout(tab.base[i], h, nseg);
  const uint32_t* recs = reinterpret_cast<const uint32_t*>(ws + lay.recs);
  int64_t* offs = reinterpret_cast<int64_t*>(ws + lay.offs);
  const int64_t per = (nseg + kThreads - 1) / kThreads;
  const int64_t k0 = t * per < nseg ? t * per : nseg, k1 = k0 + per < nseg ? k0 + per : nseg;
  int64_t bytes = 0;
  uint32_t a = 1, bsum = 0, len = 0;  // the Adler pair of no bytes
  for (int64_t k = k0; k < k1; ++k) {
    bytes += recs[4 * k];
    adler_combine(&a, &bsum, recs[4 * k + 1], recs[4 * k + 2], recs[4 * k + 3]);
    len = (len + recs[4 * k + 3]) % kAdlerMod;
  }
  run_bytes[t] = bytes;
  run_a[t] = a;
  run_b[t] = bsum;
  run_len[t] = len;
  __syncthreads();
  if (t == 0) {
    int64_t at = kFirstIdat;
    uint32_t ta = 1, tb = 0;
    for (int o = 0; o < kThreads; ++o) {
      const int64_t nb = run_bytes[o];
      run_bytes[o] = at;
      at += nb;
      adler_combine(&ta, &tb, run_a[o], run_b[o], run_len[o]);
    }
    ImageRec* rec = reinterpret_cast<ImageRec*>(ws + tab.base[i]);
    rec->total = at + 16 + 12;
    rec->adler = (tb << 16) | ta;
    rec->pad = 0;
    sizes[i] = at + 16 + 12;
  }
  __syncthreads();
  int64_t at = run_bytes[t];
  for (int64_t k = k0; k < k1; ++k) {
    offs[k] = at;
    at += recs[4 * k];
  }
}

__device__ inline uint8_t* put_be32(uint8_t* p, uint32_t v) {
  p[0] = uint8_t(v >> 24);
  p[1] = uint8_t(v >> 16);
  p[2] = uint8_t(v >> 8);
  p[3] = uint8_t(v);
  return p + 4;
}
// one small chunk, serially: length, type, data, CRC-32 of type and data
__device__ inline uint8_t* put_chunk(uint8_t* p, const char* type, const uint8_t* data, int n) {
  p = put_be32(p, uint32_t(n));
  uint32_t reg = 0xFFFFFFFFu;
  for (int e = 0; e < 4; ++e) {
    *p++ = uint8_t(type[e]);
    reg = crc_byte(reg, uint8_t(type[e]));
  }
  for (int e = 0; e < n; ++e) {
    *p++ = data[e];
    reg = crc_byte(reg, data[e]);
  }
  return put_be32(p, reg ^ 0xFFFFFFFFu);
}

__global__ __launch_bounds__(kThreads) void png_gather_kernel(const PngTable tab, const uint8_t* __restrict__ ws) {
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int all = tab.first_seg[tab.n];
  if (b >= all) {  // the picture's small chunks
    if (t != 0) return;
    const int i = b - all;
    const ImageRec* rec = reinterpret_cast<const ImageRec*>(ws + tab.base[i]);
    uint8_t* p = tab.out[i];
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int e = 0; e < 8; ++e) *p++ = sig[e];
    uint8_t ihdr[13];
    put_be32(ihdr, uint32_t(tab.w[i]));
    put_be32(ihdr + 4, uint32_t(tab.h[i]));
    ihdr[8] = 8;   // bit depth
    ihdr[9] = 2;   // colour type: RGB
    ihdr[10] = 0;  // compression
    ihdr[11] = 0;  // filter method
    ihdr[12] = 0;  // no interlace
    p = put_chunk(p, "IHDR", ihdr, 13);
    const uint8_t zhdr[2] = {0x78, 0x01};
    put_chunk(p, "IDAT", zhdr, 2);
    uint8_t adler[4];
    put_be32(adler, rec->adler);
    p = put_chunk(tab.out[i] + (rec->total - 28), "IDAT", adler, 4);
    put_chunk(p, "IEND", adler, 0);
    return;
  }
  const int i = find_image(tab.first_seg, tab.n, b);
  const int k = b - tab.first_seg[i];
  const int h = tab.h[i];
  const int64_t nseg = segments(int64_t(h) * (1 + 3 * int64_t(tab.w[i])));
  const Layout lay = image_layout(tab.base[i], h, nseg);
  const int nbytes = int(reinterpret_cast<const uint32_t*>(ws + lay.recs)[4 * size_t(k)]);
  const uint8_t* src = ws + lay.slots + int64_t(k) * kSlot;  // 16-byte aligned, readable to kSlot
  uint8_t* dst = tab.out[i] + reinterpret_cast<const int64_t*>(ws + lay.offs)[k];
  // whole words of the destination, each from the two source words it straddles
  int head = int((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
  if (head > nbytes) head = nbytes;
  const int words = (nbytes - head) >> 2;
  if (t < head) dst[t] = src[t];
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
  const int shift = 8 * (head & 3), at = head >> 2;  // head < 4
  for (int e = t; e < words; e += kThreads) {
    const uint32_t lo = s32[at + e];
    d32[e] = shift ? (lo >> shift) | (s32[at + e + 1] << (32 - shift)) : lo;
  }
  const int tail = head + 4 * words;
  if (tail + t < nbytes && t < 4) dst[tail + t] = src[tail + t];
}

}  // namespace

}  // namespace expo

using namespace expo;

namespace {

// bytes of workspace of images [base, base + m): the pictures' parts behind one another
int64_t group_workspace(const int* hs, const int* ws, int base, int m, int64_t* bases) {
  int64_t at = 0;
  for (int j = 0; j < m; ++j) {
    if (bases) bases[j] = at;
    const int h = hs[base + j];
    at = image_layout(at, h, png::segments(png::stream_bytes(h, ws[base + j]))).end;
  }
  return at;
}

}  // namespace

extern "C" {

int expo_png_segment_bytes(void) { return png::kSeg; }

int64_t expo_png_encode_bound(int h, int w) {
  const int64_t s = png::stream_bytes(h, w);
  if (s < 0) {
    fail(EXPO_E_BADARG, "h >= 1, w >= 1 and a filtered stream h (1 + 3 w) below 2^31 bytes required");
    return -1;
  }
  return png::file_bound(s);
}

size_t expo_png_encode_workspace_bytes(const int* hs, const int* ws, int n) {
  if (n < 1 || !hs || !ws) return 0;
  for (int i = 0; i < n; ++i)
    if (png::stream_bytes(hs[i], ws[i]) < 0) return 0;
  int64_t most = 0;  // a launch group at a time uses it
  for (int base = 0; base < n; base += kPngMaxImages) {
    const int64_t need = group_workspace(hs, ws, base, n - base < kPngMaxImages ? n - base : kPngMaxImages, nullptr);
    most = need > most ? need : most;
  }
  return size_t(most);
}

int expo_png_encode_ragged(const void* const* pics, const int* hs, const int* ws, int n, int filter, void* const* outs,
                           const int64_t* out_capacity, int64_t* sizes, void* workspace, size_t workspace_bytes,
                           void* stream) {
  // everything is checked before the first launch is enqueued
  if (n < 0) return fail(EXPO_E_BADARG, "n >= 0 required");
  if (filter < 0 || filter > 5) return fail(EXPO_E_BADARG, "filter must be 0..5 (None, Sub, Up, Average, Paeth, adaptive)");
  if (n == 0) return EXPO_OK;
  if (!hs || !ws) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (hs[i] < 1 || ws[i] < 1) return fail(EXPO_E_BADARG, "h >= 1, w >= 1 required");
    if (png::stream_bytes(hs[i], ws[i]) < 0)
      return fail(EXPO_E_BADARG, "the filtered stream h (1 + 3 w) of one picture must be smaller than 2^31 bytes");
  }
  if (!pics || !outs || !out_capacity || !sizes) return fail(EXPO_E_BADARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (!pics[i] || !outs[i]) return fail(EXPO_E_BADARG, "null picture pointer");
    if (out_capacity[i] < png::file_bound(png::stream_bytes(hs[i], ws[i])))
      return fail(EXPO_E_BADARG, "out_capacity below expo_png_encode_bound");
  }
  if (workspace_bytes < expo_png_encode_workspace_bytes(hs, ws, n)) return fail(EXPO_E_BADARG, "workspace too small");
  if (!workspace) return fail(EXPO_E_BADARG, "null workspace");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(EXPO_E_BADARG, "the workspace must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* wsp = static_cast<uint8_t*>(workspace);
  for (int base = 0; base < n; base += kPngMaxImages) {
    const int m = n - base < kPngMaxImages ? n - base : kPngMaxImages;
    PngTable tab = {};
    tab.n = m;
    group_workspace(hs, ws, base, m, tab.base);
    long rows = 0, segs = 0;
    for (int j = 0; j < m; ++j) {
      const int i = base + j;
      tab.pic[j] = static_cast<const uint8_t*>(pics[i]);
      tab.out[j] = static_cast<uint8_t*>(outs[i]);
      tab.h[j] = hs[i];
      tab.w[j] = ws[i];
      tab.first_row[j] = int(rows);
      tab.first_seg[j] = int(segs);
      rows += (hs[i] + kWaves - 1) / kWaves;
      segs += long(png::segments(png::stream_bytes(hs[i], ws[i])));
      if (rows > INT_MAX - kPngMaxImages || segs > INT_MAX - kPngMaxImages)
        return fail(EXPO_E_BADARG, "too many blocks in one launch");
    }
    tab.first_row[m] = int(rows);
    tab.first_seg[m] = int(segs);
    const dim3 block(kThreads);
    if (filter == 5) {
      hipLaunchKernelGGL(png_row_types_kernel, dim3(unsigned(rows)), block, 0, s, tab, wsp);
      HIP_TRY(hipGetLastError(), "png_row_types launch");
    }
    hipLaunchKernelGGL(png_segment_kernel, dim3(unsigned(segs)), block, 0, s, tab, wsp, filter);
    HIP_TRY(hipGetLastError(), "png_segment launch");
    hipLaunchKernelGGL(png_scan_kernel, dim3(unsigned(m)), block, 0, s, tab, wsp, sizes + base);
    HIP_TRY(hipGetLastError(), "png_scan launch");
    hipLaunchKernelGGL(png_gather_kernel, dim3(unsigned(segs + m)), block, 0, s, tab, static_cast<const uint8_t*>(wsp));
    HIP_TRY(hipGetLastError(), "png_gather launch");
  }
  return EXPO_OK;
}

}  // extern "C"
