// codes_loader.h -- the load of one lane-row of integer image codes, shared by the units that read the files' codes at
// pixel_io.h's coalesced positions (chain_fused_codes.hip, codes_lut.hip).
#pragma once
#include "pixel_io.h"

namespace expo {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// the NB = PPV * C * sizeof(CT) code bytes of one lane-row at byte offset off (a multiple of NB; the base is 4-byte
// aligned), with the widest load their size allows
template <typename CT, int NB, int AUX>
__device__ __forceinline__ void load_code_row(__amdgpu_buffer_rsrc_t rin, int off, CT* c) {
  if constexpr (NB == 16) {
    const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rin, off, 0, AUX);
    __builtin_memcpy(c, &q, NB);
  } else if constexpr (NB == 12) {
    const u32x3_t q = __builtin_amdgcn_raw_buffer_load_b96(rin, off, 0, AUX);
    __builtin_memcpy(c, &q, NB);
  } else if constexpr (NB == 8) {
    const u32x2_t q = __builtin_amdgcn_raw_buffer_load_b64(rin, off, 0, AUX);
    __builtin_memcpy(c, &q, NB);
  } else if constexpr (NB == 4) {
    const uint32_t q = __builtin_amdgcn_raw_buffer_load_b32(rin, off, 0, AUX);
    __builtin_memcpy(c, &q, NB);
  } else if constexpr (NB % 2 == 0) {  // 2 or 6 bytes: 2-byte aligned
    uint16_t q[NB / 2];
#pragma unroll
    for (int k = 0; k < NB / 2; ++k) q[k] = __builtin_amdgcn_raw_buffer_load_b16(rin, off + 2 * k, 0, AUX);
    __builtin_memcpy(c, q, NB);
  } else {  // 1 or 3 bytes
    uint8_t q[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) q[k] = __builtin_amdgcn_raw_buffer_load_b8(rin, off + k, 0, AUX);
    __builtin_memcpy(c, q, NB);
  }
}

}  // namespace expo
