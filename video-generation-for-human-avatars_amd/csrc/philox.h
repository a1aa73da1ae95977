// Philox4x32-10, the counter-based generator behind everything here that is random on the device and has
// to be regenerated bit for bit: the LoRA dropout mask (lora_dropout.hip) and the stochastic rounding of
// the bf16 parameter store (optim.hip, prodigy.hip). One call gives four 32-bit words, used as eight
// 16-bit lanes.
#pragma once
#include "common.h"

namespace ltx {

struct Philox4 {
  uint32_t v[4];
};

// Philox4x32-10 (Salmon et al., Random123): ten rounds, the key bumped between rounds
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                          uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    // one 32 x 32 -> 64 bit product per word (a single v_mad_u64_u32; written as a high and a low
    // multiply the compiler issues two quarter-rate instructions)
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the 16-bit lane of column k % 8 = j: low half of o[j / 2] for even j, high half for odd j
__host__ __device__ __forceinline__ uint32_t mask_lane(const Philox4& o, int j) {
  return (o.v[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
}

// ---- stochastic rounding of an f32 value to bf16 (FusedAdamW / FusedProdigy bf16_update="stochastic") ----
// The 16-bit r decides: the bf16 bits of a finite x are (bits(x) + r) >> 16, which rounds the magnitude up
// with probability (discarded 16 bits) / 2^16 and leaves a representable x alone for every r; the largest
// finite pattern plus 0xffff stays below 2^32 (and may become inf, as round-to-nearest would). NaN and
// +-inf take the round-to-nearest conversion.
__device__ __forceinline__ bf16_t sr_bf16(float x, uint32_t r) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7f800000u) == 0x7f800000u) return f2bf(x);
  return (bf16_t)((u + r) >> 16);
}

// the generator's call for the 8 elements i & ~7 .. i | 7 of parameter `ordinal` at its step `step`:
// counter (lo32(i >> 3), hi32(i >> 3), ordinal, step mod 2^32), key (seed lo, seed hi); element i takes
// lane i & 7 by mask_lane's rule
__device__ __forceinline__ Philox4 sr_philox(int64_t i, uint32_t ordinal, uint32_t step, uint32_t k0, uint32_t k1) {
  const uint64_t q = (uint64_t)i >> 3;
  return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), ordinal, step, k0, k1);
}

}  // namespace ltx
