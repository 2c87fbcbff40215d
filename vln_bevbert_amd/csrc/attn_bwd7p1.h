// The 7 + 1-wave single-pass backward (attn_bwd7p1.hip, generations 2 and 3 of one kernel body): LDS map, the packed bf16
// dot product.  No code that ends up in the kernel besides dot2_bf16: the shared parts of the body are lambdas inside it.
#pragma once
#include "attn_mfma_common.h"

#define B2_LDS_DS 36                      // row stride (bf16) of the dS image: 32 queries + 4 (conflict-free 8-byte writes)
#define B2_NKEYW 7                        // key waves
#define B2_NK (64 * B2_NKEYW)             // keys covered: 448

struct B2Lds {
  static constexpr int k_off = 0;                                   // [448][LDT] bf16   K, row-major, whole kernel
  static constexpr int ds_off = k_off + B2_NK * LDT * 2;            // [2][448][36] bf16 dS of a 32-query step
  static constexpr int q_off = ds_off + 2 * B2_NK * B2_LDS_DS * 2;  // [2][32][LDT] bf16 Q tile
  static constexpr int do_off = q_off + 2 * 32 * LDT * 2;           // [2][32][LDT] bf16 dO tile
  static constexpr int stat_off = do_off + 2 * 32 * LDT * 2;        // [2][2][32] float  lse (log2 domain), delta / ks
  static constexpr int bytes = stat_off + 2 * 2 * 32 * 4;
};

// a.lo * b.lo + a.hi * b.hi + acc on two packed bf16 pairs (v_dot2c_f32_bf16): products exact in fp32, fp32 accumulation
typedef __bf16 bb_bf16pair __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dot2_bf16(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bb_bf16pair, a), __builtin_bit_cast(bb_bf16pair, b), acc, false);
}
