// What more than one of the row-kernel sources (layernorm.hip, colwise.hip, optimizer.hip) needs: the row-group count of
// the column kernels with its second stage, and the global-address-space loads of the task-table kernels.
#pragma once
#include "common.h"

// Defined once, in colwise.hip: the LayerNorm backward and the column kernels must agree on the number of partial rows.
void launch_finalize(const float* partials, int nblocks, int nwhich, int C, float* o0, float* o1, float* o2,
                     int accumulate, hipStream_t stream);
int colwise_max_blocks();
int colwise_blocks(int rows);

// Loads through global-address-space pointers (global_load: a pointer read out of a task record is otherwise a flat one,
// whose loads also wait on the LDS counter and whose stores fence later loads)
typedef float bb_f4v __attribute__((ext_vector_type(4)));
typedef uint32_t bb_u2v __attribute__((ext_vector_type(2)));
#define BB_GLOBAL __attribute__((address_space(1)))
template <typename T> __device__ __forceinline__ float4 gld4(const BB_GLOBAL T* p);
template <> __device__ __forceinline__ float4 gld4<float>(const BB_GLOBAL float* p) {
  const bb_f4v v = *reinterpret_cast<const BB_GLOBAL bb_f4v*>(p);
  return make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ float4 gld4<bf16_raw>(const BB_GLOBAL bf16_raw* p) {
  const bb_u2v u = *reinterpret_cast<const BB_GLOBAL bb_u2v*>(p);
  return make_float4(__uint_as_float(u[0] << 16), __uint_as_float(u[0] & 0xffff0000u), __uint_as_float(u[1] << 16),
                     __uint_as_float(u[1] & 0xffff0000u));
}
