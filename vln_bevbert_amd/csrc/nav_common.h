// Graph-distance helpers shared by the fine-tune supervision kernels (nav_expert.hip, nav_obj.hip).
#pragma once
#include "common.h"

#define NE_INF __builtin_inf()

// dist (N,N) f64 of one scan; any node id outside [0, N) reads as unreachable.
__device__ __forceinline__ double ne_d(const double* __restrict__ d, int N, int u, int v) {
  return ((unsigned)u < (unsigned)N && (unsigned)v < (unsigned)N) ? d[(size_t)u * N + v] : NE_INF;
}

// sum of d[p[i]][p[i + 1]] over the n nodes of a path, left to right (the order of both _eval_item's length sums).
__device__ __forceinline__ double ne_path_length(const double* __restrict__ d, int N, const int* __restrict__ p, int n) {
  double len = 0.0;
  for (int i = 0; i + 1 < n; ++i) len += ne_d(d, N, p[i], p[i + 1]);
  return len;
}
