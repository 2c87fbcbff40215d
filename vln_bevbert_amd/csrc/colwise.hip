// HBM-bound column kernels: K4 bias+erf-GELU / bias+ReLU (fwd/bwd) and the two-stage column reductions -- per-block
// partial sums (of these kernels and of the LayerNorm backward, layernorm.hip), then a finalize stage, single or batched;
// and the column sum for any column count.
//
// Reference call sites replaced:
//   BertIntermediate + gelu                pretrain_src/model/vilmodel.py:31-37,168-180
//   prediction heads' Linear - ReLU        pretrain_src/model/pretrain_cmt.py:34-71
//
// Layout: activations are (rows, C) row-major; a thread owns 4 (or 8) columns and walks contiguous rows.
#include <math.h>
#include <type_traits>

#include "rowops_common.h"

// p[b0 * stride] + p[(b0 + 16) * stride] + ... over b < nblocks, as ONE running fp32 sum in ascending b.  Only the loads
// are batched (16, then 4, then 1 in flight; one at a time, 32 - 64 dependent round trips per thread, the finalize
// kernels ran at 0.38 of the streaming rate): the adds and their order are those of the plain loop.
template <int U>
__device__ __forceinline__ void strided_sum_batches(const BB_GLOBAL float* __restrict__ p, int& b, int nblocks, size_t stride,
                                                    float& s) {
  for (; b + (U - 1) * 16 < nblocks; b += U * 16) {
    float v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = p[(size_t)(b + k * 16) * stride];
#pragma unroll
    for (int k = 0; k < U; ++k) s += v[k];
  }
}
__device__ __forceinline__ float strided_sum16(const float* p_, int b0, int nblocks, size_t stride) {
  const BB_GLOBAL float* __restrict__ p = (const BB_GLOBAL float*)p_;
  float s = 0.f;
  int b = b0;
  strided_sum_batches<16>(p, b, nblocks, stride, s);
  strided_sum_batches<4>(p, b, nblocks, stride, s);
  strided_sum_batches<1>(p, b, nblocks, stride, s);
  return s;
}

// out_w[c] (+)= sum_b partials[b][w][c] for every w with a non-null output.  Block = 64 columns x 16 partial groups:
// coalesced 256-B reads, 16 independent running sums per column, fixed combination order => deterministic.
struct FinalizeOut { float* out[3]; };
__global__ __launch_bounds__(1024) void colsum_finalize_kernel(const float* __restrict__ partials, int nblocks,
                                                              int nwhich, int C, FinalizeOut o, int accumulate) {
  __shared__ float sh[16][64];
  const int which = blockIdx.y;
  float* out = o.out[which];
  if (out == nullptr) return;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int c = blockIdx.x * 64 + tx;
  float s = 0.f;
  if (c < C) s = strided_sum16(partials + (size_t)which * C + c, ty, nblocks, (size_t)nwhich * C);
  sh[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < C) {
    float t = sh[0][tx];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += sh[k][tx];
    out[c] = accumulate ? out[c] + t : t;
  }
}
void launch_finalize(const float* partials, int nblocks, int nwhich, int C, float* o0, float* o1, float* o2,
                     int accumulate, hipStream_t stream) {
  FinalizeOut o;
  o.out[0] = o0; o.out[1] = o1; o.out[2] = o2;
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3((C + 63) / 64, nwhich), dim3(64, 16), 0, stream, partials, nblocks,
                     nwhich, C, o, accumulate);
}

// Batched second stage: ONE launch finishes every pending column reduction of a backward pass (LayerNorm gamma / beta /
// bias, GELU bias, projection biases: ~110 per training step, each a 6-8 us launch of a few dozen workgroups when issued
// one by one).  A task = 64 columns of one output vector; the host builds the task table once per distinct step shape
// (ops.ReduceQueue) and keeps it in device memory.  Same arithmetic and summation order as colsum_finalize_kernel.
struct FinalizeTask {
  const float* partials;   // [nblocks][row_stride] floats
  float* out;              // 64-column slice of the output vector
  int nblocks, row_stride, col0, ncols, accumulate, pad;
};
__global__ __launch_bounds__(1024) void multi_finalize_kernel(const FinalizeTask* __restrict__ tasks) {
  __shared__ float sh[16][64];
  const FinalizeTask t = tasks[blockIdx.x];
  const int tx = threadIdx.x, ty = threadIdx.y;
  float s = 0.f;
  if (tx < t.ncols) s = strided_sum16(t.partials + t.col0 + tx, ty, t.nblocks, (size_t)t.row_stride);
  sh[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && tx < t.ncols) {
    float v = sh[0][tx];
#pragma unroll
    for (int k = 1; k < 16; ++k) v += sh[k][tx];
    t.out[tx] = t.accumulate ? t.out[tx] + v : v;
  }
}

// =============================================================================================
// bias + erf-GELU forward / backward, and a plain column sum (QKV bias grads)
// =============================================================================================
// Same decomposition as the backward below: grid (row groups, 1024-column slices), a thread owns 4 columns (its bias is
// loaded once) and walks CONTIGUOUS rows with 8 independent loads in flight.  The first version -- a flat grid-stride
// loop, one chunk per thread and iteration, the column recomputed as (i * 4) % C on a 64-bit index (~60 instructions
// per chunk) -- ran at 3.2 TB/s.
// ACT 0: erf-GELU (BertIntermediate, vilmodel.py:31-37); ACT 1: ReLU (the prediction heads' Linear - ReLU - LayerNorm - Linear,
// pretrain_src/model/pretrain_cmt.py:34-71)
template <typename T, int ACT> __device__ __forceinline__ float4 act4_of(float4 a, float4 b) {
  if (ACT == 0) return gelu4_of<T>(a, b);
  return make_float4(fmaxf(a.x + b.x, 0.f), fmaxf(a.y + b.y, 0.f), fmaxf(a.z + b.z, 0.f), fmaxf(a.w + b.w, 0.f));
}
template <typename T, int ACT> __device__ __forceinline__ float4 act_grad4_of(float4 d, float4 a, float4 b) {
  if (ACT == 0) return gelu_grad4_of<T>(d, a, b);
  return make_float4(a.x + b.x > 0.f ? d.x : 0.f, a.y + b.y > 0.f ? d.y : 0.f, a.z + b.z > 0.f ? d.z : 0.f,
                     a.w + b.w > 0.f ? d.w : 0.f);
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void bias_gelu_fwd_kernel(const T* __restrict__ x, const float* __restrict__ bias,
                                                            T* __restrict__ y, int rows, int C) {
  const int c0 = blockIdx.y * 1024 + threadIdx.x * 4;
  if (c0 >= C) return;
  const float4 b = *reinterpret_cast<const float4*>(bias + c0);
  const int rpb = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
  int r = blockIdx.x * rpb;
  rows = (r + rpb < rows) ? r + rpb : rows;
  constexpr int R = 8;
  for (; r + R - 1 < rows; r += R) {
    float4 a[R];
#pragma unroll
    for (int k = 0; k < R; ++k) a[k] = ld4<T>(x + (size_t)(r + k) * C + c0);
#pragma unroll
    for (int k = 0; k < R; ++k) st4<T>(y + (size_t)(r + k) * C + c0, act4_of<T, ACT>(a[k], b));
  }
  for (; r < rows; ++r) st4<T>(y + (size_t)r * C + c0, act4_of<T, ACT>(ld4<T>(x + (size_t)r * C + c0), b));
}

// bf16, 16-byte accesses: a thread owns 8 columns (128 threads per 1024-column slice)
__device__ __forceinline__ void bf16x8_to_f32(const uint4& u, float4& lo, float4& hi) {
  lo = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                   __uint_as_float(u.y & 0xffff0000u));
  hi = make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u), __uint_as_float(u.w << 16),
                   __uint_as_float(u.w & 0xffff0000u));
}
__device__ __forceinline__ uint4 f32_to_bf16x8(const float4& lo, const float4& hi) {
  return make_uint4(pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w));
}
__global__ __launch_bounds__(128) void bias_gelu_fwd8_kernel(const bf16_raw* __restrict__ x, const float* __restrict__ bias,
                                                             bf16_raw* __restrict__ y, int rows, int C) {
  const int c0 = blockIdx.y * 1024 + threadIdx.x * 8;
  if (c0 >= C) return;
  const float4 b0 = *reinterpret_cast<const float4*>(bias + c0), b1 = *reinterpret_cast<const float4*>(bias + c0 + 4);
  const int rpb = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
  int r = blockIdx.x * rpb;
  rows = (r + rpb < rows) ? r + rpb : rows;
  constexpr int R = 8;
  for (; r + R - 1 < rows; r += R) {
    uint4 a[R];
#pragma unroll
    for (int k = 0; k < R; ++k) a[k] = *reinterpret_cast<const uint4*>(x + (size_t)(r + k) * C + c0);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      float4 lo, hi;
      bf16x8_to_f32(a[k], lo, hi);
      *reinterpret_cast<uint4*>(y + (size_t)(r + k) * C + c0) =
          f32_to_bf16x8(gelu4_of<bf16_raw>(lo, b0), gelu4_of<bf16_raw>(hi, b1));
    }
  }
  for (; r < rows; ++r) {
    float4 lo, hi;
    bf16x8_to_f32(*reinterpret_cast<const uint4*>(x + (size_t)r * C + c0), lo, hi);
    *reinterpret_cast<uint4*>(y + (size_t)r * C + c0) = f32_to_bf16x8(gelu4_of<bf16_raw>(lo, b0), gelu4_of<bf16_raw>(hi, b1));
  }
}

// MODE 0: dx = dy * gelu'(x + bias) ; partial column sums of dx.   MODE 1: plain column sums of dy (no dx).
// MODE 2: as 0 with ReLU (dx = dy where x + bias > 0).
// Grid (row groups, column slices of 1024): thread t owns 4 columns and walks its row group 4 rows at a time
// (8 independent loads per tensor in flight); partials[blockIdx.x][C].
template <typename T, int MODE>
__global__ __launch_bounds__(256) void colwise_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                          const float* __restrict__ bias, T* __restrict__ dx,
                                                          float* __restrict__ partials, int rows, int C) {
  const int c0 = blockIdx.y * 1024 + threadIdx.x * 4;
  if (c0 >= C) return;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (MODE != 1) b = *reinterpret_cast<const float4*>(bias + c0);
  // block b owns the CONTIGUOUS rows [b * rpb, (b + 1) * rpb): the eight rows a thread has in flight are neighbours
  const int rpb = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
  int r = blockIdx.x * rpb;
  rows = (r + rpb < rows) ? r + rpb : rows;
  constexpr int R = 8;                   // rows in flight per thread
  for (; r + R - 1 < rows; r += R) {
    float4 d[R], a[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      d[k] = ld4<T>(dy + (size_t)(r + k) * C + c0);
      if (MODE != 1) a[k] = ld4<T>(x + (size_t)(r + k) * C + c0);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (MODE != 1) {
        d[k] = act_grad4_of<T, MODE == 2 ? 1 : 0>(d[k], a[k], b);
        st4<T>(dx + (size_t)(r + k) * C + c0, d[k]);
      }
      add4(acc, d[k]);
    }
  }
  for (; r < rows; ++r) {
    float4 d = ld4<T>(dy + (size_t)r * C + c0);
    if (MODE != 1) {
      const float4 a = ld4<T>(x + (size_t)r * C + c0);
      d = act_grad4_of<T, MODE == 2 ? 1 : 0>(d, a, b);
      st4<T>(dx + (size_t)r * C + c0, d);
    }
    add4(acc, d);
  }
  *reinterpret_cast<float4*>(partials + (size_t)blockIdx.x * C + c0) = acc;
}

// Column sums for ANY column count (the 30 522-wide vocabulary bias, the 1-wide heads: C % 4 != 0 rules out the float4
// kernels above): out[c] (+)= sum_r dy[r][c].  Wide: workgroup = 64 columns x 4 row groups, folded pairwise.  Narrow
// (C <= 4): the whole workgroup walks the rows.  Fixed summation order in both.
template <typename T>
__global__ __launch_bounds__(256) void colsum_any_kernel(const T* __restrict__ dy, float* __restrict__ out, int rows, int C,
                                                         int accumulate) {
  __shared__ float s_part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (C <= 4) {
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
      for (int r = threadIdx.x; r < rows; r += 256) s += io<T>::ld(dy + (size_t)r * C + c);
      s = wave_sum(s);
      if (lane == 0) s_part[wave][0] = s;
      __syncthreads();
      if (threadIdx.x == 0) {
        const float t = (s_part[0][0] + s_part[1][0]) + (s_part[2][0] + s_part[3][0]);
        out[c] = accumulate ? out[c] + t : t;
      }
      __syncthreads();
    }
    return;
  }
  const int c = blockIdx.x * 64 + lane;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < C) {
    int r = wave;
    for (; r + 12 < rows; r += 16) {
      s0 += io<T>::ld(dy + (size_t)r * C + c);
      s1 += io<T>::ld(dy + (size_t)(r + 4) * C + c);
      s2 += io<T>::ld(dy + (size_t)(r + 8) * C + c);
      s3 += io<T>::ld(dy + (size_t)(r + 12) * C + c);
    }
    for (; r < rows; r += 4) s0 += io<T>::ld(dy + (size_t)r * C + c);
  }
  s_part[wave][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (wave == 0 && c < C) {
    const float t = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
    out[c] = accumulate ? out[c] + t : t;
  }
}

// =============================================================================================
// C ABI
// =============================================================================================
BEVBERT_API int bevbert_colsum_any(const void* dy, float* out, int rows, int C, int dtype, int accumulate,
                                   hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && C > 0, "colsum_any: rows=%d C=%d", rows, C);
  if (rows == 0) return BB_OK;
  const dim3 grid(C <= 4 ? 1 : (C + 63) / 64);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(colsum_any_kernel<T>, grid, dim3(256), 0, stream, (const T*)dy, out, rows, C, accumulate);
  });
  if (!type_ok) return bb_dtype_unsupported("colsum_any", dtype);
  BB_CHECK_LAUNCH("colsum_any");
  return BB_OK;
}

// row groups of the column kernels (and of the LayerNorm backward, whose partial rows go through the same second stage):
// enough blocks to fill the chip, <= 1024 partial rows.  Rows per block: 16 from 8 192 rows
// up, i.e. the cap for the 28 224-row BEV problems: 1 024 blocks = four waves per SIMD.  Until round 6 the cap was 512 (two
// waves per SIMD): the fp32-stream LayerNorm backward, three input streams of 2 + 4 + 4 bytes per element and a reduction
// between its loads and its stores, ran at 4.1 TB/s; with 1 024 blocks 5.15 TB/s (84.3 -> 67.4 us; 768: 70.3, 1 280: 78.6 --
// an uneven last round --, 2 048: 69.2), the bf16 LayerNorm backward and the GELU backward do not care (31.4 -> 30.0,
// 105.4 -> 104.1 us), the bare column sums lose 0.8 us (r06al).  Below 8 192 rows the kernels are latency-bound -- a wave walks its rows one after the other, every row
// a dependent load -> reduce -> store chain -- and 10 rows per block (two or three per wave; 512 blocks for the 5 120 text
// rows instead of 320) shortens that chain; up to 512 blocks the fp32-stream LayerNorm backward also loads a wave's next
// row while it reduces the current one (ln_res32_bwd_loads_ahead).
int colwise_max_blocks() { return 1024; }
int colwise_blocks(int rows) {
  const int per = rows >= 8192 ? 16 : 10;
  int nb = (rows + per - 1) / per;
  if (nb > colwise_max_blocks()) nb = colwise_max_blocks();
  return nb < 1 ? 1 : nb;
}

// workspace: >= bevbert_colsum_workspace_floats(3*H) floats
BEVBERT_API int64_t bevbert_colsum_workspace_floats(int total_cols) { return (int64_t)colwise_max_blocks() * total_cols; }

// Two-stage column reductions, split: layernorm_bwd / bias_gelu_bwd called with NULL parameter-gradient outputs leave
// their per-block partial sums in `workspace` ([bevbert_colsum_partial_rows(rows)][nwhich][C] floats); this entry is the
// second stage.  The host runs it on the weight-gradient stream, off the activation-gradient critical path.
BEVBERT_API int bevbert_colsum_partial_rows(int rows) { return colwise_blocks(rows); }

BEVBERT_API int bevbert_colsum_finalize(const float* partials, int nblocks, int nwhich, int C, float* out0, float* out1,
                                        float* out2, int accumulate, hipStream_t stream) {
  BB_REQUIRE(nblocks >= 1 && nwhich >= 1 && nwhich <= 3 && C >= 1, "colsum_finalize: bad shape (%d, %d, %d)", nblocks, nwhich, C);
  launch_finalize(partials, nblocks, nwhich, C, out0, out1, out2, accumulate, stream);
  BB_CHECK_LAUNCH("colsum_finalize");
  return BB_OK;
}

static int bias_act_fwd(const void* x, const float* bias, void* y, int rows, int C, int dtype, int act, hipStream_t stream) {
  BB_REQUIRE(C % 4 == 0, "bias_act_fwd: C=%d must be a multiple of 4", C);
  BB_REQUIRE(act == 0 || act == 1, "bias_act_fwd: activation %d (0 erf-GELU, 1 ReLU)", act);
  if (rows <= 0) return BB_OK;
  const dim3 grid(elementwise_row_groups(rows), (C + 1023) / 1024);
  if (dtype == BB_BF16 && act == 0 && C % 8 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0) {   // 71 vs 76 us at 28224 x 3072
    hipLaunchKernelGGL(bias_gelu_fwd8_kernel, grid, dim3(128), 0, stream, (const bf16_raw*)x, bias, (bf16_raw*)y, rows, C);
  } else {
    const bool type_ok = bb_with_type(dtype, [&](auto t) {
      using T = decltype(t);
      bb_with_int<0, 1>(act, [&](auto a) {
        hipLaunchKernelGGL((bias_gelu_fwd_kernel<T, decltype(a)::value>), grid, dim3(256), 0, stream, (const T*)x, bias, (T*)y, rows, C);
      });
    });
    if (!type_ok) return bb_dtype_unsupported("bias_act_fwd", dtype);
  }
  BB_CHECK_LAUNCH("bias_act_fwd");
  return BB_OK;
}

static int bias_act_bwd(const void* dy, const void* x, const float* bias, void* dx, float* dbias, float* workspace, int rows,
                        int C, int dtype, int accumulate, int act, hipStream_t stream) {
  BB_REQUIRE(C % 4 == 0, "bias_act_bwd: C=%d must be a multiple of 4", C);
  BB_REQUIRE(act == 0 || act == 1, "bias_act_bwd: activation %d (0 erf-GELU, 1 ReLU)", act);
  if (rows <= 0) return BB_OK;
  const int nb = colwise_blocks(rows);
  const dim3 grid(nb, (C + 1023) / 1024);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    bb_with_int<0, 1>(act, [&](auto a) {
      constexpr int MODE = decltype(a)::value == 0 ? 0 : 2;      // of colwise_bwd_kernel: 0 erf-GELU, 2 ReLU
      hipLaunchKernelGGL((colwise_bwd_kernel<T, MODE>), grid, dim3(256), 0, stream, (const T*)dy, (const T*)x, bias, (T*)dx, workspace, rows, C);
    });
  });
  if (!type_ok) return bb_dtype_unsupported("bias_act_bwd", dtype);
  BB_CHECK_LAUNCH("bias_act_bwd");
  if (dbias) {
    launch_finalize(workspace, nb, 1, C, dbias, nullptr, nullptr, accumulate, stream);
    BB_CHECK_LAUNCH("bias_act_bwd finalize");
  }
  return BB_OK;
}

BEVBERT_API int bevbert_bias_gelu_fwd(const void* x, const float* bias, void* y, int rows, int C, int dtype,
                                      hipStream_t stream) {
  return bias_act_fwd(x, bias, y, rows, C, dtype, 0, stream);
}

BEVBERT_API int bevbert_bias_gelu_bwd(const void* dy, const void* x, const float* bias, void* dx, float* dbias,
                                      float* workspace, int rows, int C, int dtype, int accumulate,
                                      hipStream_t stream) {
  return bias_act_bwd(dy, x, bias, dx, dbias, workspace, rows, C, dtype, accumulate, 0, stream);
}

// The prediction heads' Linear -> ReLU (pretrain_src/model/pretrain_cmt.py:34-71) on the same kernels.
BEVBERT_API int bevbert_bias_relu_fwd(const void* x, const float* bias, void* y, int rows, int C, int dtype,
                                      hipStream_t stream) {
  return bias_act_fwd(x, bias, y, rows, C, dtype, 1, stream);
}

BEVBERT_API int bevbert_bias_relu_bwd(const void* dy, const void* x, const float* bias, void* dx, float* dbias,
                                      float* workspace, int rows, int C, int dtype, int accumulate,
                                      hipStream_t stream) {
  return bias_act_bwd(dy, x, bias, dx, dbias, workspace, rows, C, dtype, accumulate, 1, stream);
}

BEVBERT_API int bevbert_colsum(const void* dy, float* out, float* workspace, int rows, int C, int dtype, int accumulate,
                               hipStream_t stream) {
  BB_REQUIRE(C % 4 == 0, "colsum: C=%d must be a multiple of 4", C);
  if (rows <= 0) return BB_OK;
  const int nb = colwise_blocks(rows);
  const dim3 grid(nb, (C + 1023) / 1024);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((colwise_bwd_kernel<T, 1>), grid, dim3(256), 0, stream, (const T*)dy, nullptr, nullptr, nullptr, workspace, rows, C);
  });
  if (!type_ok) return bb_dtype_unsupported("colsum", dtype);
  BB_CHECK_LAUNCH("colsum");
  launch_finalize(workspace, nb, 1, C, out, nullptr, nullptr, accumulate, stream);
  BB_CHECK_LAUNCH("colsum finalize");
  return BB_OK;
}

// First stage of bevbert_colsum alone: partials [bevbert_colsum_partial_rows(rows)][C]; the second stage goes through
// bevbert_multi_finalize together with the other pending reductions of the step.
BEVBERT_API int bevbert_colsum_partials(const void* dy, float* partials, int rows, int C, int dtype, hipStream_t stream) {
  BB_REQUIRE(C % 4 == 0 && rows > 0, "colsum_partials: C=%d must be a multiple of 4, rows=%d positive", C, rows);
  const int nb = colwise_blocks(rows);
  const dim3 grid(nb, (C + 1023) / 1024);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((colwise_bwd_kernel<T, 1>), grid, dim3(256), 0, stream, (const T*)dy, nullptr, nullptr, nullptr, partials, rows, C);
  });
  if (!type_ok) return bb_dtype_unsupported("colsum_partials", dtype);
  BB_CHECK_LAUNCH("colsum_partials");
  return BB_OK;
}

// tasks: device array of `ntasks` 40-byte records {u64 partials, u64 out, i32 nblocks, row_stride, col0, ncols, accumulate, pad}
BEVBERT_API int bevbert_multi_finalize(const void* tasks, int ntasks, hipStream_t stream) {
  static_assert(sizeof(FinalizeTask) == 40, "FinalizeTask is part of the C ABI");
  if (ntasks <= 0) return BB_OK;
  BB_REQUIRE(tasks != nullptr, "multi_finalize: null task table");
  hipLaunchKernelGGL(multi_finalize_kernel, dim3(ntasks), dim3(64, 16), 0, stream, (const FinalizeTask*)tasks);
  BB_CHECK_LAUNCH("multi_finalize");
  return BB_OK;
}
