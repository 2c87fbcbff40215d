// Element-wise kernels: dropout + residual add (with the loader's fp32 -> bf16 cast), the global map's graph-aware
// attention bias and its backward, and the test hook that materialises a dropout keep-mask.
//
// Reference call sites replaced:
//   sprel_linear (graph bias)              pretrain_src/model/vilmodel.py:543-546, 575-577
#include <math.h>
#include <type_traits>

#include "common.h"

// y = residual + dropout(x)   (residual optional; input and output dtypes independent: fuses the fp32 -> bf16 cast of
// the loader's features into their feature dropout).  Mask = the library's counter-based stream (common.h).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void dropout_add_kernel(const TI* __restrict__ x, const TO* __restrict__ residual,
                                                          TO* __restrict__ y, size_t n4, float keep_scale,
                                                          uint32_t thr, uint32_t key, const uint32_t* __restrict__ salt) {
  key = bb_salted(key, salt);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 a = bb_drop4(ld4<TI>(x + i * 4), (uint32_t)(i * 4), key, thr, keep_scale);   // n < 2^32 (checked by the entry)
    if (residual != nullptr) add4(a, ld4<TO>(residual + i * 4));
    st4<TO>(y + i * 4, a);
  }
}

// Graph-aware attention bias of the global-map encoder (vilmodel.py:543-546, 575-577: sprel_linear = nn.Linear(1, 1) on
// the pairwise node distances): bias = dists * w + b with w, b read from the parameters in device memory; and its backward
// over the per-head, per-layer bias gradients the attention kernels leave: dw = sum dbias * dists, db = sum dbias.  One
// workgroup, a fixed summation order (the tensors are a few MB and the global-map branch runs beside the BEV encoder).
__global__ __launch_bounds__(256) void graph_bias_fwd_kernel(const float* __restrict__ dists, const float* __restrict__ w,
                                                             const float* __restrict__ b, float* __restrict__ out, int n) {
  const float ww = *w, bb = *b;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = dists[i] * ww + bb;
}
// stage 1: workgroup g sums a contiguous run of elements -> partials[g] = (sum dbias * dists, sum dbias); stage 2: one
// wave folds the partials in ascending order and adds them to the two gradients
__global__ __launch_bounds__(256) void graph_bias_bwd_kernel(const float* __restrict__ dbias, const float* __restrict__ dists,
                                                             uint32_t n, uint32_t per_sample, uint32_t per_layer,
                                                             uint32_t nh_gg, uint32_t gg, float2* __restrict__ partials) {
  // dbias: (layers, B, nh, G, G); element e -> sample (e % per_layer) / nh_gg, pair e % gg
  const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  const uint32_t lo = blockIdx.x * per, hi = min(n, lo + per);
  float sw = 0.f, sb = 0.f;
  for (uint32_t e = lo + threadIdx.x; e < hi; e += 256) {
    const float d = dbias[e];
    const uint32_t r = e % per_layer;
    sw = fmaf(d, dists[(r / nh_gg) * per_sample + r % gg], sw);
    sb += d;
  }
  __shared__ float s_w[4], s_b[4];
  sw = wave_sum(sw);
  sb = wave_sum(sb);
  if ((threadIdx.x & 63) == 0) { s_w[threadIdx.x >> 6] = sw; s_b[threadIdx.x >> 6] = sb; }
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = make_float2((s_w[0] + s_w[1]) + (s_w[2] + s_w[3]), (s_b[0] + s_b[1]) + (s_b[2] + s_b[3]));
}
__global__ __launch_bounds__(64) void graph_bias_finalize_kernel(const float2* __restrict__ partials, int nb,
                                                                 float* __restrict__ dw, float* __restrict__ db) {
  float sw = 0.f, sb = 0.f;
  for (int i = threadIdx.x; i < nb; i += 64) { sw += partials[i].x; sb += partials[i].y; }
  sw = wave_sum(sw);
  sb = wave_sum(sb);
  if (threadIdx.x == 0) {
    if (dw) *dw += sw;
    if (db) *db += sb;
  }
}

// Test hook: materialise the dropout keep-mask the kernels derive from (seed, offset + element index).
__global__ void keep_mask_kernel(uint8_t* out, size_t n, uint32_t key, uint32_t thr, const uint32_t* salt) {
  key = bb_salted(key, salt);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    out[i] = (uint8_t)bb_keep(key, (uint32_t)i, thr);
}

// =============================================================================================
// C ABI
// =============================================================================================
BEVBERT_API int bevbert_graph_bias_fwd(const float* dists, const float* w, const float* b, float* out, int64_t n,
                                       hipStream_t stream) {
  BB_REQUIRE(n >= 0 && n < 2147483647 && w != nullptr && b != nullptr, "graph_bias_fwd: bad arguments");
  if (n == 0) return BB_OK;
  int nb = (int)((n + 255) / 256);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(graph_bias_fwd_kernel, dim3(nb), dim3(256), 0, stream, dists, w, b, out, (int)n);
  BB_CHECK_LAUNCH("graph_bias_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_graph_bias_bwd(const float* dbias, const float* dists, int layers, int B, int nh, int G, float* dw,
                                       float* db, float* workspace, hipStream_t stream) {
  BB_REQUIRE(layers > 0 && B > 0 && nh > 0 && G > 0 && workspace != nullptr, "graph_bias_bwd: empty problem or no workspace");
  const int64_t per_layer = (int64_t)B * nh * G * G, n = per_layer * layers;
  BB_REQUIRE(n < 2147483647, "graph_bias_bwd: %lld elements do not fit 31 bits", (long long)n);
  int nb = (int)((n + 4095) / 4096);
  if (nb > 512) nb = 512;                                 // workspace: 2 * 512 floats
  hipLaunchKernelGGL(graph_bias_bwd_kernel, dim3(nb), dim3(256), 0, stream, dbias, dists, (uint32_t)n, (uint32_t)(G * G),
                     (uint32_t)per_layer, (uint32_t)(nh * G * G), (uint32_t)(G * G), reinterpret_cast<float2*>(workspace));
  BB_CHECK_LAUNCH("graph_bias_bwd");
  hipLaunchKernelGGL(graph_bias_finalize_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const float2*>(workspace), nb, dw, db);
  BB_CHECK_LAUNCH("graph_bias_bwd finalize");
  return BB_OK;
}

BEVBERT_API int bevbert_dropout_add(const void* x, const void* residual, void* y, int64_t n, int in_dtype,
                                    int out_dtype, float drop_p, uint64_t seed, uint64_t offset, hipStream_t stream) {
  BB_REQUIRE(n % 4 == 0 && n < ((int64_t)1 << 32), "dropout_add: n=%ld must be a multiple of 4 below 2^32", (long)n);
  BB_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "dropout_add: p=%f out of range", drop_p);
  if (n == 0) return BB_OK;
  size_t nb = ((size_t)n / 4 + 255) / 256;
  if (nb > 8192) nb = 8192;
  const float ks = 1.0f / (1.0f - drop_p);
  const uint32_t thr = bb_drop_threshold(drop_p), key = bb_site_key(seed, offset);
#define GO(TI, TO)                                                                                                   \
  hipLaunchKernelGGL((dropout_add_kernel<TI, TO>), dim3(nb), dim3(256), 0, stream, (const TI*)x, (const TO*)residual, \
                     (TO*)y, (size_t)n / 4, ks, thr, key, bb_step_salt())
  if (in_dtype == BB_F32 && out_dtype == BB_F32) GO(float, float);
  else if (in_dtype == BB_F32 && out_dtype == BB_BF16) GO(float, bf16_raw);
  else if (in_dtype == BB_BF16 && out_dtype == BB_BF16) GO(bf16_raw, bf16_raw);
  else if (in_dtype == BB_F16 && out_dtype == BB_F16) GO(_Float16, _Float16);
  else if (in_dtype == BB_F32 && out_dtype == BB_F16) GO(float, _Float16);
  else {
    bb_set_error("dropout_add: dtype pair %d -> %d unsupported", in_dtype, out_dtype);
    return BB_EUNSUPPORTED;
  }
#undef GO
  BB_CHECK_LAUNCH("dropout_add");
  return BB_OK;
}

BEVBERT_API int bevbert_dropout_keep_mask(uint8_t* out, int64_t n, float drop_p, uint64_t seed, uint64_t offset,
                                          hipStream_t stream) {
  if (n <= 0) return BB_OK;
  size_t nb = ((size_t)n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(keep_mask_kernel, dim3(nb), dim3(256), 0, stream, out, (size_t)n, bb_site_key(seed, offset),
                     bb_drop_threshold(drop_p), bb_step_salt());
  BB_CHECK_LAUNCH("dropout_keep_mask");
  return BB_OK;
}
