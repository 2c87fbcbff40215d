// Row kernels of the CLIP vision transformer (clip_vit.py): the image encoder of the continuous-environment agent's
// panorama views, forward only.
//
// Reference call sites replaced:
//   CLIPEncoderB16.rgb_transform + conv1's im2col   bevbert_ce/vlnce_baselines/models/encoders/resnet_encoders.py:299-312
//   VisionTransformer.forward                      encoders/clip/model.py:219-237 (token assembly, ln_pre, ln_post)
//   ResidualAttentionBlock.forward, QuickGELU      encoders/clip/model.py:162-188
//   grid_pool_depth = AdaptiveAvgPool2d((14, 14))  models/Policy_ViewSelection_BEV.py:127,190
//
// Layout as in layernorm.hip: activations are (rows, H) row-major with H % 256 == 0 and H <= 1024; one 64-lane wave owns one
// row and keeps it in registers (H / 64 values per lane as float4s).  The residual stream z32 is fp32 whatever the compute
// dtype T of the GEMM operands; statistics are fp32, and every LayerNorm here is ln_row_stats + ln_norm4 (common.h), the
// row body of ln_fwd_kernel.  No atomics, plain vector stores, one launch per entry.
#include <math.h>

#include "common.h"

// =============================================================================================
// patchify: uint8 (n_src, R, R, 3) -> patch rows (N * g * g, 3 * P * P), column (c, ky, kx): conv1.weight.view(width, -1)
// is then the GEMM operand.  One wave per patch; a lane takes four neighbouring pixels of one patch line (12 bytes, three
// aligned words) and stores four values per channel.  Arithmetic of ConvertImageDtype + Normalize as torch executes it on
// fp32 tensors: float(u8) / 255, then (x - mean) / std, every operation rounded to nearest on its own.
// =============================================================================================
struct VitNorm { float mean[3], std[3]; };

template <typename T, int P>
__global__ __launch_bounds__(256) void vit_patchify_kernel(const uint8_t* __restrict__ img, const int* __restrict__ map,
                                                           T* __restrict__ out, int N, int n_src, int R, VitNorm nm) {
  const int g = R / P;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)N * g * g) return;
  const int n = (int)(row / (g * g)), cell = (int)(row % (g * g));
  const int py = cell / g, px = cell % g;
  const int src = map ? map[n] : n;
  const bool ok = (unsigned)src < (unsigned)n_src;                  // a view index outside the input: a row of zeros
  const uint8_t* base = img + (size_t)(ok ? src : 0) * R * R * 3;
  T* orow = out + (size_t)row * (3 * P * P);
  for (int it = lane; it < P * P / 4; it += 64) {
    const int ky = it / (P / 4), kx = (it % (P / 4)) * 4;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(base + ((size_t)(py * P + ky) * R + px * P + kx) * 3);
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
    // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    const uint32_t u[3][4] = {{w0 & 255u, w0 >> 24, (w1 >> 16) & 255u, (w2 >> 8) & 255u},
                              {(w0 >> 8) & 255u, w1 & 255u, w1 >> 24, (w2 >> 16) & 255u},
                              {(w0 >> 16) & 255u, (w1 >> 8) & 255u, w2 & 255u, w2 >> 24}};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        v[k] = ok ? __fdiv_rn(__fsub_rn(__fdiv_rn((float)u[c][k], 255.0f), nm.mean[c]), nm.std[c]) : 0.f;
      st4<T>(orow + c * P * P + ky * P + kx, make_float4(v[0], v[1], v[2], v[3]));
    }
  }
}

// =============================================================================================
// embed_prenorm: token row t of image n is class_embedding + pos[0] (t = 0) or conv_out[n, t - 1] + pos[t]; z32 = ln_pre
// of it (the start of the residual stream), y = ln_1 of block 0 on z32.  The row stays in registers between the two.
// =============================================================================================
template <typename T, int NV>
__global__ __launch_bounds__(256) void vit_embed_prenorm_kernel(const T* __restrict__ conv, const float* __restrict__ cls,
                                                                const float* __restrict__ pos, const float* __restrict__ g_pre,
                                                                const float* __restrict__ b_pre, const float* __restrict__ g1,
                                                                const float* __restrict__ b1, float* __restrict__ z32,
                                                                T* __restrict__ y, int rows, int L, float eps) {
  constexpr int H = NV * 256;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int n = row / L, t = row % L;
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    const float4 a = t == 0 ? *reinterpret_cast<const float4*>(cls + col)
                            : ld4<T>(conv + ((size_t)n * (L - 1) + (t - 1)) * H + col);
    const float4 p = *reinterpret_cast<const float4*>(pos + (size_t)t * H + col);
    v[i] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
  }
  float mean, rstd;
  ln_row_stats<NV>(v, eps, mean, rstd);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    v[i] = ln_norm4(v[i], mean, rstd, g_pre, b_pre, col);
    st4<float>(z32 + (size_t)row * H + col, v[i]);
  }
  ln_row_stats<NV>(v, eps, mean, rstd);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    st4<T>(y + (size_t)row * H + col, ln_norm4(v[i], mean, rstd, g1, b1, col));
  }
}

// =============================================================================================
// bias_residual_prenorm: z = z32 + (x + bias).
//   FINAL = false: z32 <- z in place, y = LayerNorm(z) (the LayerNorm that opens the next sub-layer).
//   FINAL = true (after the last block): token rows t > 0 go to x_patch (N, L - 1, H) fp32 as they are; the class row
//   t = 0 goes through LayerNorm (ln_post) to cls_out (N, H).  z32 is not written back: nothing reads it afterwards.
// =============================================================================================
template <typename T, int NV, bool FINAL>
__global__ __launch_bounds__(256) void vit_bias_residual_prenorm_kernel(float* __restrict__ z32, const T* __restrict__ x,
                                                                        const float* __restrict__ bias,
                                                                        const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta, T* __restrict__ y,
                                                                        float* __restrict__ x_patch, int rows, int L,
                                                                        float eps) {
  constexpr int H = NV * 256;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    const float4 a = ld4<T>(x + (size_t)row * H + col);
    const float4 bb = *reinterpret_cast<const float4*>(bias + col);
    const float4 z = *reinterpret_cast<const float4*>(z32 + (size_t)row * H + col);
    v[i] = make_float4(z.x + (a.x + bb.x), z.y + (a.y + bb.y), z.z + (a.z + bb.z), z.w + (a.w + bb.w));
  }
  if (FINAL) {
    const int n = row / L, t = row % L;
    if (t != 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i)
        st4<float>(x_patch + ((size_t)n * (L - 1) + (t - 1)) * H + (i * 64 + lane) * 4, v[i]);
      return;
    }
    float mean, rstd;
    ln_row_stats<NV>(v, eps, mean, rstd);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int col = (i * 64 + lane) * 4;
      st4<T>(y + (size_t)n * H + col, ln_norm4(v[i], mean, rstd, gamma, beta, col));
    }
  } else {
    float mean, rstd;
    ln_row_stats<NV>(v, eps, mean, rstd);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int col = (i * 64 + lane) * 4;
      st4<float>(z32 + (size_t)row * H + col, v[i]);
      st4<T>(y + (size_t)row * H + col, ln_norm4(v[i], mean, rstd, gamma, beta, col));
    }
  }
}

// =============================================================================================
// bias_quickgelu: t = x + bias, y = t * sigmoid(1.702 t) = t / (1 + exp(-1.702 t)).  The exponential overflows to +inf
// only on the side where the quotient goes to (-)0, so the result is finite for every finite t.  Grid as bias_gelu_fwd:
// (row groups, column slices of 1024), a thread owns 4 columns and keeps 8 rows of loads in flight.
// =============================================================================================
template <typename T> __device__ __forceinline__ float quickgelu_of(float t);
template <> __device__ __forceinline__ float quickgelu_of<float>(float t) { return t / (1.0f + expf(-1.702f * t)); }
// bf16 results: the hardware exponential and reciprocal (2 ulp each in fp32, far below the bf16 rounding of the result)
template <> __device__ __forceinline__ float quickgelu_of<bf16_raw>(float t) {
  return t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t * -2.45546696148071f));   // 1.702 * log2(e)
}
// fp16 results take the same form.  The two hardware functions are good to 1 ulp of fp32 each and the product adds one
// rounding: a relative error of about 2^-22 wherever the sigmoid is not negligible, a thousand times below the 2^-12 (half
// an ulp) of the fp16 rounding that follows; the rounded argument of the exponential moves the result by |1.702 t| 2^-24
// relative to the exponential, which only counts where the quotient is already tiny (t < 0) or the exponential is (t > 0).
// t + bias is formed in fp32, so a result beyond 65504 becomes inf in the store's conversion, as IEEE fp16 does.
template <> __device__ __forceinline__ float quickgelu_of<_Float16>(float t) { return quickgelu_of<bf16_raw>(t); }
template <typename T> __device__ __forceinline__ float4 quickgelu4_of(float4 a, float4 b) {
  return make_float4(quickgelu_of<T>(a.x + b.x), quickgelu_of<T>(a.y + b.y), quickgelu_of<T>(a.z + b.z),
                     quickgelu_of<T>(a.w + b.w));
}

template <typename T>
__global__ __launch_bounds__(256) void vit_bias_quickgelu_kernel(const T* __restrict__ x, const float* __restrict__ bias,
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
    for (int k = 0; k < R; ++k) st4<T>(y + (size_t)(r + k) * C + c0, quickgelu4_of<T>(a[k], b));
  }
  for (; r < rows; ++r) st4<T>(y + (size_t)r * C + c0, quickgelu4_of<T>(ld4<T>(x + (size_t)r * C + c0), b));
}

// =============================================================================================
// depth_grid_pool: AdaptiveAvgPool2d((G, G)) of (n_src, Hd, Wd) fp32; cell i covers [floor(i Hd / G), ceil((i + 1) Hd / G)).
// One wave per output cell: the lanes stride over the window, one wave reduction, one store.
// =============================================================================================
__global__ __launch_bounds__(256) void vit_depth_grid_pool_kernel(const float* __restrict__ depth, const int* __restrict__ map,
                                                                  float* __restrict__ out, int N, int n_src, int Hd, int Wd,
                                                                  int G) {
  const int lane = threadIdx.x & 63;
  const int64_t cell = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= (int64_t)N * G * G) return;
  const int n = (int)(cell / (G * G)), i = (int)(cell % (G * G)) / G, j = (int)(cell % G);
  const int src = map ? map[n] : n;
  float s = 0.f;
  const int h0 = i * Hd / G, h1 = ((i + 1) * Hd + G - 1) / G, w0 = j * Wd / G, w1 = ((j + 1) * Wd + G - 1) / G;
  const int ww = w1 - w0, cnt = (h1 - h0) * ww;
  if ((unsigned)src < (unsigned)n_src) {
    const float* p = depth + (size_t)src * Hd * Wd;
    for (int e = lane; e < cnt; e += 64) s += p[(size_t)(h0 + e / ww) * Wd + w0 + e % ww];
  }
  s = wave_sum(s);
  if (lane == 0) out[cell] = s / (float)cnt;
}

// =============================================================================================
// C ABI
// =============================================================================================
static int vit_width_unsupported(const char* name, int H) {
  bb_set_error("%s: H=%d unsupported (need H in {256,512,768,1024})", name, H);
  return BB_EUNSUPPORTED;
}

BEVBERT_API int bevbert_vit_patchify(const uint8_t* images, const int* view_map, void* out, int N, int n_src, int R, int P,
                                     const float* mean_std, int dtype, hipStream_t stream) {
  BB_REQUIRE(N >= 0 && n_src > 0 && (P == 16 || P == 32) && R >= P && R % P == 0, "vit_patchify: N=%d n_src=%d R=%d P=%d", N,
             n_src, R, P);
  BB_REQUIRE(((uintptr_t)images % 4) == 0 && ((uintptr_t)out % 16) == 0, "vit_patchify: unaligned images / out");
  BB_REQUIRE((int64_t)N * (R / P) * (R / P) < (int64_t)1 << 31, "vit_patchify: too many patch rows");
  if (N == 0) return BB_OK;
  VitNorm nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = mean_std[c]; nm.std[c] = mean_std[3 + c]; }
  const int64_t rows = (int64_t)N * (R / P) * (R / P);
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool type_ok = bb_with_type_of<float, bf16_raw, _Float16>(dtype, [&](auto t) {
    using T = decltype(t);
    bb_with_int<16, 32>(P, [&](auto p) {
      hipLaunchKernelGGL((vit_patchify_kernel<T, decltype(p)::value>), grid, dim3(256), 0, stream, images, view_map, (T*)out, N,
                         n_src, R, nm);
    });
  });
  if (!type_ok) return bb_dtype_unsupported("vit_patchify", dtype);
  BB_CHECK_LAUNCH("vit_patchify");
  return BB_OK;
}

BEVBERT_API int bevbert_vit_embed_prenorm(const void* conv_out, const float* class_embedding, const float* pos,
                                          const float* gamma_pre, const float* beta_pre, const float* gamma1,
                                          const float* beta1, float* z32, void* y, int N, int L, int H, float eps, int dtype,
                                          hipStream_t stream) {
  BB_REQUIRE(N >= 0 && L >= 2 && H % 256 == 0 && (int64_t)N * L < (int64_t)1 << 31, "vit_embed_prenorm: N=%d L=%d H=%d", N, L, H);
  if (N == 0) return BB_OK;
  const int rows = N * L;
  const dim3 grid((rows + 3) / 4);
  bool width_ok = false;
  const bool type_ok = bb_with_type_of<float, bf16_raw, _Float16>(dtype, [&](auto t) {
    using T = decltype(t);
    width_ok = bb_with_width<1, 2, 3, 4>(H, [&](auto nv) {
      hipLaunchKernelGGL((vit_embed_prenorm_kernel<T, decltype(nv)::value>), grid, dim3(256), 0, stream, (const T*)conv_out,
                         class_embedding, pos, gamma_pre, beta_pre, gamma1, beta1, z32, (T*)y, rows, L, eps);
    });
  });
  if (!type_ok) return bb_dtype_unsupported("vit_embed_prenorm", dtype);
  if (!width_ok) return vit_width_unsupported("vit_embed_prenorm", H);
  BB_CHECK_LAUNCH("vit_embed_prenorm");
  return BB_OK;
}

BEVBERT_API int bevbert_vit_bias_residual_prenorm(float* z32, const void* x, const float* bias, const float* gamma,
                                                  const float* beta, void* y, float* x_patch, int rows, int L, int H,
                                                  float eps, int final_form, int dtype, hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && H % 256 == 0, "vit_bias_residual_prenorm: rows=%d H=%d", rows, H);
  BB_REQUIRE(!final_form || (x_patch != nullptr && L >= 2 && rows % L == 0),
             "vit_bias_residual_prenorm: the final form needs x_patch and rows = N * L (rows=%d L=%d)", rows, L);
  if (rows == 0) return BB_OK;
  const dim3 grid((rows + 3) / 4);
  bool width_ok = false;
  const bool type_ok = bb_with_type_of<float, bf16_raw, _Float16>(dtype, [&](auto t) {
    using T = decltype(t);
    width_ok = bb_with_width<1, 2, 3, 4>(H, [&](auto nv) {
      bb_with_bool(final_form != 0, [&](auto fin) {
        hipLaunchKernelGGL((vit_bias_residual_prenorm_kernel<T, decltype(nv)::value, decltype(fin)::value>), grid, dim3(256), 0,
                           stream, z32, (const T*)x, bias, gamma, beta, (T*)y, x_patch, rows, L, eps);
      });
    });
  });
  if (!type_ok) return bb_dtype_unsupported("vit_bias_residual_prenorm", dtype);
  if (!width_ok) return vit_width_unsupported("vit_bias_residual_prenorm", H);
  BB_CHECK_LAUNCH("vit_bias_residual_prenorm");
  return BB_OK;
}

BEVBERT_API int bevbert_vit_bias_quickgelu(const void* x, const float* bias, void* y, int rows, int C, int dtype,
                                           hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && C > 0 && C % 4 == 0, "vit_bias_quickgelu: rows=%d C=%d (C must be a multiple of 4)", rows, C);
  if (rows == 0) return BB_OK;
  const dim3 grid(elementwise_row_groups(rows), (C + 1023) / 1024);
  const bool type_ok = bb_with_type_of<float, bf16_raw, _Float16>(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(vit_bias_quickgelu_kernel<T>, grid, dim3(256), 0, stream, (const T*)x, bias, (T*)y, rows, C);
  });
  if (!type_ok) return bb_dtype_unsupported("vit_bias_quickgelu", dtype);
  BB_CHECK_LAUNCH("vit_bias_quickgelu");
  return BB_OK;
}

BEVBERT_API int bevbert_depth_grid_pool(const float* depth, const int* view_map, float* out, int N, int n_src, int Hd, int Wd,
                                        int G, hipStream_t stream) {
  BB_REQUIRE(N >= 0 && n_src > 0 && G > 0 && Hd >= 1 && Wd >= 1 && Hd <= 16384 && Wd <= 16384,
             "depth_grid_pool: N=%d n_src=%d Hd=%d Wd=%d G=%d", N, n_src, Hd, Wd, G);
  BB_REQUIRE((int64_t)N * G * G < (int64_t)1 << 31 && G <= 1024, "depth_grid_pool: too many cells");
  if (N == 0) return BB_OK;
  const int64_t cells = (int64_t)N * G * G;
  hipLaunchKernelGGL(vit_depth_grid_pool_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, stream, depth, view_map, out,
                     N, n_src, Hd, Wd, G);
  BB_CHECK_LAUNCH("depth_grid_pool");
  return BB_OK;
}
