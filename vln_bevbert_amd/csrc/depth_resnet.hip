// Row kernels of the depth ResNet encoder (depth_resnet.py): the GroupNorm ResNet-50 that turns the continuous-environment
// agent's depth views into the (128, 4, 4) embeddings the waypoint predictor reads, forward only.
//
// Reference call sites replaced:
//   VlnResnetDepthEncoder.forward                   bevbert_ce/vlnce_baselines/models/encoders/resnet_encoders.py:76-86
//   its call in the policy                          models/Policy_ViewSelection_BEV.py:189
// (the network itself is habitat-lab's ResNetEncoder, restated in DESIGN.md section 7b).
//
// Activations are NHWC, so a 1x1 convolution is a row-major GEMM on them as they are; the 3x3 and the strided 1x1
// convolutions read rows gathered here (dr_gather_rows_kernel) and every GEMM runs in the library (ops.linear).  What is
// left between two GEMMs is GroupNorm: statistics over (HW, C / G) per image and group, then one elementwise pass that
// also adds the shortcut, applies ReLU and, after the stem, takes the 3x3 max pool.  Statistics are fp32, two-pass inside a
// block (the values stay in registers between the passes) and combined over blocks with the pairwise update of Chan et
// al. in a fixed order: no atomics anywhere, two runs give the same bits, and a large mean does not cancel.
#include <math.h>

#include "common.h"

// =============================================================================================
// stem: avg_pool2d(2) of the depth image + Conv2d(1, 32, 7, stride 2, pad 3), direct, fp32.  One thread owns one output
// pixel and its 32 channels; the tap loop is uniform over the wave, so the weights (49, 32) are scalar loads.
// =============================================================================================
constexpr int DR_STEM_C = 32;

__global__ __launch_bounds__(256) void dr_stem_kernel(const float* __restrict__ depth, const int* __restrict__ map,
                                                      const float* __restrict__ w, float* __restrict__ out, int N, int n_src,
                                                      int H, int W, int Ho, int Wo) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)N * Ho * Wo) return;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), n = (int)(p / ((int64_t)Wo * Ho));
  const int src = map ? map[n] : n;
  const bool img_ok = (unsigned)src < (unsigned)n_src;              // a view index outside the input: zeros
  const float* base = depth + (size_t)(img_ok ? src : 0) * H * W;
  const int Hp = H >> 1, Wp = W >> 1;
  float acc[DR_STEM_C];
#pragma unroll
  for (int c = 0; c < DR_STEM_C; ++c) acc[c] = 0.f;
  for (int ky = 0; ky < 7; ++ky) {
    const int py = oy * 2 - 3 + ky;
    const bool y_ok = img_ok && py >= 0 && py < Hp;
    const int pyc = py < 0 ? 0 : (py >= Hp ? Hp - 1 : py);
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const int px = ox * 2 - 3 + kx;
      const bool ok = y_ok && px >= 0 && px < Wp;
      const int pxc = px < 0 ? 0 : (px >= Wp ? Wp - 1 : px);
      const float2 a = *reinterpret_cast<const float2*>(base + (size_t)(2 * pyc) * W + 2 * pxc);
      const float2 b = *reinterpret_cast<const float2*>(base + (size_t)(2 * pyc + 1) * W + 2 * pxc);
      const float v = ok ? ((a.x + a.y) + (b.x + b.y)) * 0.25f : 0.f;
      const float* wt = w + (ky * 7 + kx) * DR_STEM_C;
#pragma unroll
      for (int c = 0; c < DR_STEM_C; ++c) acc[c] = fmaf(v, wt[c], acc[c]);
    }
  }
  float* o = out + (size_t)p * DR_STEM_C;
#pragma unroll
  for (int c = 0; c < DR_STEM_C; c += 4) st4<float>(o + c, make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]));
}

// =============================================================================================
// GroupNorm statistics.  x is (N, HW, C); group g of image n holds the HW * (C / G) values of channels [g C / G, (g + 1) C / G).
// A block owns DR_CHUNK = 8192 values of one image: 8 steps of 256 float4s, rows whole (C / 4 divides 256), all of them kept
// in registers.  Pass 1 sums them per group, pass 2 sums the squared distances from the block's own group mean.  The
// per-thread sums (two per thread: channels c, c + 1 and c + 2, c + 3, so that C / G = 2 works) are reduced through LDS by 16
// helper lanes per group in a fixed order.  One chunk per image: the block writes mean and rstd itself; otherwise it writes
// (mean, M2) of its chunk and dr_gn_combine_kernel merges the chunks in ascending order.
// =============================================================================================
constexpr int DR_CHUNK = 8192;
constexpr int DR_MAX_G = 16;

// Sum of the block's (a, b) pairs per group; every thread gets the totals of the two groups its pairs belong to.
__device__ __forceinline__ void dr_group_sums(float a, float b, int vpr, int G, int ppg, int ga, int gb, float* s_part,
                                              float* s_tot, float& ta, float& tb) {
  const int t = threadIdx.x;
  s_part[2 * t] = a;
  s_part[2 * t + 1] = b;
  __syncthreads();
  float acc = 0.f;
  if (t < 16 * G) {
    const int g = t >> 4, j = t & 15, per = 512 / G;                 // entries of one group: (256 / vpr) rows x ppg pairs
    for (int e = j; e < per; e += 16) acc += s_part[(e / ppg) * vpr * 2 + g * ppg + e % ppg];
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (t < 16 * G && (t & 15) == 0) s_tot[t >> 4] = acc;
  __syncthreads();
  ta = s_tot[ga];
  tb = s_tot[gb];
}

template <typename T>
__global__ __launch_bounds__(256) void dr_gn_partial_kernel(const T* __restrict__ x, float* __restrict__ partial,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out, int HW,
                                                            int C, int G, int chunks, float eps) {
  __shared__ float s_part[512];
  __shared__ float s_tot[DR_MAX_G];
  const int t = threadIdx.x, chunk = blockIdx.x, n = blockIdx.y;
  const int vpr = C >> 2, rps = 256 / vpr;                            // float4s per row, rows per step
  const int v = t % vpr, ro = t / vpr;
  const int r0 = chunk * 8 * rps;
  const int cpg = C / G, ppg = cpg >> 1;
  const int ga = (4 * v) / cpg, gb = (4 * v + 2) / cpg;
  const T* xi = x + (size_t)n * HW * C;
  float4 val[8];
  bool ok[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = r0 + i * rps + ro;
    ok[i] = row < HW;
    val[i] = ok[i] ? ld4<T>(xi + (size_t)row * C + 4 * v) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int rows = HW - r0 < 8 * rps ? HW - r0 : 8 * rps;
  const float inv_cnt = 1.0f / ((float)rows * (float)cpg);
  float a = 0.f, b = 0.f, ma, mb;
#pragma unroll
  for (int i = 0; i < 8; ++i) { a += val[i].x + val[i].y; b += val[i].z + val[i].w; }
  dr_group_sums(a, b, vpr, G, ppg, ga, gb, s_part, s_tot, ma, mb);
  ma *= inv_cnt;
  mb *= inv_cnt;
  a = 0.f, b = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (ok[i]) {
      const float dx = val[i].x - ma, dy = val[i].y - ma, dz = val[i].z - mb, dw = val[i].w - mb;
      a += dx * dx + dy * dy;
      b += dz * dz + dw * dw;
    }
  }
  float qa, qb;
  dr_group_sums(a, b, vpr, G, ppg, ga, gb, s_part, s_tot, qa, qb);
  // the first thread whose first pair lies in group g writes it (ro = 0, the group's first float4 or, for C / G = 2, pair)
  if (ro == 0 && (4 * v) % cpg == 0) {
    if (chunks == 1) { mean_out[n * G + ga] = ma; rstd_out[n * G + ga] = rsqrtf(qa * inv_cnt + eps); }
    else { float* p = partial + ((size_t)(n * chunks + chunk) * G + ga) * 2; p[0] = ma; p[1] = qa; }
  }
  if (ro == 0 && cpg == 2) {
    if (chunks == 1) { mean_out[n * G + gb] = mb; rstd_out[n * G + gb] = rsqrtf(qb * inv_cnt + eps); }
    else { float* p = partial + ((size_t)(n * chunks + chunk) * G + gb) * 2; p[0] = mb; p[1] = qb; }
  }
}

// (mean, M2) of the chunks of one (image, group), merged in ascending chunk order (Chan, Golub, LeVeque); one thread each.
__global__ __launch_bounds__(256) void dr_gn_combine_kernel(const float* __restrict__ partial, float* __restrict__ mean_out,
                                                            float* __restrict__ rstd_out, int NG, int G, int HW, int C,
                                                            int chunks, float eps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= NG) return;
  const int n = i / G, g = i % G;
  const int cpg = C / G, rpc = 8 * (256 / (C >> 2));
  double cnt = 0.0, mean = 0.0, m2 = 0.0;
  for (int k = 0; k < chunks; ++k) {
    const float* p = partial + ((size_t)(n * chunks + k) * G + g) * 2;
    const int rows = HW - k * rpc < rpc ? HW - k * rpc : rpc;
    const double cb = (double)rows * cpg, delta = (double)p[0] - mean, tot = cnt + cb;
    mean += delta * (cb / tot);
    m2 += (double)p[1] + delta * delta * (cnt * cb / tot);
    cnt = tot;
  }
  mean_out[i] = (float)mean;
  rstd_out[i] = (float)(1.0 / sqrt(m2 / cnt + (double)eps));
}

// =============================================================================================
// GroupNorm apply, elementwise over (N, HW, C), a thread per float4 of channels:
//   MODE 0  y = relu(gn(x))
//   MODE 1  y = relu(gn(x) + r)                       r: the block's input (N, HW, C) in T
//   MODE 2  y = relu(gn(x) + gn2(r))                  r: the raw downsample branch with its own statistics and affine
//   MODE 3  y = relu(gn(x)) written as NCHW           the last layer
// gn(x) = (x - mean[n, g]) * rstd[n, g] * gamma[c] + beta[c].
// =============================================================================================
struct DrNorm { float4 m, r, g, b; };
__device__ __forceinline__ DrNorm dr_norm_of(const float* __restrict__ mean, const float* __restrict__ rstd,
                                             const float* __restrict__ gamma, const float* __restrict__ beta, int n, int G,
                                             int cpg, int c) {
  const int g0 = n * G + c / cpg, g1 = n * G + (c + 2) / cpg;
  DrNorm d;
  d.m = make_float4(mean[g0], mean[g0], mean[g1], mean[g1]);
  d.r = make_float4(rstd[g0], rstd[g0], rstd[g1], rstd[g1]);
  d.g = *reinterpret_cast<const float4*>(gamma + c);
  d.b = *reinterpret_cast<const float4*>(beta + c);
  return d;
}
__device__ __forceinline__ float4 dr_apply(const DrNorm& d, float4 v) {
  return make_float4((v.x - d.m.x) * d.r.x * d.g.x + d.b.x, (v.y - d.m.y) * d.r.y * d.g.y + d.b.y,
                     (v.z - d.m.z) * d.r.z * d.g.z + d.b.z, (v.w - d.m.w) * d.r.w * d.g.w + d.b.w);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void dr_gn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const T* __restrict__ r,
                                                          const float* __restrict__ mean2, const float* __restrict__ rstd2,
                                                          const float* __restrict__ gamma2, const float* __restrict__ beta2,
                                                          T* __restrict__ y, int64_t total, int HW, int C, int G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int vpr = C >> 2, cpg = C / G;
  const int c = (int)(i % vpr) * 4;
  const int64_t row = i / vpr;
  const int n = (int)(row / HW);
  float4 v = dr_apply(dr_norm_of(mean, rstd, gamma, beta, n, G, cpg, c), ld4<T>(x + i * 4));
  if (MODE == 1) add4(v, ld4<T>(r + i * 4));
  if (MODE == 2) add4(v, dr_apply(dr_norm_of(mean2, rstd2, gamma2, beta2, n, G, cpg, c), ld4<T>(r + i * 4)));
  v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
  if (MODE == 3) {
    T* o = y + ((size_t)n * C + c) * HW + (int)(row % HW);
    io<T>::st(o, v.x);
    io<T>::st(o + HW, v.y);
    io<T>::st(o + 2 * (size_t)HW, v.z);
    io<T>::st(o + 3 * (size_t)HW, v.w);
  } else {
    st4<T>(y + i * 4, v);
  }
}

// The stem's form: GroupNorm + ReLU + MaxPool2d(3, stride 2, pad 1) of the raw fp32 stem output (N, H, W, C) -> (N, Ho, Wo, C)
// in T.  The maximum is taken over the NORMALISED values (gamma may be negative); ReLU is monotone and comes last.
template <typename T>
__global__ __launch_bounds__(256) void dr_gn_relu_maxpool_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, T* __restrict__ y,
                                                                 int64_t total, int H, int W, int Ho, int Wo, int C, int G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int vpr = C >> 2, cpg = C / G;
  const int c = (int)(i % vpr) * 4;
  const int64_t pix = i / vpr;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), n = (int)(pix / ((int64_t)Wo * Ho));
  const DrNorm d = dr_norm_of(mean, rstd, gamma, beta, n, G, cpg, c);
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * 2 - 1 + ky;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * 2 - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const float4 v = dr_apply(d, *reinterpret_cast<const float4*>(x + (((size_t)n * H + iy) * W + ix) * C + c));
      m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
    }
  }
  st4<T>(y + i * 4, make_float4(fmaxf(m.x, 0.f), fmaxf(m.y, 0.f), fmaxf(m.z, 0.f), fmaxf(m.w, 0.f)));
}

// =============================================================================================
// Row gather of a K x K convolution with stride S and padding (K - 1) / 2 on NHWC: row (n, oy, ox) of the output is the
// K * K input pixels (ky, kx) around (oy S, ox S), C values each, zeros outside the image: column order (ky, kx, c).
// A copy of 16-byte pieces, whatever the element type (a pixel is Cv = C * sizeof(T) / 16 of them).
// =============================================================================================
__global__ __launch_bounds__(256) void dr_gather_rows_kernel(const uint4* __restrict__ x, uint4* __restrict__ out, int64_t total,
                                                             int H, int W, int Cv, int K, int S, int Ho, int Wo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cv = (int)(i % Cv);
  const int tap = (int)((i / Cv) % (K * K));
  const int64_t pix = i / ((int64_t)Cv * K * K);
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const int64_t n = pix / ((int64_t)Wo * Ho);
  const int pad = (K - 1) >> 1;
  const int iy = oy * S - pad + tap / K, ix = ox * S - pad + tap % K;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((n * H + iy) * W + ix) * Cv + cv];
  out[i] = v;
}

// =============================================================================================
// C ABI
// =============================================================================================
BEVBERT_API int bevbert_dr_stem(const float* depth, const int* view_map, const float* weight_t, float* out, int N, int n_src,
                                int H, int W, hipStream_t stream) {
  BB_REQUIRE(N >= 0 && n_src > 0 && H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0 && H <= 16384 && W <= 16384,
             "dr_stem: N=%d n_src=%d H=%d W=%d (H and W must be multiples of 4)", N, n_src, H, W);
  BB_REQUIRE(((uintptr_t)depth % 8) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_t % 4) == 0,
             "dr_stem: unaligned depth / out / weight");
  const int Ho = H / 4, Wo = W / 4;
  const int64_t pixels = (int64_t)N * Ho * Wo;
  BB_REQUIRE(pixels < (int64_t)1 << 31, "dr_stem: too many output pixels");
  if (N == 0) return BB_OK;
  hipLaunchKernelGGL(dr_stem_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, depth, view_map, weight_t, out,
                     N, n_src, H, W, Ho, Wo);
  BB_CHECK_LAUNCH("dr_stem");
  return BB_OK;
}

static bool dr_gn_shape_ok(int C, int G) {
  return C >= 4 && C <= 1024 && C % 4 == 0 && 256 % (C / 4) == 0 && G >= 1 && G <= DR_MAX_G && (G & (G - 1)) == 0 &&
         C % G == 0 && (C / G) % 2 == 0 && ((C / G) == 2 || (C / G) % 4 == 0);
}

// blocks per image: DR_CHUNK values each, rows whole (depth_resnet.py gn_chunks sizes the partial buffer with the same rule)
static int dr_gn_chunks(int HW, int C) {
  const int rpc = DR_CHUNK / C;
  return (HW + rpc - 1) / rpc;
}

BEVBERT_API int bevbert_dr_gn_stats(const void* x, float* partial, int64_t partial_floats, float* mean, float* rstd, int N,
                                    int HW, int C, int G, float eps, int dtype, hipStream_t stream) {
  BB_REQUIRE(N >= 0 && N <= 65535 && HW >= 1 && dr_gn_shape_ok(C, G), "dr_gn_stats: N=%d HW=%d C=%d G=%d unsupported", N, HW, C, G);
  BB_REQUIRE(((uintptr_t)x % 16) == 0, "dr_gn_stats: unaligned x");
  if (N == 0) return BB_OK;
  const int chunks = dr_gn_chunks(HW, C);
  BB_REQUIRE(chunks == 1 || (partial != nullptr && partial_floats >= (int64_t)N * chunks * G * 2),
             "dr_gn_stats: the partial buffer holds %lld floats, %lld needed", (long long)partial_floats,
             (long long)N * chunks * G * 2);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(dr_gn_partial_kernel<T>, dim3(chunks, N), dim3(256), 0, stream, (const T*)x, partial, mean, rstd, HW, C,
                       G, chunks, eps);
  });
  if (!type_ok) return bb_dtype_unsupported("dr_gn_stats", dtype);
  BB_CHECK_LAUNCH("dr_gn_stats");
  if (chunks > 1) {
    hipLaunchKernelGGL(dr_gn_combine_kernel, dim3((N * G + 255) / 256), dim3(256), 0, stream, partial, mean, rstd, N * G, G, HW,
                       C, chunks, eps);
    BB_CHECK_LAUNCH("dr_gn_stats (combine)");
  }
  return BB_OK;
}

BEVBERT_API int bevbert_dr_gn_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    const void* r, const float* mean2, const float* rstd2, const float* gamma2,
                                    const float* beta2, void* y, int N, int HW, int C, int G, int mode, int dtype,
                                    hipStream_t stream) {
  BB_REQUIRE(N >= 0 && HW >= 1 && dr_gn_shape_ok(C, G) && mode >= 0 && mode <= 3, "dr_gn_apply: N=%d HW=%d C=%d G=%d mode=%d", N,
             HW, C, G, mode);
  BB_REQUIRE(mode == 0 || mode == 3 || r != nullptr, "dr_gn_apply: mode %d needs the second tensor", mode);
  BB_REQUIRE(mode != 2 || (mean2 && rstd2 && gamma2 && beta2), "dr_gn_apply: mode 2 needs the second statistics and affine");
  BB_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 8) == 0 && ((uintptr_t)r % 8) == 0 && ((uintptr_t)gamma % 16) == 0 &&
             ((uintptr_t)beta % 16) == 0 && ((uintptr_t)gamma2 % 16) == 0 && ((uintptr_t)beta2 % 16) == 0,
             "dr_gn_apply: unaligned operand");
  if (N == 0) return BB_OK;
  const int64_t total = (int64_t)N * HW * (C / 4);
  BB_REQUIRE((total + 255) / 256 < (int64_t)1 << 31, "dr_gn_apply: too many elements");
  const dim3 grid((unsigned)((total + 255) / 256));
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    bb_with_int<0, 1, 2, 3>(mode, [&](auto m) {
      hipLaunchKernelGGL((dr_gn_apply_kernel<T, decltype(m)::value>), grid, dim3(256), 0, stream, (const T*)x, mean, rstd, gamma,
                         beta, (const T*)r, mean2, rstd2, gamma2, beta2, (T*)y, total, HW, C, G);
    });
  });
  if (!type_ok) return bb_dtype_unsupported("dr_gn_apply", dtype);
  BB_CHECK_LAUNCH("dr_gn_apply");
  return BB_OK;
}

BEVBERT_API int bevbert_dr_gn_relu_maxpool(const float* x, const float* mean, const float* rstd, const float* gamma,
                                           const float* beta, void* y, int N, int H, int W, int C, int G, int dtype,
                                           hipStream_t stream) {
  BB_REQUIRE(N >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && dr_gn_shape_ok(C, G),
             "dr_gn_relu_maxpool: N=%d H=%d W=%d C=%d G=%d", N, H, W, C, G);
  BB_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 8) == 0 && ((uintptr_t)gamma % 16) == 0 && ((uintptr_t)beta % 16) == 0,
             "dr_gn_relu_maxpool: unaligned operand");
  if (N == 0) return BB_OK;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int64_t total = (int64_t)N * Ho * Wo * (C / 4);
  BB_REQUIRE((total + 255) / 256 < (int64_t)1 << 31, "dr_gn_relu_maxpool: too many elements");
  const dim3 grid((unsigned)((total + 255) / 256));
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(dr_gn_relu_maxpool_kernel<T>, grid, dim3(256), 0, stream, x, mean, rstd, gamma, beta, (T*)y, total, H, W,
                       Ho, Wo, C, G);
  });
  if (!type_ok) return bb_dtype_unsupported("dr_gn_relu_maxpool", dtype);
  BB_CHECK_LAUNCH("dr_gn_relu_maxpool");
  return BB_OK;
}

BEVBERT_API int bevbert_dr_gather_rows(const void* x, void* out, int N, int H, int W, int C, int ksize, int stride, int dtype,
                                       hipStream_t stream) {
  BB_REQUIRE(N >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && C >= 1 && (ksize == 1 || ksize == 3) &&
             (stride == 1 || stride == 2), "dr_gather_rows: N=%d H=%d W=%d C=%d ksize=%d stride=%d", N, H, W, C, ksize, stride);
  int esize = 0;
  if (!bb_with_type(dtype, [&](auto t) { esize = (int)sizeof(t); })) return bb_dtype_unsupported("dr_gather_rows", dtype);
  BB_REQUIRE(((int64_t)C * esize) % 16 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0,
             "dr_gather_rows: a pixel must be a whole number of aligned 16-byte pieces (C=%d)", C);
  if (N == 0) return BB_OK;
  const int Cv = C * esize / 16;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;       // (H + 2 pad - K) / S + 1 with pad = (K - 1) / 2
  const int64_t total = (int64_t)N * Ho * Wo * ksize * ksize * Cv;
  BB_REQUIRE((total + 255) / 256 < (int64_t)1 << 31, "dr_gather_rows: too many elements");
  hipLaunchKernelGGL(dr_gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const uint4*)x,
                     (uint4*)out, total, H, W, Cv, ksize, stride, Ho, Wo);
  BB_CHECK_LAUNCH("dr_gather_rows");
  return BB_OK;
}
