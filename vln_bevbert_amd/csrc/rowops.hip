// HBM-bound row kernels: K3 bias+dropout+residual+LayerNorm (fwd/bwd), K4 bias+erf-GELU (fwd/bwd),
// K5 embedding-sum+LayerNorm, K6 weighted segment gather (gmap aggregation fwd and bwd), column sums,
// and the flat-arena optimiser kernels (K7 fused AdamW, grad-norm, clip coefficient).
//
// Reference call sites replaced:
//   BertSelfOutput / BertOutput            pretrain_src/model/vilmodel.py:143-154,182-193  (dense bias + dropout + add + LN)
//   BertIntermediate + gelu                vilmodel.py:31-37,168-180
//   BertEmbeddings                         vilmodel.py:48-77
//   _aggregate_gmap_features               vilmodel.py:632-666 (Python dict loops -> one CSR gather)
//   clip_grad_norm_ + AdamW.step           pretrain_src/train_r2r.py:295-306, pretrain_src/optim/adamw.py:53-112
//
// Layout: activations are (rows, H) row-major with H % 256 == 0; one 64-lane wave owns one row and keeps it in
// registers (H/64 values per lane as float4s), so each tensor is read once and written once; statistics are fp32.
#include <math.h>
#include <type_traits>

#include "common.h"

// =============================================================================================
// LayerNorm forward:  z = dropout(x + bias) + residual ;  y = (z - mean) * rstd * gamma + beta
// GATHER: x row = word[ids[row]] + pos[row % L] + type_row   (BertEmbeddings)
// =============================================================================================
// The input stage of one float4 chunk, shared by ln_fwd_kernel and ln_res32_fwd_kernel: bias, then the dropout mask (elem
// = the chunk's first element index in the tensor), then the residual chunk r, which the caller has loaded through its
// own storage type (has_res: there is one).
__device__ __forceinline__ float4 ln_fwd_input(float4 a, const float* __restrict__ bias, int col, float drop_p, uint32_t elem,
                                               uint32_t drop_key, uint32_t drop_thr, float keep_scale, bool has_res,
                                               const float4 r) {
  if (bias != nullptr) add4(a, *reinterpret_cast<const float4*>(bias + col));
  if (drop_p > 0.f) a = bb_drop4(a, elem, drop_key, drop_thr, keep_scale);
  if (has_res) add4(a, r);
  return a;
}

template <typename T, int NV, bool GATHER>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ bias,
                                                     const T* __restrict__ residual, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, T* __restrict__ y,
                                                     T* __restrict__ z_out, float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out, int rows, float eps, float drop_p,
                                                     uint32_t drop_thr, uint32_t drop_key,
                                                     const int64_t* __restrict__ ids, const T* __restrict__ word,
                                                     const T* __restrict__ pos, const T* __restrict__ type_row, int L,
                                                     const uint32_t* __restrict__ salt) {
  constexpr int H = NV * 256;
  if (drop_p > 0.f) drop_key = bb_salted(drop_key, salt);
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4 v[NV];
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    float4 a;
    if (GATHER) {
      const int64_t id = ids[row];
      a = ld4<T>(word + (size_t)id * H + col);
      const float4 p = ld4<T>(pos + (size_t)(row % L) * H + col);
      const float4 t = ld4<T>(type_row + col);
      a.x = (a.x + p.x) + t.x; a.y = (a.y + p.y) + t.y; a.z = (a.z + p.z) + t.z; a.w = (a.w + p.w) + t.w;
    } else {
      a = ld4<T>(x + (size_t)row * H + col);
    }
    const bool has_res = residual != nullptr;
    const float4 r = has_res ? ld4<T>(residual + (size_t)row * H + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    v[i] = ln_fwd_input(a, bias, col, drop_p, (uint32_t)row * H + col, drop_key, drop_thr, keep_scale, has_res, r);
  }
  // The text of ln_row_stats (common.h), on purpose not a call: inlined from the helper the compiler contracts the sum of
  // squares the other way round (which product of dx * dx + dy * dy goes into the fma), and rstd -- which the backward
  // kernels and every replayed graph rely on -- differs in the last bit on some rows.  Keep the texts equal.
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mean = wave_sum(s) * (1.0f / H);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
    q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / H) + eps);
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    if (z_out != nullptr) st4<T>(z_out + (size_t)row * H + col, v[i]);
    float4 o = ln_norm4(v[i], mean, rstd, gamma, beta, col);
    if (!GATHER) {   // post-normalisation terms (bevbert_layernorm_post_fwd): y = LN(..) + post1 + post2, in that order --
      // the GATHER-only pointers carry them, so the plain variant costs two null tests
      if (word != nullptr) add4(o, ld4<T>(word + (size_t)row * H + col));
      if (pos != nullptr) add4(o, ld4<T>(pos + (size_t)row * H + col));
    }
    st4<T>(y + (size_t)row * H + col, o);
  }
}

// =============================================================================================
// LayerNorm backward.  Given dy, the saved z, mean, rstd:
//   dz = rstd * (g*dy - mean_H(g*dy) - xhat * mean_H(g*dy*xhat))        -> d(residual)
//   dx = dz * keep/(1-p)                                                  -> d(dense output)   (== dz when p == 0)
//   per-column partial sums of dy*xhat (dgamma), dy (dbeta), dx (dbias) -> partials[block][3][H]
// Persistent-style grid: each wave strides over rows and keeps its column partials in registers.
// =============================================================================================
// The arithmetic of one float4 chunk of a row, shared by every LayerNorm backward kernel of this file (the plain one,
// the fp32-stream one and its load-ahead form): one place for what must stay bit-identical between them.
// First half: xhat of the chunk, its terms of the dgamma / dbeta column partials, d <- gamma * dy, the row sums' terms.
__device__ __forceinline__ void ln_bwd_chunk_reduce(float4& d, const float4 zz, float mu, float rs, const float4 g, float4& xh,
                                                    float4& ag, float4& ab, float& s1, float& s2) {
  xh = make_float4((zz.x - mu) * rs, (zz.y - mu) * rs, (zz.z - mu) * rs, (zz.w - mu) * rs);
  ag.x += d.x * xh.x; ag.y += d.y * xh.y; ag.z += d.z * xh.z; ag.w += d.w * xh.w;
  add4(ab, d);
  d.x *= g.x; d.y *= g.y; d.z *= g.z; d.w *= g.w;
  s1 += (d.x + d.y) + (d.z + d.w);
  s2 += (d.x * xh.x + d.y * xh.y) + (d.z * xh.z + d.w * xh.w);
}
// Second half, with s1 / s2 the row means: the chunk of dz; dx is dz through the forward's dropout mask (bb_drop4)
__device__ __forceinline__ float4 ln_bwd_chunk_dz(const float4 d, const float4 xh, float rs, float s1, float s2) {
  float4 o;
  o.x = rs * (d.x - s1 - xh.x * s2);
  o.y = rs * (d.y - s1 - xh.y * s2);
  o.z = rs * (d.z - s1 - xh.z * s2);
  o.w = rs * (d.w - s1 - xh.w * s2);
  return o;
}
// The end of these kernels: the four waves' column partials folded through LDS in wave order into partials[block][3][H]
template <int NV>
__device__ __forceinline__ void ln_bwd_store_partials(float4 (&s_red)[3][4][NV * 64], const float4 (&ag)[NV],
                                                      const float4 (&ab)[NV], const float4 (&ax)[NV],
                                                      float* __restrict__ partials, int lane, int wave) {
  constexpr int H = NV * 256;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    s_red[0][wave][i * 64 + lane] = ag[i];
    s_red[1][wave][i * 64 + lane] = ab[i];
    s_red[2][wave][i * 64 + lane] = ax[i];
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 3 * NV * 64; k += 256) {
    const int which = k / (NV * 64), j = k % (NV * 64);
    float4 a = s_red[which][0][j];
#pragma unroll
    for (int w = 1; w < 4; ++w) add4(a, s_red[which][w][j]);
    *reinterpret_cast<float4*>(partials + ((size_t)blockIdx.x * 3 + which) * H + j * 4) = a;
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ z,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, T* __restrict__ dz_out,
                                                     T* __restrict__ dx_out, float* __restrict__ partials, int rows,
                                                     float drop_p, uint32_t drop_thr, uint32_t drop_key,
                                                     const uint32_t* __restrict__ salt, const T* __restrict__ dz_add) {
  constexpr int H = NV * 256;
  if (drop_p > 0.f) drop_key = bb_salted(drop_key, salt);
  __shared__ float4 s_red[3][4][NV * 64];  // [which][wave][lane-major float4]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  float4 ag[NV], ab[NV], ax[NV];
  float4 g[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    ag[i] = ab[i] = ax[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    g[i] = *reinterpret_cast<const float4*>(gamma + (i * 64 + lane) * 4);
  }
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const float mu = mean[row], rs = rstd[row];
    float4 d[NV], xh[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int col = (i * 64 + lane) * 4;
      d[i] = ld4<T>(dy + (size_t)row * H + col);
      const float4 zz = ld4<T>(z + (size_t)row * H + col);
      ln_bwd_chunk_reduce(d[i], zz, mu, rs, g[i], xh[i], ag[i], ab[i], s1, s2);
    }
    s1 = wave_sum(s1) * (1.0f / H);
    s2 = wave_sum(s2) * (1.0f / H);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int col = (i * 64 + lane) * 4;
      float4 o = ln_bwd_chunk_dz(d[i], xh[i], rs, s1, s2);
      // z has a second consumer (pre-norm residual stream): its gradient joins here
      if (dz_add != nullptr) add4(o, ld4<T>(dz_add + (size_t)row * H + col));
      if (dz_out != nullptr) st4<T>(dz_out + (size_t)row * H + col, o);
      if (drop_p > 0.f) o = bb_drop4(o, (uint32_t)row * H + col, drop_key, drop_thr, keep_scale);
      if (dx_out != nullptr) st4<T>(dx_out + (size_t)row * H + col, o);
      add4(ax[i], o);
    }
  }
  ln_bwd_store_partials<NV>(s_red, ag, ab, ax, partials, lane, wave);
}

// ---- helpers of the fp32-stream backward with the NEXT row's loads in flight (ln_res32_bwd_ahead_kernel) ----------
// A row's operands are held as they leave memory (16-bit types still packed): a conversion issued with the loads
// would wait for them.
template <typename T> struct raw4;
template <> struct raw4<float> {
  typedef float4 type;
  static __device__ __forceinline__ float4 ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ float4 f32(float4 v) { return v; }
};
template <> struct raw4<bf16_raw> {
  typedef uint2 type;
  static __device__ __forceinline__ uint2 ld(const bf16_raw* p) { return *reinterpret_cast<const uint2*>(p); }
  static __device__ __forceinline__ float4 f32(uint2 u) {      // as ld4<bf16_raw>
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
};
// apply(row, buffer) for row0, row0 + stride, ... < rows: two register buffers in turn, the next row's fill(buffer, row)
// issued before the current row's apply()
template <typename Row, typename F, typename A>
__device__ __forceinline__ void walk_rows_ahead(int row, int rows, int stride, F&& fill, A&& apply) {
  if (row >= rows) return;
  Row a, b;
  fill(a, row);
  for (;;) {
    int next = row + stride;
    if (next < rows) fill(b, next);
    apply(row, a);
    if (next >= rows) break;
    row = next;
    next = row + stride;
    if (next < rows) fill(a, next);
    apply(row, b);
    if (next >= rows) break;
    row = next;
  }
}

// =============================================================================================
// The same pair with an fp32 RESIDUAL STREAM around bf16 matrix operands (round 5; torch.autocast keeps LayerNorm outputs
// and residual sums in fp32 and only rounds what enters a GEMM: pretrain_src/train_r2r.py:256-258).
//   forward:  z = dropout(x + bias) + residual, x bf16 (a GEMM output), residual fp32 (the previous LayerNorm's fp32 output)
//             or bf16 (a stream that starts here); writes y16 = bf16(y) for the next GEMMs, y32 = y for the next residual
//             add, z in fp32 for the backward
//   backward: dy = dy16 (bf16: from the GEMMs that read y16) + dy32 (fp32: from the residual add that read y32), either
//             may be null; dz32 (fp32) continues the residual stream's gradient, dx16 = bf16(dz through the dropout mask)
//             feeds the dense layer's backward GEMMs; column partials as in ln_bwd_kernel
//   CHAIN:    the residual is the fp32 output of the PREVIOUS LayerNorm of the stream, which that launch did not write:
//             `residual` is its saved pre-norm sum z32 and the chunk is ln_norm4 of it with that launch's mean, rstd, gamma
//             and beta -- the producer's own expression on the producer's own fp32 operands, hence its bits.  The stream
//             then costs 12 B per element and launch (x, z_prev in; y16, z32 out) instead of 16.
// =============================================================================================
struct LnPrev { const float* mean; const float* rstd; const float* gamma; const float* beta; };   // CHAIN: of the producer

// (eight waves per SIMD, i.e. at most 64 VGPRs: what the plain forms take anyway, while the chained one at H = 768 would
// otherwise keep every chunk's operands in flight at once -- 66 VGPRs, seven waves; at H = 1 024 it would need 82 and
// spills under 64, so there it is left six waves)
template <typename TR, int NV, bool CHAIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CHAIN && NV == 4 ? 6 : 8, 8))) void ln_res32_fwd_kernel(const bf16_raw* __restrict__ x, const float* __restrict__ bias,
                                                           const TR* __restrict__ residual, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, bf16_raw* __restrict__ y16,
                                                           float* __restrict__ y32, float* __restrict__ z_out,
                                                           float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                           int rows, float eps, float drop_p, uint32_t drop_thr,
                                                           uint32_t drop_key, const uint32_t* __restrict__ salt,
                                                           const LnPrev prev) {
  static_assert(!CHAIN || std::is_same<TR, float>::value, "a chained residual is the producer's fp32 z");
  constexpr int H = NV * 256;
  if (drop_p > 0.f) drop_key = bb_salted(drop_key, salt);
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4 v[NV];
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  float mean_prev = 0.f, rstd_prev = 0.f;
  if (CHAIN) {
    mean_prev = prev.mean[row];
    rstd_prev = prev.rstd[row];
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    const float4 a = ld4<bf16_raw>(x + (size_t)row * H + col);
    const bool has_res = CHAIN || residual != nullptr;
    float4 r = has_res ? ld4<TR>(residual + (size_t)row * H + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (CHAIN) r = ln_norm4(r, mean_prev, rstd_prev, prev.gamma, prev.beta, col);
    v[i] = ln_fwd_input(a, bias, col, drop_p, (uint32_t)row * H + col, drop_key, drop_thr, keep_scale, has_res, r);
  }
  // ln_row_stats written out, for the reason given in ln_fwd_kernel
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mean = wave_sum(s) * (1.0f / H);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
    q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / H) + eps);
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    if (z_out != nullptr) st4<float>(z_out + (size_t)row * H + col, v[i]);
    const float4 o = ln_norm4(v[i], mean, rstd, gamma, beta, col);
    st4<bf16_raw>(y16 + (size_t)row * H + col, o);
    if (y32 != nullptr) st4<float>(y32 + (size_t)row * H + col, o);
  }
}

// One row of the backward, shared by ln_res32_bwd_kernel and its load-ahead form.  d_of(i) / z_of(i) hand over chunk i of
// d = dy16 + dy32 and of z: from memory in the one, from the prefetched LnRes32BwdRow in the other.  Callables, not two
// filled arrays: the reduce of a chunk stays next to its operands; with the row gathered first the compiler contracts the
// terms of s2 the other way round (which product goes into the fma) and dz differs in the last bit.
// dz_bf16: dz_out is a bf16 tensor (the residual was a bf16 tensor -- where an fp32 residual stream starts).
template <int NV, typename D, typename Z>
__device__ __forceinline__ void ln_res32_bwd_row(int row, int lane, D&& d_of, Z&& z_of, float mu, float rs,
                                                 const float4 (&g)[NV], float4 (&ag)[NV], float4 (&ab)[NV], float4 (&ax)[NV],
                                                 float* __restrict__ dz_out, bf16_raw* __restrict__ dx_out, int dz_bf16,
                                                 float drop_p, uint32_t drop_key, uint32_t drop_thr, float keep_scale) {
  constexpr int H = NV * 256;
  float4 d[NV], xh[NV];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    d[i] = d_of(i);
    const float4 zz = z_of(i);
    ln_bwd_chunk_reduce(d[i], zz, mu, rs, g[i], xh[i], ag[i], ab[i], s1, s2);
  }
  s1 = wave_sum(s1) * (1.0f / H);
  s2 = wave_sum(s2) * (1.0f / H);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (i * 64 + lane) * 4;
    float4 o = ln_bwd_chunk_dz(d[i], xh[i], rs, s1, s2);
    if (dz_out != nullptr) {
      if (dz_bf16) st4<bf16_raw>(reinterpret_cast<bf16_raw*>(dz_out) + (size_t)row * H + col, o);
      else st4<float>(dz_out + (size_t)row * H + col, o);
    }
    if (drop_p > 0.f) o = bb_drop4(o, (uint32_t)row * H + col, drop_key, drop_thr, keep_scale);
    if (dx_out != nullptr) st4<bf16_raw>(dx_out + (size_t)row * H + col, o);
    add4(ax[i], o);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void ln_res32_bwd_kernel(const bf16_raw* __restrict__ dy16, const float* __restrict__ dy32,
                                                           const float* __restrict__ z, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           float* __restrict__ dz_out, bf16_raw* __restrict__ dx_out,
                                                           float* __restrict__ partials, int rows, float drop_p,
                                                           uint32_t drop_thr, uint32_t drop_key,
                                                           const uint32_t* __restrict__ salt, int dz_bf16) {
  constexpr int H = NV * 256;
  if (drop_p > 0.f) drop_key = bb_salted(drop_key, salt);
  __shared__ float4 s_red[3][4][NV * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  float4 ag[NV], ab[NV], ax[NV];
  float4 g[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    ag[i] = ab[i] = ax[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    g[i] = *reinterpret_cast<const float4*>(gamma + (i * 64 + lane) * 4);
  }
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const float mu = mean[row], rs = rstd[row];
    auto d_of = [&](int i) __attribute__((always_inline)) {
      const size_t at = (size_t)row * H + (i * 64 + lane) * 4;
      float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
      if (dy16 != nullptr) d = ld4<bf16_raw>(dy16 + at);
      if (dy32 != nullptr) add4(d, ld4<float>(dy32 + at));
      return d;
    };
    auto z_of = [&](int i) __attribute__((always_inline)) { return ld4<float>(z + (size_t)row * H + (i * 64 + lane) * 4); };
    ln_res32_bwd_row<NV>(row, lane, d_of, z_of, mu, rs, g, ag, ab, ax, dz_out, dx_out, dz_bf16, drop_p, drop_key, drop_thr,
                         keep_scale);
  }
  ln_bwd_store_partials<NV>(s_red, ag, ab, ax, partials, lane, wave);
}

// The same with the NEXT row's loads in flight.  Up to 512 workgroups (5 120 rows) a launch has two waves per SIMD and a
// wave two or three rows, each a dependent load -> reduce -> store chain: the kernel is latency-bound and the registers for
// a second row are free.  The host picks this form there (ln_res32_bwd_loads_ahead); larger launches need four waves per
// SIMD (<= 128 VGPRs) and keep the kernel above.  Which rows a wave takes and the order in which it adds them into its
// column partials are those of the kernel above; the arithmetic of a row is the same function (ln_res32_bwd_row).
template <int NV> struct LnRes32BwdRow {
  uint2 d16[NV];          // dy16, packed (when there is one)
  float4 d32[NV], z[NV];  // dy32 (when there is one), z
  float mu, rs;
};
template <int NV>
__global__ __launch_bounds__(256) void ln_res32_bwd_ahead_kernel(const bf16_raw* __restrict__ dy16, const float* __restrict__ dy32,
                                                                 const float* __restrict__ z, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 float* __restrict__ dz_out, bf16_raw* __restrict__ dx_out,
                                                                 float* __restrict__ partials, int rows, float drop_p,
                                                                 uint32_t drop_thr, uint32_t drop_key,
                                                                 const uint32_t* __restrict__ salt, int dz_bf16) {
  constexpr int H = NV * 256;
  if (drop_p > 0.f) drop_key = bb_salted(drop_key, salt);
  __shared__ float4 s_red[3][4][NV * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  float4 ag[NV], ab[NV], ax[NV];
  float4 g[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    ag[i] = ab[i] = ax[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    g[i] = *reinterpret_cast<const float4*>(gamma + (i * 64 + lane) * 4);
  }
  auto fill = [&](LnRes32BwdRow<NV>& r, int row) __attribute__((always_inline)) {
    r.mu = mean[row];
    r.rs = rstd[row];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const size_t at = (size_t)row * H + (i * 64 + lane) * 4;
      if (dy16 != nullptr) r.d16[i] = raw4<bf16_raw>::ld(dy16 + at);
      if (dy32 != nullptr) r.d32[i] = raw4<float>::ld(dy32 + at);
      r.z[i] = raw4<float>::ld(z + at);
    }
  };
  auto apply = [&](int row, const LnRes32BwdRow<NV>& r) __attribute__((always_inline)) {
    auto d_of = [&](int i) __attribute__((always_inline)) {
      float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
      if (dy16 != nullptr) d = raw4<bf16_raw>::f32(r.d16[i]);
      if (dy32 != nullptr) add4(d, r.d32[i]);
      return d;
    };
    auto z_of = [&](int i) __attribute__((always_inline)) { return r.z[i]; };
    ln_res32_bwd_row<NV>(row, lane, d_of, z_of, r.mu, r.rs, g, ag, ab, ax, dz_out, dx_out, dz_bf16, drop_p, drop_key, drop_thr,
                         keep_scale);
  };
  walk_rows_ahead<LnRes32BwdRow<NV>>(blockIdx.x * 4 + wave, rows, gridDim.x * 4, fill, apply);
  ln_bwd_store_partials<NV>(s_red, ag, ab, ax, partials, lane, wave);
}

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
static void launch_finalize(const float* partials, int nblocks, int nwhich, int C, float* o0, float* o1, float* o2,
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

// =============================================================================================
// K6: weighted segment gather: out[r] = sum_{e in [rowptr[r], rowptr[r+1])} w[e] * src[idx[e]]
// (gmap node aggregation with the CSR built on the host from the vpid lists; its backward is the same
//  kernel over the transposed CSR).
// =============================================================================================
template <typename T>
__global__ __launch_bounds__(192) void gather_wsum_kernel(const T* __restrict__ src, const int* __restrict__ rowptr,
                                                          const int* __restrict__ idx, const float* __restrict__ w,
                                                          T* __restrict__ out, int H) {
  const int r = blockIdx.x;
  const int e0 = rowptr[r], e1 = rowptr[r + 1];
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = e0; e < e1; ++e) {
      const float ww = w[e];
      const float4 v = ld4<T>(src + (size_t)idx[e] * H + c);
      acc.x += ww * v.x; acc.y += ww * v.y; acc.z += ww * v.z; acc.w += ww * v.w;
    }
    st4<T>(out + (size_t)r * H + c, acc);
  }
}

// sink[i] += sum_s partials[s][i]: the reduction step of the host-side split-K weight-gradient GEMMs, fused with the
// accumulation into the fp32 gradient arena (replaces a torch sum + add_ pair).  S is small (<= 32).
// Both folds below are latency times a trip count, not bandwidth, when a thread has one load in flight (the first form:
// 16 x (1 + S) dependent round trips per 4096-group task).  accum_fold keeps ACCUM_U elements x ACCUM_SC slices in flight:
// every load of a batch is issued before the first add, through global-address-space pointers (a pointer read out of a
// task record is otherwise a flat one, and the store of one element would fence the loads of the next).  The adds of an
// element stay ((sink + p0) + p1) + ... + p(S-1), whatever S: slices beyond the last full batch are taken one at a time
// in the same order.  Elements past the end are clamped to the last one for the loads and not stored.
// STORE (a task flag of bevbert_multi_accum): the caller knows the sink range to be zero (the arena fill, nothing added
// since), so the chain starts from 0.f -- ((0 + p0) + p1) + ..., the same bits -- and the sink is never loaded: a third of
// the fold's bytes at fp32 S = 1, a quarter at bf16 S = 4.  The return value is the thread's sum of squares of what it stored, in
// the order it stored it (clamped duplicates not counted): the fused gradient norm of the NORM flag.
#define ACCUM_U 4
#define ACCUM_SC 4
// sink[i] (+)= sum_s part[s * stride4 + i] for the float4 groups i = first, first + step, ... < n4
template <typename T, bool STORE = false>
__device__ __forceinline__ float accum_fold(const T* part_, float* sink_, size_t stride4, size_t n4, int S, size_t first,
                                            size_t step) {
  const BB_GLOBAL T* __restrict__ part = (const BB_GLOBAL T*)part_;
  BB_GLOBAL float* __restrict__ sink = (BB_GLOBAL float*)sink_;
  float sq = 0.f;
  for (size_t i = first; i < n4; i += ACCUM_U * step) {
    size_t idx[ACCUM_U];
    float4 acc[ACCUM_U];
#pragma unroll
    for (int u = 0; u < ACCUM_U; ++u) {
      idx[u] = i + u * step < n4 ? i + u * step : n4 - 1;
      if constexpr (STORE) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      else acc[u] = gld4<float>(sink + idx[u] * 4);
    }
    int s = 0;
    for (; s + ACCUM_SC <= S; s += ACCUM_SC) {
      float4 v[ACCUM_SC][ACCUM_U];
#pragma unroll
      for (int k = 0; k < ACCUM_SC; ++k)
#pragma unroll
        for (int u = 0; u < ACCUM_U; ++u) v[k][u] = gld4<T>(part + ((size_t)(s + k) * stride4 + idx[u]) * 4);
#pragma unroll
      for (int k = 0; k < ACCUM_SC; ++k)
#pragma unroll
        for (int u = 0; u < ACCUM_U; ++u) add4(acc[u], v[k][u]);
    }
    for (; s < S; ++s) {
      float4 v[ACCUM_U];
#pragma unroll
      for (int u = 0; u < ACCUM_U; ++u) v[u] = gld4<T>(part + ((size_t)s * stride4 + idx[u]) * 4);
#pragma unroll
      for (int u = 0; u < ACCUM_U; ++u) add4(acc[u], v[u]);
    }
#pragma unroll
    for (int u = 0; u < ACCUM_U; ++u)
      if (i + u * step < n4) {
        const bb_f4v o = {acc[u].x, acc[u].y, acc[u].z, acc[u].w};
        *reinterpret_cast<BB_GLOBAL bb_f4v*>(sink + idx[u] * 4) = o;
        sq += (acc[u].x * acc[u].x + acc[u].y * acc[u].y) + (acc[u].z * acc[u].z + acc[u].w * acc[u].w);
      }
  }
  return sq;
}

template <typename T>
__global__ __launch_bounds__(256) void accum_partials_kernel(const T* __restrict__ partials, float* __restrict__ sink,
                                                             int S, size_t n4) {
  accum_fold<T>(partials, sink, n4, n4, S, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}

// Batched form of accum_partials_kernel: one launch folds the split-K partial products of EVERY weight-gradient GEMM of
// a backward pass into the fp32 gradient arena (~100 launches of 7-9 us per training step when issued one by one).
// A task = up to 4096 float4 of one weight; the host keeps the table on the device (ops.ReduceQueue).
struct AccumTask {
  const void* partials;    // [S][n4_total] float4-groups of T
  float* sink;             // this task's first element in the arena
  unsigned long long n4_total;   // stride between the S partial slices, in float4 groups
  unsigned int off4, n4;   // range of this task inside a slice, in float4 groups
  int S, dtype;            // dtype: bits 0-7 BB_F32 / BB_BF16, bit 8 STORE, bit 9 NORM, bits 12-31 the NORM slot
};
#define ACCUM_STORE 0x100
#define ACCUM_NORM 0x200
// sum of the 256 threads' values, in the fixed order of sumsq_kernel; the result is valid in thread 0
__device__ __forceinline__ float block_sum_256(float s) {
  __shared__ float sh[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
template <typename T, bool STORE>
__device__ __forceinline__ float accum_task(const AccumTask& t) {
  return accum_fold<T, STORE>((const T*)t.partials + (size_t)t.off4 * 4, t.sink, t.n4_total, t.n4, t.S, threadIdx.x, 256);
}
// NORM: slots[slot] = sum of squares of the task's stored values -- one writer per slot, no atomics; the optimiser sums
// the slots (clip_from_slots) instead of reading the arena again.  Ignored without a registered slot array
// (bevbert_set_fold_norm_slots) or with a slot beyond its capacity.
__global__ __launch_bounds__(256) void multi_accum_kernel(const AccumTask* __restrict__ tasks, float* __restrict__ slots,
                                                          unsigned int capacity) {
  const AccumTask t = tasks[blockIdx.x];
  const bool bf16 = (t.dtype & 0xff) == BB_BF16;
  float sq;
  if (t.dtype & ACCUM_STORE) sq = bf16 ? accum_task<bf16_raw, true>(t) : accum_task<float, true>(t);
  else sq = bf16 ? accum_task<bf16_raw, false>(t) : accum_task<float, false>(t);
  const unsigned int slot = (unsigned int)t.dtype >> 12;
  if ((t.dtype & ACCUM_NORM) && slot < capacity) {       // block-uniform: the barrier inside is reached by all or none
    sq = block_sum_256(sq);
    if (threadIdx.x == 0) slots[slot] = sq;
  }
}

// table_grad[t] += sum of d[r] over the rows r with ids[r] == t, WITHOUT atomics and in a fixed order (training runs are
// bit-reproducible; the reference's index_add is not).  One workgroup per gradient row r: it returns at once unless r
// is the FIRST row carrying its id (and the id is not padding_idx: nn.Embedding(padding_idx=0) gives the padding row no
// lookup gradient, vilmodel.py:50).  The leader's four waves each scan one contiguous quarter of the rows [r, rows) for
// the same id -- 64 ids per ballot, four ballots' loads in flight -- and add the matching rows of d in ascending row
// order, every lane owning its columns (no LDS list, no barrier inside the scan); the four partial sums are folded as
// (w0 + w1) + (w2 + w3) and the leader alone read-modify-writes the table row.  The result is a pure function of (ids, d).
// rows^2 / 256 id comparisons per launch (5 120 rows: the id vector stays in L2).
#define EG_MAXJ 4          // float4 column groups per lane: H <= 64 lanes * 4 floats * EG_MAXJ = 1024
// TO / ACCUM: the destination rows are fp32 and accumulated into (embedding tables in the gradient arena), or of the
// activations' type -- rows of a zero-initialised activation gradient, the backward of a row gather (bevbert_rows_scatter):
// ACCUM false stores the id's sum, true adds it to what the row holds (a second scatter onto the same tensor).
template <typename T, typename TO = float, bool ACCUM = true>
__global__ __launch_bounds__(256) void embedding_grad_kernel(const int64_t* __restrict__ ids, const T* __restrict__ d,
                                                             TO* __restrict__ table_grad, int rows, int H,
                                                             int padding_idx) {
  __shared__ int s_flag;
  __shared__ float s_part[4][256 * EG_MAXJ];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t id = ids[r];
  if (id == (int64_t)padding_idx) return;
  if (tid == 0) s_flag = 0;
  __syncthreads();
  int hit = 0;
  for (int i = tid; i < r; i += 256) hit |= (ids[i] == id);
  if (hit) s_flag = 1;
  __syncthreads();
  if (s_flag) return;                       // an earlier row leads this id
  float4 acc[EG_MAXJ];
#pragma unroll
  for (int j = 0; j < EG_MAXJ; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int span = rows - r, q = (span + 3) >> 2;
  const int lo = r + wave * q, hi = min(rows, lo + q);
  for (int base = lo; base < hi; base += 256) {
    unsigned long long bal[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {           // four independent loads, then four ballots
      const int i = base + 64 * u + lane;
      bal[u] = __ballot(i < hi && ids[i] == id);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      unsigned long long b = bal[u];
      while (b) {                           // wave-uniform: the matching rows of these 64, in ascending order
        const int row = base + 64 * u + (__ffsll((long long)b) - 1);
        b &= b - 1;
#pragma unroll
        for (int j = 0; j < EG_MAXJ; ++j) {
          const int c = (lane + 64 * j) * 4;
          if (c < H) add4(acc[j], ld4<T>(d + (size_t)row * H + c));
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < EG_MAXJ; ++j) *reinterpret_cast<float4*>(&s_part[wave][(lane + 64 * j) * 4]) = acc[j];
  __syncthreads();
  TO* dst = table_grad + (size_t)id * H;
  for (int c = tid * 4; c < H; c += 1024) {
    const float4 p0 = *reinterpret_cast<const float4*>(&s_part[0][c]), p1 = *reinterpret_cast<const float4*>(&s_part[1][c]);
    const float4 p2 = *reinterpret_cast<const float4*>(&s_part[2][c]), p3 = *reinterpret_cast<const float4*>(&s_part[3][c]);
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ACCUM) t = ld4<TO>(dst + c);
    t.x += (p0.x + p1.x) + (p2.x + p3.x); t.y += (p0.y + p1.y) + (p2.y + p3.y);
    t.z += (p0.z + p1.z) + (p2.z + p3.z); t.w += (p0.w + p1.w) + (p2.w + p3.w);
    st4<TO>(dst + c, t);
  }
}

// out[i, :] = src[ids[i], :]: one workgroup per output row (index_select of activation rows: the masked tokens of the
// MLM head, the candidate cells of the SAP head, the supervised cells of the semantic head)
template <typename T>
__global__ __launch_bounds__(256) void rows_gather_kernel(const T* __restrict__ src, const int64_t* __restrict__ ids,
                                                          T* __restrict__ out, int H) {
  const int64_t id = ids[blockIdx.x];
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4)
    st4<T>(out + (size_t)blockIdx.x * H + c, ld4<T>(src + (size_t)id * H + c));
}

// Small tables (2 .. ~128 rows: navigation types, step ids, token types) with MANY gradient rows: the atomic version
// piles 28 224 rows onto two destination rows.  Here workgroup (t, s) sums the rows of slice s whose id is t and writes
// partials[s][t][:]; the slices are folded into the fp32 table gradient by the step's batched second reduction stage
// (bevbert_multi_finalize): no atomics, a fixed summation order.  The id test is wave-uniform; the loads of a group of
// four rows are issued together.
template <typename T>
__global__ __launch_bounds__(256) void embedding_grad_sliced_kernel(const int64_t* __restrict__ ids, const T* __restrict__ d,
                                                                    float* __restrict__ partials, int rows, int H,
                                                                    int rows_per_slice, int ntab) {
  const int t = blockIdx.x, s = blockIdx.y;
  const int r0 = s * rows_per_slice, r1 = min(rows, r0 + rows_per_slice);
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = r0; r < r1; r += 4) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r + j < r1 && ids[r + j] == t) v[j] = ld4<T>(d + (size_t)(r + j) * H + c);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) add4(acc, v[j]);
    }
    *reinterpret_cast<float4*>(partials + ((size_t)s * ntab + t) * H + c) = acc;
  }
}

// =============================================================================================
// Flat-arena optimiser kernels.  The arena is padded so every tensor starts on a 1024-element
// boundary; flags[i] describes chunk i: bit0 = apply weight decay, bit1 = tensor has ever had a
// gradient (the reference skips params whose .grad is None: adamw.py:66-67).
// =============================================================================================
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, size_t n4, float* __restrict__ partials) {
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = *reinterpret_cast<const float4*>(g + i * 4);
    s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  __shared__ float sh[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// Sum of squares of the arena ranges no NORM fold covers (embedding tables, biases, LayerNorm vectors, padding): one
// block per record {ptr, n4 <= 4096 float4 groups, slot}, every load of a thread issued before its adds.
struct SumsqTask {
  const float* ptr;
  unsigned int n4, slot;
};
__global__ __launch_bounds__(256) void sumsq_tasks_kernel(const SumsqTask* __restrict__ tasks, float* __restrict__ slots,
                                                          unsigned int capacity) {
  const SumsqTask t = tasks[blockIdx.x];
  if (t.slot >= capacity) return;                        // block-uniform
  const unsigned int n4 = t.n4 < 4096u ? t.n4 : 4096u;
  float s = 0.f;
  if (n4) {
    const BB_GLOBAL float* __restrict__ g = (const BB_GLOBAL float*)t.ptr;
    float4 v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const unsigned int i = threadIdx.x + u * 256;
      v[u] = gld4<float>(g + (size_t)(i < n4 ? i : n4 - 1) * 4);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (threadIdx.x + u * 256 < n4) s += (v[u].x * v[u].x + v[u].y * v[u].y) + (v[u].z * v[u].z + v[u].w * v[u].w);
  }
  s = block_sum_256(s);
  if (threadIdx.x == 0) slots[t.slot] = s;
}

// scalars[0] = total L2 norm of (pre_scale * g) ; scalars[1] = multiplier the optimiser applies to g:
//   pre_scale * min(1, max_norm / (norm + 1e-6))      (torch.nn.utils.clip_grad_norm_)
__global__ void clip_coef_kernel(const float* __restrict__ partials, int n, float pre_scale, float max_norm,
                                 float* __restrict__ scalars) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partials[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(sh[0]) * pre_scale;
    float coef = 1.0f;
    if (max_norm > 0.f) {
      coef = max_norm / (norm + 1e-6f);
      coef = coef < 1.0f ? coef : 1.0f;
    }
    scalars[0] = norm;
    scalars[1] = pre_scale * coef;
  }
}

// One block per 1024-element chunk.  The bias-correction step count is PER CHUNK (the reference keeps state["step"]
// per parameter and only advances it when the parameter has a gradient: adamw.py:66-67,84,96-100).
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    bf16_raw* __restrict__ p_bf16, const uint8_t* __restrict__ flags,
                                                    int* __restrict__ chunk_steps, size_t nchunks,
                                                    const float* __restrict__ gscale_ptr,
                                                    const float* __restrict__ lr_ptr, float lr, float beta1,
                                                    float beta2, float eps, float wd, float log2_beta1,
                                                    float log2_beta2) {
  if (lr_ptr) lr = *lr_ptr;            // device-resident learning rate: a captured hipGraph replays with the current one
  const size_t chunk = blockIdx.x;
  if (chunk >= nchunks) return;
  const uint8_t f = flags[chunk];
  if (!(f & 2)) return;
  const int t = chunk_steps[chunk] + 1;          // every thread reads the old value before thread 0 bumps it
  __syncthreads();
  if (threadIdx.x == 0) chunk_steps[chunk] = t;
  // beta^t = 2^(t * log2(beta)) on the transcendental unit (two instructions per thread, exact to ~1e-7)
  const float bc1 = 1.0f - __builtin_amdgcn_exp2f((float)t * log2_beta1);
  const float bc2 = 1.0f - __builtin_amdgcn_exp2f((float)t * log2_beta2);
  const float step_size = lr * sqrtf(bc2) / bc1;
  const float gs = gscale_ptr ? *gscale_ptr : 1.0f;
  const float decay = (f & 1) ? lr * wd : 0.f;
  const size_t i = chunk * 1024 + threadIdx.x * 4;
  const float4 gg = *reinterpret_cast<const float4*>(g + i);
  float4 pp = *reinterpret_cast<float4*>(p + i);
  float4 mm = *reinterpret_cast<float4*>(m + i);
  float4 vv = *reinterpret_cast<float4*>(v + i);
#define UPD(c)                                                    \
  {                                                               \
    const float gr = gg.c * gs;                                   \
    mm.c = mm.c * beta1 + (1.0f - beta1) * gr;                    \
    vv.c = vv.c * beta2 + (1.0f - beta2) * gr * gr;               \
    pp.c = pp.c - step_size * (mm.c / (sqrtf(vv.c) + eps));       \
    pp.c = pp.c - decay * pp.c;                                   \
  }
  UPD(x) UPD(y) UPD(z) UPD(w)
#undef UPD
  *reinterpret_cast<float4*>(p + i) = pp;
  *reinterpret_cast<float4*>(m + i) = mm;
  *reinterpret_cast<float4*>(v + i) = vv;
  if (p_bf16 != nullptr) st4<bf16_raw>(p_bf16 + i, pp);
}

template <typename TO>
__global__ __launch_bounds__(256) void cast_f32_kernel(const float* __restrict__ src, TO* __restrict__ dst, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
    st4<TO>(dst + i * 4, *reinterpret_cast<const float4*>(src + i * 4));
}

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

// loss.mean() of the step (pretrain_src/train_r2r.py:263) with the zero-weight padding rows of a static batch:
// out = sum_i w[i] * x[i] / denom   (w NULL: all ones; denom from device memory when denom_dev is given -- the number of
// real rows of the batch that currently sits in the buffers).  One workgroup (n is at most a few thousand), fixed order.
__global__ __launch_bounds__(1024) void weighted_mean_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ denom_dev, float denom, int n,
                                                                 float* __restrict__ out) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) s += (w ? w[i] : 1.0f) * x[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < 16; ++i) t += sh[i];
    *out = t / (denom_dev ? *denom_dev : denom);
  }
}
__global__ __launch_bounds__(256) void weighted_mean_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ w,
                                                                const float* __restrict__ denom_dev, float denom, int n,
                                                                float* __restrict__ dx) {
  const float g = *dout / (denom_dev ? *denom_dev : denom);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dx[i] = (w ? w[i] : 1.0f) * g;
}

BEVBERT_API int bevbert_weighted_mean_fwd(const float* x, const float* w, const float* denom_dev, float denom, int n,
                                          float* out, hipStream_t stream) {
  BB_REQUIRE(n > 0 && x != nullptr && out != nullptr, "weighted_mean_fwd: empty input");
  hipLaunchKernelGGL(weighted_mean_fwd_kernel, dim3(1), dim3(1024), 0, stream, x, w, denom_dev, denom, n, out);
  BB_CHECK_LAUNCH("weighted_mean_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_weighted_mean_bwd(const float* dout, const float* w, const float* denom_dev, float denom, int n,
                                          float* dx, hipStream_t stream) {
  BB_REQUIRE(n > 0 && dout != nullptr && dx != nullptr, "weighted_mean_bwd: empty input");
  int nb = (n + 255) / 256;
  if (nb > 256) nb = 256;
  hipLaunchKernelGGL(weighted_mean_bwd_kernel, dim3(nb), dim3(256), 0, stream, dout, w, denom_dev, denom, n, dx);
  BB_CHECK_LAUNCH("weighted_mean_bwd");
  return BB_OK;
}

// Semantic head (pretrain_cmt.py:391-441, MaskSEM / SEM): the supervised cells are those of a boolean mask (two masks ANDed
// for MaskSEM) -- a data-dependent count only the device knows.  sem_select: ONE workgroup compacts their row numbers into a
// fixed-capacity index (padding: row 0, weight 0), and leaves the weights and the divisor of the mean (count x classes).
// bce_rows: sum over the classes of binary_cross_entropy_with_logits for the selected rows, labels read through the index.
__global__ __launch_bounds__(1024) void sem_select_kernel(const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2, int n,
                                                         int cap, int classes, int64_t* __restrict__ idx,
                                                         float* __restrict__ valid, float* __restrict__ denom) {
  __shared__ int s_cnt[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024, lo = t * per, hi = min(n, lo + per);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += (m1[i] != 0) && (m2 == nullptr || m2[i] != 0);
  s_cnt[t] = c;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {       // inclusive scan (Hillis-Steele; 10 rounds on 1024 counters)
    const int v = (t >= off) ? s_cnt[t - off] : 0;
    __syncthreads();
    s_cnt[t] += v;
    __syncthreads();
  }
  const int total = s_cnt[1023];
  int pos = s_cnt[t] - c;
  for (int i = lo; i < hi; ++i)
    if ((m1[i] != 0) && (m2 == nullptr || m2[i] != 0)) {
      if (pos < cap) idx[pos] = i;
      ++pos;
    }
  const int kept = total < cap ? total : cap;
  for (int i = t; i < cap; i += 1024) {
    if (i >= kept) idx[i] = 0;
    valid[i] = i < kept ? 1.0f : 0.0f;
  }
  if (t == 0) *denom = (float)total * (float)classes;
}

template <typename T>
__global__ __launch_bounds__(256) void bce_rows_fwd_kernel(const T* __restrict__ x, const uint8_t* __restrict__ labels,
                                                           const int64_t* __restrict__ idx, float* __restrict__ out, int rows,
                                                           int C) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint8_t* lab = labels + (size_t)(idx ? idx[row] : row) * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = io<T>::ld(x + (size_t)row * C + c), y = lab[c] ? 1.0f : 0.0f;
    s += fmaxf(v, 0.f) - v * y + log1pf(__expf(-fabsf(v)));       // the numerically stable form torch uses
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}
template <typename T>
__global__ __launch_bounds__(256) void bce_rows_bwd_kernel(const T* __restrict__ x, const uint8_t* __restrict__ labels,
                                                           const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                           T* __restrict__ dx, int rows, int C) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint8_t* lab = labels + (size_t)(idx ? idx[row] : row) * C;
  const float gr = g[row];
  for (int c = lane; c < C; c += 64) {
    const float v = io<T>::ld(x + (size_t)row * C + c), y = lab[c] ? 1.0f : 0.0f;
    io<T>::st(dx + (size_t)row * C + c, (1.0f / (1.0f + __expf(-v)) - y) * gr);
  }
}

BEVBERT_API int bevbert_sem_select(const uint8_t* mask1, const uint8_t* mask2, int n, int cap, int classes, int64_t* idx,
                                   float* valid, float* denom, hipStream_t stream) {
  BB_REQUIRE(mask1 != nullptr && n > 0 && cap > 0 && classes > 0, "sem_select: bad arguments");
  hipLaunchKernelGGL(sem_select_kernel, dim3(1), dim3(1024), 0, stream, mask1, mask2, n, cap, classes, idx, valid, denom);
  BB_CHECK_LAUNCH("sem_select");
  return BB_OK;
}

BEVBERT_API int bevbert_bce_rows_fwd(const void* logits, const uint8_t* labels, const int64_t* idx, float* out, int rows,
                                     int C, int dtype, hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && C > 0, "bce_rows_fwd: rows=%d C=%d", rows, C);
  if (rows == 0) return BB_OK;
  const dim3 grid((rows + 3) / 4);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bce_rows_fwd_kernel<T>, grid, dim3(256), 0, stream, (const T*)logits, labels, idx, out, rows, C);
  });
  if (!type_ok) return bb_dtype_unsupported("bce_rows_fwd", dtype);
  BB_CHECK_LAUNCH("bce_rows_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_bce_rows_bwd(const void* logits, const uint8_t* labels, const int64_t* idx, const float* g, void* dlogits,
                                     int rows, int C, int dtype, hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && C > 0, "bce_rows_bwd: rows=%d C=%d", rows, C);
  if (rows == 0) return BB_OK;
  const dim3 grid((rows + 3) / 4);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bce_rows_bwd_kernel<T>, grid, dim3(256), 0, stream, (const T*)logits, labels, idx, g, (T*)dlogits, rows, C);
  });
  if (!type_ok) return bb_dtype_unsupported("bce_rows_bwd", dtype);
  BB_CHECK_LAUNCH("bce_rows_bwd");
  return BB_OK;
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

// =============================================================================================
// C ABI
// =============================================================================================
// the three plain forward entries behind their argument checks; `name` as in their messages
template <bool GATHER>
static int ln_fwd_launch(const char* name, hipStream_t st, const void* x, const float* bias, const void* residual,
                         const float* gamma, const float* beta, void* y, void* z_out, float* mean, float* rstd,
                         int rows, int H, float eps, int dtype, float p, uint64_t seed, uint64_t offset,
                         const int64_t* ids, const void* word, const void* pos, const void* type_row, int L) {
  const dim3 grid((rows + 3) / 4);
  const uint32_t thr = bb_drop_threshold(p);
  bool width_ok = false;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    width_ok = bb_with_width<1, 2, 3, 4, 6, 8>(H, [&](auto nv) {
      hipLaunchKernelGGL((ln_fwd_kernel<T, decltype(nv)::value, GATHER>), grid, dim3(256), 0, st, (const T*)x, bias, (const T*)residual,
                         gamma, beta, (T*)y, (T*)z_out, mean, rstd, rows, eps, p, thr, bb_site_key(seed, offset), ids,
                         (const T*)word, (const T*)pos, (const T*)type_row, L, bb_step_salt());
    });
  });
  if (!type_ok) return bb_dtype_unsupported(name, dtype);
  if (!width_ok) {
    bb_set_error("layernorm: H=%d unsupported (need H in {256,512,768,1024,1536,2048})", H);
    return BB_EUNSUPPORTED;
  }
  BB_CHECK_LAUNCH(name);
  return BB_OK;
}

BEVBERT_API int bevbert_bias_dropout_residual_layernorm_fwd(const void* x, const float* bias, const void* residual,
                                                           const float* gamma, const float* beta, void* y, void* z_out,
                                                           float* mean, float* rstd, int rows, int H, float eps,
                                                           int dtype, float drop_p, uint64_t seed, uint64_t offset,
                                                           hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && H % 256 == 0, "layernorm_fwd: H=%d must be a multiple of 256", H);
  BB_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "layernorm_fwd: dropout p=%f", drop_p);
  if (rows == 0) return BB_OK;
  return ln_fwd_launch<false>("layernorm_fwd", stream, x, bias, residual, gamma, beta, y, z_out, mean, rstd, rows, H, eps,
                              dtype, drop_p, seed, offset, nullptr, nullptr, nullptr, nullptr, 1);
}

// y = LayerNorm(x + bias) + post1 + post2 (either may be NULL): the element-wise sums that follow a LayerNorm in the
// embedding compositions (vilmodel.py:494-532 image embeddings, :589-593 BEV input embedding) ride on its store.
BEVBERT_API int bevbert_layernorm_post_fwd(const void* x, const float* bias, const float* gamma, const float* beta,
                                           const void* post1, const void* post2, void* y, void* z_out, float* mean,
                                           float* rstd, int rows, int H, float eps, int dtype, hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && H % 256 == 0, "layernorm_post_fwd: H=%d must be a multiple of 256", H);
  if (rows == 0) return BB_OK;
  return ln_fwd_launch<false>("layernorm_post_fwd", stream, x, bias, nullptr, gamma, beta, y, z_out, mean, rstd, rows, H,
                              eps, dtype, 0.f, 0, 0, nullptr, post1, post2, nullptr, 1);
}

BEVBERT_API int bevbert_embed_sum_layernorm_fwd(const int64_t* ids, const void* word, const void* pos,
                                                const void* type_row, const float* gamma, const float* beta, void* y,
                                                void* z_out, float* mean, float* rstd, int rows, int L, int H,
                                                float eps, int dtype, float drop_p, uint64_t seed, uint64_t offset,
                                                hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && H % 256 == 0 && L > 0, "embed_sum_layernorm_fwd: bad shape rows=%d L=%d H=%d", rows, L, H);
  if (rows == 0) return BB_OK;
  return ln_fwd_launch<true>("embed_sum_layernorm_fwd", stream, nullptr, nullptr, nullptr, gamma, beta, y, z_out, mean,
                             rstd, rows, H, eps, dtype, drop_p, seed, offset, ids, word, pos, type_row, L);
}

// row groups of the column kernels (and of the LayerNorm backward, whose partial rows go through the same second stage):
// enough blocks to fill the chip, <= 1024 partial rows (BEVBERT_COLWISE_MAX_BLOCKS).  Rows per block: 16 from 8 192 rows
// up, i.e. the cap for the 28 224-row BEV problems: 1 024 blocks = four waves per SIMD.  Until round 6 the cap was 512 (two
// waves per SIMD): the fp32-stream LayerNorm backward, three input streams of 2 + 4 + 4 bytes per element and a reduction
// between its loads and its stores, ran at 4.1 TB/s; with 1 024 blocks 5.15 TB/s (84.3 -> 67.4 us; 768: 70.3, 1 280: 78.6 --
// an uneven last round --, 2 048: 69.2), the bf16 LayerNorm backward and the GELU backward do not care (31.4 -> 30.0,
// 105.4 -> 104.1 us), the bare column sums lose 0.8 us (r06al).  Below 8 192 rows the kernels are latency-bound -- a wave walks its rows one after the other, every row
// a dependent load -> reduce -> store chain -- and 10 rows per block (two or three per wave; 512 blocks for the 5 120 text
// rows instead of 320) shortens that chain; up to 512 blocks the fp32-stream LayerNorm backward also loads a wave's next
// row while it reduces the current one (ln_res32_bwd_loads_ahead).  BEVBERT_ROWS_PER_BLOCK overrides (A/B measurements).
static int colwise_max_blocks() {
  static const int cap = [] { const char* v = getenv("BEVBERT_COLWISE_MAX_BLOCKS"); const int c = v ? atoi(v) : 0; return c > 0 ? c : 1024; }();
  return cap;
}
static int colwise_blocks(int rows) {
  static const int env = [] { const char* v = getenv("BEVBERT_ROWS_PER_BLOCK"); return v ? atoi(v) : 0; }();
  const int per = env > 0 ? env : (rows >= 8192 ? 16 : 10);
  int nb = (rows + per - 1) / per;
  if (nb > colwise_max_blocks()) nb = colwise_max_blocks();
  return nb < 1 ? 1 : nb;
}

// ln_res32_bwd_ahead_kernel (the next row's loads in flight, ~190 VGPRs at H = 768) where its workgroups are all resident
// at two waves per SIMD: up to 512 of them on the 256 CUs, i.e. up to 5 120 rows.  Larger launches keep the plain kernel.
static bool ln_res32_bwd_loads_ahead(int nblocks) { return nblocks <= 512; }

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

static int layernorm_bwd_impl(const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                              void* dz, void* dx, const void* dz_add, float* dgamma, float* dbeta, float* dbias,
                              float* workspace, int rows, int H, int dtype, float drop_p, uint64_t seed, uint64_t offset,
                              int accumulate, hipStream_t stream) {
  BB_REQUIRE(H % 256 == 0, "layernorm_bwd: H=%d must be a multiple of 256", H);
  if (rows <= 0) return BB_OK;
  const int nb = colwise_blocks(rows);
  const uint32_t thr = bb_drop_threshold(drop_p);
  bool width_ok = false;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    width_ok = bb_with_width<1, 2, 3, 4>(H, [&](auto nv) {
      hipLaunchKernelGGL((ln_bwd_kernel<T, decltype(nv)::value>), dim3(nb), dim3(256), 0, stream, (const T*)dy, (const T*)z, mean, rstd,
                         gamma, (T*)dz, (T*)dx, workspace, rows, drop_p, thr, bb_site_key(seed, offset), bb_step_salt(),
                         (const T*)dz_add);
    });
  });
  if (!type_ok) return bb_dtype_unsupported("layernorm_bwd", dtype);
  if (!width_ok) {
    bb_set_error("layernorm_bwd: H=%d unsupported", H);
    return BB_EUNSUPPORTED;
  }
  BB_CHECK_LAUNCH("layernorm_bwd");
  if (dgamma || dbeta || dbias) launch_finalize(workspace, nb, 3, H, dgamma, dbeta, dbias, accumulate, stream);
  BB_CHECK_LAUNCH("layernorm_bwd finalize");
  return BB_OK;
}

BEVBERT_API int bevbert_layernorm_bwd(const void* dy, const void* z, const float* mean, const float* rstd,
                                      const float* gamma, void* dz, void* dx, float* dgamma, float* dbeta,
                                      float* dbias, float* workspace, int rows, int H, int dtype, float drop_p,
                                      uint64_t seed, uint64_t offset, int accumulate, hipStream_t stream) {
  return layernorm_bwd_impl(dy, z, mean, rstd, gamma, dz, dx, nullptr, dgamma, dbeta, dbias, workspace, rows, H, dtype,
                            drop_p, seed, offset, accumulate, stream);
}

// The same with an addend: dz (and dx behind the dropout mask) receive LayerNorm's input gradient PLUS dz_add -- the
// gradient that reaches z through its other consumer when z is also an output (the pre-norm residual stream of the
// panorama encoder: src = src + dropout(sublayer(norm(src))), transformer.py:170-182).
BEVBERT_API int bevbert_layernorm_bwd_add(const void* dy, const void* z, const float* mean, const float* rstd,
                                          const float* gamma, void* dz, void* dx, const void* dz_add, float* dgamma,
                                          float* dbeta, float* dbias, float* workspace, int rows, int H, int dtype,
                                          float drop_p, uint64_t seed, uint64_t offset, int accumulate,
                                          hipStream_t stream) {
  return layernorm_bwd_impl(dy, z, mean, rstd, gamma, dz, dx, dz_add, dgamma, dbeta, dbias, workspace, rows, H, dtype,
                            drop_p, seed, offset, accumulate, stream);
}

// bf16 activations around an fp32 residual stream (see ln_res32_*_kernel): residual_dtype BB_F32 / BB_BF16 (ignored when
// residual is NULL); y32 / z32 may be NULL (inference: no backward, or a consumer that only wants the bf16 copy)
BEVBERT_API int bevbert_layernorm_res32_fwd(const void* x, const float* bias, const void* residual, int residual_dtype,
                                            const float* gamma, const float* beta, void* y16, float* y32, float* z32,
                                            float* mean, float* rstd, int rows, int H, float eps, float drop_p,
                                            uint64_t seed, uint64_t offset, hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && H >= 256 && H % 256 == 0 && H / 256 <= 4, "layernorm_res32_fwd: H=%d must be 256, 512, 768 or 1024", H);
  BB_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "layernorm_res32_fwd: dropout p=%f", drop_p);
  BB_REQUIRE(residual == nullptr || residual_dtype == BB_F32 || residual_dtype == BB_BF16, "layernorm_res32_fwd: residual dtype %d", residual_dtype);
  if (rows == 0) return BB_OK;
  const dim3 grid((rows + 3) / 4);
  const uint32_t thr = bb_drop_threshold(drop_p);
  bb_with_type(residual != nullptr && residual_dtype == BB_BF16 ? BB_BF16 : BB_F32, [&](auto t) {
    using TR = decltype(t);
    bb_with_width<1, 2, 3, 4>(H, [&](auto nv) {
      hipLaunchKernelGGL((ln_res32_fwd_kernel<TR, decltype(nv)::value, false>), grid, dim3(256), 0, stream, (const bf16_raw*)x,
                         bias, (const TR*)residual, gamma, beta, (bf16_raw*)y16, y32, z32, mean, rstd, rows, eps, drop_p, thr,
                         bb_site_key(seed, offset), bb_step_salt(), LnPrev{});
    });
  });
  BB_CHECK_LAUNCH("layernorm_res32_fwd");
  return BB_OK;
}

// The same where the residual is the previous LayerNorm's fp32 output and that launch wrote no y32: the kernel recomputes
// it from what the producer saved for its own backward (z_prev, mean_prev, rstd_prev) and the producer's gamma / beta.
BEVBERT_API int bevbert_layernorm_res32_chain_fwd(const void* x, const float* bias, const float* z_prev,
                                                  const float* mean_prev, const float* rstd_prev, const float* gamma_prev,
                                                  const float* beta_prev, const float* gamma, const float* beta, void* y16,
                                                  float* y32, float* z32, float* mean, float* rstd, int rows, int H,
                                                  float eps, float drop_p, uint64_t seed, uint64_t offset,
                                                  hipStream_t stream) {
  BB_REQUIRE(rows >= 0 && H >= 256 && H % 256 == 0 && H / 256 <= 4, "layernorm_res32_chain_fwd: H=%d must be 256, 512, 768 or 1024", H);
  BB_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "layernorm_res32_chain_fwd: dropout p=%f", drop_p);
  if (rows == 0) return BB_OK;
  BB_REQUIRE(z_prev && mean_prev && rstd_prev && gamma_prev && beta_prev, "layernorm_res32_chain_fwd: %s", "the producer's z, mean, rstd, gamma and beta are all required");
  const dim3 grid((rows + 3) / 4);
  const uint32_t thr = bb_drop_threshold(drop_p);
  bb_with_width<1, 2, 3, 4>(H, [&](auto nv) {
    hipLaunchKernelGGL((ln_res32_fwd_kernel<float, decltype(nv)::value, true>), grid, dim3(256), 0, stream, (const bf16_raw*)x,
                       bias, z_prev, gamma, beta, (bf16_raw*)y16, y32, z32, mean, rstd, rows, eps, drop_p, thr,
                       bb_site_key(seed, offset), bb_step_salt(), LnPrev{mean_prev, rstd_prev, gamma_prev, beta_prev});
  });
  BB_CHECK_LAUNCH("layernorm_res32_chain_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_layernorm_res32_bwd(const void* dy16, const float* dy32, const float* z32, const float* mean,
                                            const float* rstd, const float* gamma, void* dz, void* dx16, float* dgamma,
                                            float* dbeta, float* dbias, float* workspace, int rows, int H, float drop_p,
                                            uint64_t seed, uint64_t offset, int accumulate, int dz_dtype,
                                            hipStream_t stream) {
  BB_REQUIRE(dz_dtype == BB_F32 || dz_dtype == BB_BF16, "layernorm_res32_bwd: dz dtype %d (fp32 or bf16)", dz_dtype);
  BB_REQUIRE(H >= 256 && H % 256 == 0 && H / 256 <= 4, "layernorm_res32_bwd: H=%d must be 256, 512, 768 or 1024", H);
  BB_REQUIRE(dy16 != nullptr || dy32 != nullptr, "layernorm_res32_bwd: no output gradient");
  if (rows <= 0) return BB_OK;
  const int nb = colwise_blocks(rows);
  const uint32_t thr = bb_drop_threshold(drop_p);
  bb_with_width<1, 2, 3, 4>(H, [&](auto nv) {
    auto* kernel = ln_res32_bwd_loads_ahead(nb) ? ln_res32_bwd_ahead_kernel<decltype(nv)::value> : ln_res32_bwd_kernel<decltype(nv)::value>;
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, stream, (const bf16_raw*)dy16, dy32, z32, mean,
                       rstd, gamma, (float*)dz, (bf16_raw*)dx16, workspace, rows, drop_p, thr, bb_site_key(seed, offset),
                       bb_step_salt(), dz_dtype == BB_BF16 ? 1 : 0);
  });
  BB_CHECK_LAUNCH("layernorm_res32_bwd");
  if (dgamma || dbeta || dbias) launch_finalize(workspace, nb, 3, H, dgamma, dbeta, dbias, accumulate, stream);
  BB_CHECK_LAUNCH("layernorm_res32_bwd finalize");
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

// tasks: device array of `ntasks` 40-byte records {u64 partials, u64 sink, u64 n4_total, u32 off4, u32 n4, i32 S, i32 dtype}
// dtype: bits 0-7 the dtype code, bit 8 STORE (the sink range is known to be zero: not read), bit 9 NORM (the task's sum
// of squares goes to slot `dtype >> 12` of the array registered with bevbert_set_fold_norm_slots); both zero: as before.
BEVBERT_API int bevbert_multi_accum(const void* tasks, int ntasks, hipStream_t stream) {
  static_assert(sizeof(AccumTask) == 40, "AccumTask is part of the C ABI");
  if (ntasks <= 0) return BB_OK;
  BB_REQUIRE(tasks != nullptr, "multi_accum: null task table");
  int capacity = 0;
  float* slots = bb_fold_norm_slots(&capacity);
  hipLaunchKernelGGL(multi_accum_kernel, dim3(ntasks), dim3(256), 0, stream, (const AccumTask*)tasks, slots,
                     (unsigned int)(slots ? capacity : 0));
  BB_CHECK_LAUNCH("multi_accum");
  return BB_OK;
}

// tasks: device array of `ntasks` 16-byte records {u64 ptr, u32 n4 <= 4096, u32 slot}: slots[slot] = sum of squares of the
// n4 float4 groups at ptr (slots: the array registered with bevbert_set_fold_norm_slots)
BEVBERT_API int bevbert_sumsq_tasks(const void* tasks, int ntasks, hipStream_t stream) {
  static_assert(sizeof(SumsqTask) == 16, "SumsqTask is part of the C ABI");
  if (ntasks <= 0) return BB_OK;
  int capacity = 0;
  float* slots = bb_fold_norm_slots(&capacity);
  BB_REQUIRE(tasks != nullptr && slots != nullptr, "sumsq_tasks: null task table, or no slot array registered");
  hipLaunchKernelGGL(sumsq_tasks_kernel, dim3(ntasks), dim3(256), 0, stream, (const SumsqTask*)tasks, slots,
                     (unsigned int)capacity);
  BB_CHECK_LAUNCH("sumsq_tasks");
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

BEVBERT_API int bevbert_segment_wsum(const void* src, const int* rowptr, const int* idx, const float* w, void* out,
                                     int out_rows, int H, int dtype, hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0, "segment_wsum: H=%d must be a multiple of 4", H);
  if (out_rows <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gather_wsum_kernel<T>, dim3(out_rows), dim3(192), 0, stream, (const T*)src, rowptr, idx, w, (T*)out, H);
  });
  if (!type_ok) return bb_dtype_unsupported("segment_wsum", dtype);
  BB_CHECK_LAUNCH("segment_wsum");
  return BB_OK;
}

BEVBERT_API int bevbert_accum_partials(const void* partials, float* sink, int S, int64_t n, int dtype,
                                       hipStream_t stream) {
  BB_REQUIRE(n % 4 == 0 && S >= 1, "accum_partials: n must be a multiple of 4 and S >= 1");
  if (n == 0) return BB_OK;
  size_t nb = ((size_t)n / 4 + 255) / 256;
  if (nb > 8192) nb = 8192;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(accum_partials_kernel<T>, dim3(nb), dim3(256), 0, stream, (const T*)partials, sink, S, (size_t)n / 4);
  });
  if (!type_ok) return bb_dtype_unsupported("accum_partials", dtype);
  BB_CHECK_LAUNCH("accum_partials");
  return BB_OK;
}

BEVBERT_API int bevbert_rows_gather(const void* src, const int64_t* ids, void* out, int rows, int H, int dtype,
                                    hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0 && H > 0, "rows_gather: H=%d must be a positive multiple of 4", H);
  if (rows <= 0) return BB_OK;
  const int nt = H / 4 >= 256 ? 256 : (H / 4 + 63) / 64 * 64;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(rows_gather_kernel<T>, dim3(rows), dim3(nt), 0, stream, (const T*)src, ids, (T*)out, H);
  });
  if (!type_ok) return bb_dtype_unsupported("rows_gather", dtype);
  BB_CHECK_LAUNCH("rows_gather");
  return BB_OK;
}

BEVBERT_API int bevbert_rows_scatter(const int64_t* ids, const void* d, void* out, int rows, int H, int dtype, int accumulate,
                                     hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0 && H <= 256 * EG_MAXJ, "rows_scatter: H=%d must be a multiple of 4 and <= %d", H, 256 * EG_MAXJ);
  if (rows <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    bb_with_bool(accumulate != 0, [&](auto accum) {
      hipLaunchKernelGGL((embedding_grad_kernel<T, T, decltype(accum)::value>), dim3(rows), dim3(256), 0, stream, ids, (const T*)d, (T*)out, rows, H, -1);
    });
  });
  if (!type_ok) return bb_dtype_unsupported("rows_scatter", dtype);
  BB_CHECK_LAUNCH("rows_scatter");
  return BB_OK;
}

BEVBERT_API int bevbert_embedding_grad(const int64_t* ids, const void* d, float* table_grad, int rows, int H,
                                       int padding_idx, int dtype, hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0 && H <= 256 * EG_MAXJ, "embedding_grad: H=%d must be a multiple of 4 and <= %d", H, 256 * EG_MAXJ);
  if (rows <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(embedding_grad_kernel<T>, dim3(rows), dim3(256), 0, stream, ids, (const T*)d, table_grad, rows, H, padding_idx);
  });
  if (!type_ok) return bb_dtype_unsupported("embedding_grad", dtype);
  BB_CHECK_LAUNCH("embedding_grad");
  return BB_OK;
}

BEVBERT_API int bevbert_embedding_grad_sliced(const int64_t* ids, const void* d, float* partials, int rows, int H,
                                              int table_rows, int rows_per_slice, int dtype, hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0, "embedding_grad_sliced: H=%d must be a multiple of 4", H);
  BB_REQUIRE(table_rows > 0 && rows_per_slice > 0 && rows > 0, "embedding_grad_sliced: empty problem (%d table rows, %d rows)",
             table_rows, rows);
  const int slices = (rows + rows_per_slice - 1) / rows_per_slice;
  BB_REQUIRE(slices <= 65535, "embedding_grad_sliced: %d slices exceed the grid limit", slices);
  const int nt = H / 4 < 256 ? ((H / 4 + 63) / 64) * 64 : 256;
  const dim3 grid(table_rows, slices);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(embedding_grad_sliced_kernel<T>, grid, dim3(nt), 0, stream, ids, (const T*)d, partials, rows, H, rows_per_slice,
                       table_rows);
  });
  if (!type_ok) return bb_dtype_unsupported("embedding_grad_sliced", dtype);
  BB_CHECK_LAUNCH("embedding_grad_sliced");
  return BB_OK;
}

// scalars: device float[2] -> {norm, grad multiplier}; partials: device float[1024]
BEVBERT_API int bevbert_grad_norm_clip(const float* grads, int64_t n, float pre_scale, float max_norm,
                                       float* partials, float* scalars, hipStream_t stream) {
  BB_REQUIRE(n % 4 == 0, "grad_norm_clip: n must be a multiple of 4");
  hipLaunchKernelGGL(sumsq_kernel, dim3(1024), dim3(256), 0, stream, grads, (size_t)n / 4, partials);
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, stream, partials, 1024, pre_scale, max_norm, scalars);
  BB_CHECK_LAUNCH("grad_norm_clip");
  return BB_OK;
}

// bevbert_grad_norm_clip's second half over `n` per-task sums of squares (NORM folds + bevbert_sumsq_tasks): fp64 sum in a
// fixed order, the same scalars[0..1]
BEVBERT_API int bevbert_clip_from_slots(const float* slots, int n, float pre_scale, float max_norm, float* scalars,
                                        hipStream_t stream) {
  BB_REQUIRE(n >= 0 && (slots != nullptr || n == 0) && scalars != nullptr, "clip_from_slots: null pointer or negative count");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, stream, slots, n, pre_scale, max_norm, scalars);
  BB_CHECK_LAUNCH("clip_from_slots");
  return BB_OK;
}

BEVBERT_API int bevbert_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                   void* params_bf16, const uint8_t* chunk_flags, int* chunk_steps, int64_t n,
                                   const float* grad_scale_dev, const float* lr_dev, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, hipStream_t stream) {
  BB_REQUIRE(n % 1024 == 0, "adamw_step: arena length must be a multiple of 1024 elements");
  BB_REQUIRE(chunk_steps != nullptr, "adamw_step: per-chunk step counters are required");
  const size_t nchunks = (size_t)n / 1024;
  hipLaunchKernelGGL(adamw_kernel, dim3(nchunks), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq,
                     (bf16_raw*)params_bf16, chunk_flags, chunk_steps, nchunks, grad_scale_dev, lr_dev, lr, beta1, beta2, eps,
                     weight_decay, (float)log2((double)beta1), (float)log2((double)beta2));
  BB_CHECK_LAUNCH("adamw_step");
  return BB_OK;
}

BEVBERT_API int bevbert_cast_f32(const float* src, void* dst, int64_t n, int dst_dtype, hipStream_t stream) {
  BB_REQUIRE(n % 4 == 0, "cast_f32: n must be a multiple of 4");
  if (n == 0) return BB_OK;
  size_t nb = ((size_t)n / 4 + 255) / 256;
  if (nb > 8192) nb = 8192;
  const bool type_ok = bb_with_type_of<bf16_raw, _Float16>(dst_dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(cast_f32_kernel<T>, dim3(nb), dim3(256), 0, stream, src, (T*)dst, (size_t)n / 4);
  });
  if (!type_ok) {                                             // its own wording: "dst dtype"
    bb_set_error("cast_f32: dst dtype %d unsupported", dst_dtype);
    return BB_EUNSUPPORTED;
  }
  BB_CHECK_LAUNCH("cast_f32");
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
