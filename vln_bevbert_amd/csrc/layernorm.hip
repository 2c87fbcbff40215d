// HBM-bound LayerNorm row kernels: K3 bias+dropout+residual+LayerNorm (fwd/bwd), K5 embedding-sum+LayerNorm, and the same
// pair around an fp32 residual stream (plain, chained, and the backward with the next row's loads in flight).
//
// Reference call sites replaced:
//   BertSelfOutput / BertOutput            pretrain_src/model/vilmodel.py:143-154,182-193  (dense bias + dropout + add + LN)
//   BertEmbeddings                         vilmodel.py:48-77
//
// Layout: activations are (rows, H) row-major with H % 256 == 0; one 64-lane wave owns one row and keeps it in
// registers (H/64 values per lane as float4s), so each tensor is read once and written once; statistics are fp32.
// The backward kernels leave per-block column partials; their second stage is colwise.hip's (rowops_common.h).
#include <math.h>
#include <type_traits>

#include "rowops_common.h"

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

// ln_res32_bwd_ahead_kernel (the next row's loads in flight, ~190 VGPRs at H = 768) where its workgroups are all resident
// at two waves per SIMD: up to 512 of them on the 256 CUs, i.e. up to 5 120 rows.  Larger launches keep the plain kernel.
static bool ln_res32_bwd_loads_ahead(int nblocks) { return nblocks <= 512; }

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
