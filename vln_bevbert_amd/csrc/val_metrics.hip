// Validation metrics of the pre-training tasks (pretrain_src/train_r2r.py:351-510 validate_mlm / _sap / _sem / _masksem,
// train_reverie_obj.py validate_og), accumulated on the device so that a validation pass reads back ONCE per task:
//   (a) bevbert_val_ce_rows    sum of cross-entropies, number of arg-max hits and number of rows of (R, C) logits
//   (a') bevbert_val_kl_rows   sum of KL divergences to soft target rows, arg-max agreements and number of rows (MRC)
//   (b) bevbert_val_bce_keys  sum of BCE-with-logits, number of rows, and one packed sort key per element for the AUC
//   (c) bevbert_val_auc        exact Mann-Whitney statistic 2U, P, N of an ascending-sorted key array, in integers
// Launch-only, caller-owned memory, no atomics: (a) and (b) leave one {value, flags} record per row in scratch, (c) one
// {sum, P, N} record per workgroup, and a single workgroup folds the records in index order -- two runs give the same
// bits.  The accumulator of (a) and (b) is three 8-byte words {double sum; int64 a; int64 b} the fold ADDS into.
#include "common.h"

#define VAL_WAVE_ROW_MAX 1024       // rows up to this width: one wave per row (SAP, OG); beyond: one workgroup (vocabulary)
#define VAL_AUC_MAX_WGS 1024

struct ValRow {                     // scratch record of one row
  float v;                          // its contribution to the fp64 sum (0 when it has none)
  uint32_t f;                       // bit 0 -> accumulator word a, bit 1 -> accumulator word b
};

// ---- one pass over a row: running maximum / sum of exponentials and the arg-max -------------------------------------
struct RowStat {
  float m, s, best;                 // running maximum, sum of exp(x - m); best value and its index (lowest index on a tie)
  int idx;
};
__device__ __forceinline__ void stat_init(RowStat& r) { r.m = -INFINITY; r.s = 0.f; r.best = -INFINITY; r.idx = 0x7fffffff; }
// a lane meets its elements in ascending index order, so `>` alone keeps the lowest index among equals; an element of
// -inf adds nothing to the sum (exp(-inf - m) = 0, and -inf - -inf would be NaN) but can still be the arg-max of a row
// that holds nothing else
__device__ __forceinline__ void stat_add(RowStat& r, float x, int i) {
  if (x > r.best || r.idx == 0x7fffffff) { r.best = x; r.idx = i; }
  if (x == -INFINITY) return;
  if (x > r.m) {
    r.s = r.s * expf(r.m - x) + 1.f;          // r.m = -inf: s = 0 * 0 + 1
    r.m = x;
  } else {
    r.s += expf(x - r.m);
  }
}
__device__ __forceinline__ void stat_merge(RowStat& r, float m, float s, float best, int idx) {
  if (best > r.best || (best == r.best && idx < r.idx)) { r.best = best; r.idx = idx; }
  const float M = fmaxf(r.m, m);
  if (M == -INFINITY) return;                  // both empty: s stays 0
  r.s = r.s * expf(r.m - M) + s * expf(m - M); // an empty side: 0 * exp(-inf) = 0
  r.m = M;
}
__device__ __forceinline__ void stat_wave(RowStat& r) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    stat_merge(r, __shfl_xor(r.m, o, 64), __shfl_xor(r.s, o, 64), __shfl_xor(r.best, o, 64), __shfl_xor(r.idx, o, 64));
}

// 16 bytes of T as floats
template <typename T> struct vec16;
template <> struct vec16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void ld(const float* p, float (&x)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  }
};
template <> struct vec16<bf16_raw> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void ld(const bf16_raw* p, float (&x)[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = __uint_as_float(w[i] << 16);
      x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
};

// NT threads (t = 0 .. NT-1) scan row p[0 .. C): 16-byte loads when the row starts on a 16-byte boundary, the tail and
// unaligned rows element by element
template <typename T, int NT>
__device__ __forceinline__ void row_scan(const T* __restrict__ p, int C, int t, RowStat& r) {
  constexpr int V = vec16<T>::N;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const int nv = C / V;
    for (int v = t; v < nv; v += NT) {
      float x[V];
      vec16<T>::ld(p + (size_t)v * V, x);
#pragma unroll
      for (int j = 0; j < V; ++j) stat_add(r, x[j], v * V + j);
    }
    done = nv * V;
  }
  for (int i = done + t; i < C; i += NT) stat_add(r, io<T>::ld(p + i), i);
}

// the record of a row from its merged statistics (one thread)
template <typename T>
__device__ __forceinline__ ValRow ce_record(const RowStat& r, const T* __restrict__ p, int C, int64_t target) {
  ValRow out;
  out.v = 0.f;
  out.f = 2u;                                            // counted in n_rows
  if (target >= 0 && target < C) {                       // ignore_index (and anything outside the row): no loss, no hit
    const float lse = r.m + logf(r.s);
    out.v = lse - io<T>::ld(p + target);
    out.f |= (r.idx == (int)target) ? 1u : 0u;
  }
  return out;
}

// (a1) one wave per row, four rows per workgroup
template <typename T>
__global__ __launch_bounds__(256) void val_ce_wave_kernel(const T* __restrict__ x, int64_t ld, const int64_t* __restrict__ target,
                                                          const float* __restrict__ valid, int R, int C,
                                                          ValRow* __restrict__ rec) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  if (valid && valid[row] == 0.f) {
    if (lane == 0) rec[row] = ValRow{0.f, 0u};
    return;
  }
  const T* p = x + (size_t)row * ld;
  RowStat r;
  stat_init(r);
  row_scan<T, 64>(p, C, lane, r);
  stat_wave(r);
  if (lane == 0) rec[row] = ce_record<T>(r, p, C, target[row]);
}

// (a2) one workgroup per row
template <typename T>
__global__ __launch_bounds__(256) void val_ce_block_kernel(const T* __restrict__ x, int64_t ld, const int64_t* __restrict__ target,
                                                           const float* __restrict__ valid, int R, int C,
                                                           ValRow* __restrict__ rec) {
  __shared__ RowStat part[4];
  const int row = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (valid && valid[row] == 0.f) {                      // uniform over the workgroup
    if (threadIdx.x == 0) rec[row] = ValRow{0.f, 0u};
    return;
  }
  const T* p = x + (size_t)row * ld;
  RowStat r;
  stat_init(r);
  row_scan<T, 256>(p, C, threadIdx.x, r);
  stat_wave(r);
  if (lane == 0) part[w] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) stat_merge(r, part[i].m, part[i].s, part[i].best, part[i].idx);
    rec[row] = ce_record<T>(r, p, C, target[row]);
  }
}

// The fold: ONE workgroup adds the R records into the accumulator.  Thread t sums records t, t + 256, ... in fp64 / int64,
// a fixed tree over the 256 partial sums follows, thread 0 adds the totals into acc.
__global__ __launch_bounds__(256) void val_fold_kernel(const ValRow* __restrict__ rec, int R, void* __restrict__ acc) {
  __shared__ double s_v[256];
  __shared__ long long s_a[256], s_b[256];
  const int t = threadIdx.x;
  double v = 0.0;
  long long a = 0, b = 0;
  for (int i = t; i < R; i += 256) {
    const ValRow r = rec[i];
    v += (double)r.v;
    a += r.f & 1u;
    b += (r.f >> 1) & 1u;
  }
  s_v[t] = v; s_a[t] = a; s_b[t] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { s_v[t] += s_v[t + o]; s_a[t] += s_a[t + o]; s_b[t] += s_b[t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    *reinterpret_cast<double*>(acc) += s_v[0];
    reinterpret_cast<long long*>(acc)[1] += s_a[0];
    reinterpret_cast<long long*>(acc)[2] += s_b[0];
  }
}

BEVBERT_API int bevbert_val_ce_rows(const void* logits, int64_t ld, const int64_t* target, const float* valid, int R, int C,
                                    int dtype, void* acc, void* scratch, hipStream_t stream) {
  BB_REQUIRE(R >= 0 && C >= 1 && ld >= C, "val_ce_rows: R=%d C=%d ld=%lld", R, C, (long long)ld);
  if (R == 0) return BB_OK;
  BB_REQUIRE(logits && target && acc && scratch, "val_ce_rows: null tensor%s", "");
  BB_REQUIRE(((uintptr_t)acc & 7) == 0 && ((uintptr_t)scratch & 7) == 0, "val_ce_rows: acc / scratch not 8-byte aligned%s", "");
  ValRow* rec = static_cast<ValRow*>(scratch);
  if (!bb_with_type(dtype, [&](auto T_) {
        using T = decltype(T_);
        if (C <= VAL_WAVE_ROW_MAX)
          hipLaunchKernelGGL(val_ce_wave_kernel<T>, dim3((R + 3) / 4), dim3(256), 0, stream, (const T*)logits, ld, target, valid,
                             R, C, rec);
        else
          hipLaunchKernelGGL(val_ce_block_kernel<T>, dim3(R), dim3(256), 0, stream, (const T*)logits, ld, target, valid, R, C,
                             rec);
      }))
    return bb_dtype_unsupported("val_ce_rows", dtype);
  BB_CHECK_LAUNCH("val_ce_rows");
  hipLaunchKernelGGL(val_fold_kernel, dim3(1), dim3(256), 0, stream, rec, R, acc);
  BB_CHECK_LAUNCH("val_ce_rows (fold)");
  return BB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// (a') Soft targets (MRC): the row's KL to a row of fp32 probabilities read through an index, and whether the two arg-maxes
// agree.  Pass one is (a)'s scan of the logits (m, s, arg-max); pass two walks the target row: its arg-max (lowest index on a
// tie: a thread meets its columns in ascending order) and sum_c xlogy(t, t) - t ((x - m) - log s), formed and summed in fp64
// from the fp32 statistics m and s, the fp32 difference x - m and the fp32 log t.  The row's sum is then rounded to fp32 once
// for its ValRow record, as (a)'s row loss is; the fold adds the records in fp64.
// NT = 64: one wave per row, four rows per workgroup; NT = 256: one workgroup per row.
struct KlPart { double kl; float best; int idx; };
__device__ __forceinline__ void kl_merge(KlPart& a, double kl, float best, int idx) {
  if (best > a.best || (best == a.best && idx < a.idx)) { a.best = best; a.idx = idx; }
  a.kl += kl;
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void val_kl_kernel(const T* __restrict__ x, int64_t ld, const float* __restrict__ targets,
                                                     const int64_t* __restrict__ idx, const float* __restrict__ valid, int R,
                                                     int C, ValRow* __restrict__ rec) {
  __shared__ RowStat part[4];
  __shared__ KlPart kpart[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = threadIdx.x & (NT - 1);
  const int row = NT == 64 ? blockIdx.x * 4 + w : blockIdx.x;
  if (row >= R) return;                                  // NT = 64: whole waves; nothing below synchronises them
  if (valid && valid[row] == 0.f) {                      // uniform over the row's threads
    if (t == 0) rec[row] = ValRow{0.f, 0u};
    return;
  }
  const T* p = x + (size_t)row * ld;
  const float* tg = targets + (size_t)(idx ? idx[row] : row) * C;
  RowStat r;
  stat_init(r);
  row_scan<T, NT>(p, C, t, r);
  stat_wave(r);                                          // every lane of the wave holds the wave's statistics
  if constexpr (NT == 256) {
    if (lane == 0) part[w] = r;
    __syncthreads();
    r = part[0];
    for (int i = 1; i < 4; ++i) stat_merge(r, part[i].m, part[i].s, part[i].best, part[i].idx);
  }
  const float m = r.m;
  const double ls = log((double)r.s);                    // x - m is exact in fp32 near the maximum; log s and the sum in fp64
  KlPart k{0.0, -INFINITY, 0x7fffffff};
  for (int c = t; c < C; c += NT) {
    const float q = tg[c];
    if (q > k.best || k.idx == 0x7fffffff) { k.best = q; k.idx = c; }
    if (q != 0.f) k.kl += (double)q * ((double)logf(q) - ((double)(io<T>::ld(p + c) - m) - ls));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kl_merge(k, __shfl_xor(k.kl, o, 64), __shfl_xor(k.best, o, 64), __shfl_xor(k.idx, o, 64));
  if constexpr (NT == 256) {
    if (lane == 0) kpart[w] = k;
    __syncthreads();
    k = kpart[0];
    for (int i = 1; i < 4; ++i) kl_merge(k, kpart[i].kl, kpart[i].best, kpart[i].idx);
  }
  if (t == 0) rec[row] = ValRow{(float)k.kl, 2u | (r.idx == k.idx ? 1u : 0u)};
}

BEVBERT_API int bevbert_val_kl_rows(const void* logits, int64_t ld, const float* targets, const int64_t* idx, const float* valid,
                                    int R, int C, int dtype, void* acc, void* scratch, hipStream_t stream) {
  BB_REQUIRE(R >= 0 && C >= 1 && ld >= C, "val_kl_rows: R=%d C=%d ld=%lld", R, C, (long long)ld);
  if (R == 0) return BB_OK;
  if (dtype != BB_F32 && dtype != BB_BF16) return bb_dtype_unsupported("val_kl_rows", dtype);
  BB_REQUIRE(logits && targets && acc && scratch, "val_kl_rows: null tensor%s", "");
  BB_REQUIRE(((uintptr_t)acc & 7) == 0 && ((uintptr_t)scratch & 7) == 0, "val_kl_rows: acc / scratch not 8-byte aligned%s", "");
  ValRow* rec = static_cast<ValRow*>(scratch);
  bb_with_type(dtype, [&](auto T_) {
    using T = decltype(T_);
    if (C <= VAL_WAVE_ROW_MAX)
      hipLaunchKernelGGL((val_kl_kernel<T, 64>), dim3((R + 3) / 4), dim3(256), 0, stream, (const T*)logits, ld, targets, idx, valid,
                         R, C, rec);
    else
      hipLaunchKernelGGL((val_kl_kernel<T, 256>), dim3(R), dim3(256), 0, stream, (const T*)logits, ld, targets, idx, valid, R, C,
                         rec);
  });
  BB_CHECK_LAUNCH("val_kl_rows");
  hipLaunchKernelGGL(val_fold_kernel, dim3(1), dim3(256), 0, stream, rec, R, acc);
  BB_CHECK_LAUNCH("val_kl_rows (fold)");
  return BB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) One wave per row (C = 40 classes).  key = (monotone_u32(logit) << 1) | (label != 0): ascending keys are ascending
// logits, equal logits are neighbours whatever their label.  monotone_u32 flips the sign bit of a non-negative float and
// all bits of a negative one; -0.0 is +0.0 first.  Rows with valid == 0 (the padding of a static batch) leave the
// sentinel INT64_MAX, which sorts behind every key (keys are < 2^33).  Element (r, c) goes to keys[cursor + r C + c]; a
// position >= capacity is dropped and *overflow becomes 1 (every writer stores the same value).
#define VAL_KEY_SENTINEL 0x7fffffffffffffffll
__device__ __forceinline__ uint32_t monotone_u32(float v) {
  uint32_t b = v == 0.f ? 0u : __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T>
__global__ __launch_bounds__(256) void val_bce_keys_kernel(const T* __restrict__ x, int64_t ld, const uint8_t* __restrict__ labels,
                                                           const int64_t* __restrict__ idx, const float* __restrict__ valid,
                                                           int R, int C, ValRow* __restrict__ rec, long long* __restrict__ keys,
                                                           int64_t cursor, int64_t capacity, long long* __restrict__ overflow) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const bool on = !(valid && valid[row] == 0.f);
  const uint8_t* lab = labels + (size_t)(idx ? idx[row] : row) * C;      // padding rows carry index 0: in bounds
  const int64_t base = cursor + (int64_t)row * C;
  float s = 0.f;
  bool dropped = false;
  for (int c = lane; c < C; c += 64) {
    long long key = VAL_KEY_SENTINEL;
    if (on) {
      const float v = io<T>::ld(x + (size_t)row * ld + c);
      const bool y = lab[c] != 0;
      // max(v, 0) - v y + log1p(exp(-|v|)) with the product written out, so that an infinite logit on the right side of
      // its label costs 0 and not inf - inf
      s += fmaxf(y ? -v : v, 0.f) + log1pf(expf(-fabsf(v)));
      key = (long long)(((uint64_t)monotone_u32(v) << 1) | (y ? 1u : 0u));
    }
    if (base + c < capacity) keys[base + c] = key; else dropped = true;
  }
  if (dropped) *overflow = 1;
  s = wave_sum(s);
  if (lane == 0) rec[row] = ValRow{on ? s : 0.f, on ? 1u : 0u};
}

BEVBERT_API int bevbert_val_bce_keys(const void* logits, int64_t ld, const uint8_t* labels, const int64_t* idx,
                                     const float* valid, int R, int C, int dtype, void* acc, void* scratch, int64_t* keys,
                                     int64_t cursor, int64_t capacity, int64_t* overflow, hipStream_t stream) {
  BB_REQUIRE(R >= 0 && C >= 1 && ld >= C, "val_bce_keys: R=%d C=%d ld=%lld", R, C, (long long)ld);
  BB_REQUIRE(cursor >= 0 && capacity >= 0, "val_bce_keys: cursor=%lld capacity=%lld", (long long)cursor, (long long)capacity);
  if (R == 0) return BB_OK;
  BB_REQUIRE(logits && labels && acc && scratch && keys && overflow, "val_bce_keys: null tensor%s", "");
  BB_REQUIRE(((uintptr_t)acc & 7) == 0 && ((uintptr_t)scratch & 7) == 0, "val_bce_keys: acc / scratch not 8-byte aligned%s", "");
  ValRow* rec = static_cast<ValRow*>(scratch);
  if (!bb_with_type(dtype, [&](auto T_) {
        using T = decltype(T_);
        hipLaunchKernelGGL(val_bce_keys_kernel<T>, dim3((R + 3) / 4), dim3(256), 0, stream, (const T*)logits, ld, labels, idx,
                           valid, R, C, rec, reinterpret_cast<long long*>(keys), cursor, capacity,
                           reinterpret_cast<long long*>(overflow));
      }))
    return bb_dtype_unsupported("val_bce_keys", dtype);
  BB_CHECK_LAUNCH("val_bce_keys");
  hipLaunchKernelGGL(val_fold_kernel, dim3(1), dim3(256), 0, stream, rec, R, acc);
  BB_CHECK_LAUNCH("val_bce_keys (fold)");
  return BB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// (c) Exact AUC statistic of sorted keys.  With 0-based positions, a positive whose tie group (equal key >> 1) is [s, e)
// has the mid-rank (s + e + 1) / 2, and U = sum of the positives' ranks - P (P + 1) / 2, so
//     2U = sum over positives (s + e + 1) - P (P + 1)                     -- integers throughout.
// A thread looks at its neighbours first: a key whose neighbours differ is its own group (the common case on continuous
// logits); otherwise the group's end on the tied side is found by a binary search.  Sentinels sort last and are skipped.
__device__ __forceinline__ int lower_bound_ll(const long long* __restrict__ k, int n, long long x) {   // first i with k[i] >= x
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (k[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void val_auc_partial_kernel(const long long* __restrict__ k, int n, long long* __restrict__ part) {
  __shared__ long long s_s[256], s_p[256], s_n[256];
  const int t = threadIdx.x;
  long long sum = 0, P = 0, N = 0;
  for (long long i0 = (long long)blockIdx.x * 256 + t; i0 < n; i0 += (long long)gridDim.x * 256) {
    const int i = (int)i0;
    const long long key = k[i];
    if (key == VAL_KEY_SENTINEL) continue;
    if (!(key & 1)) { ++N; continue; }
    ++P;
    const long long g = key >> 1;
    int s = i, e = i + 1;
    if (i > 0 && (k[i - 1] >> 1) == g) s = lower_bound_ll(k, i, g << 1);
    if (i + 1 < n && (k[i + 1] >> 1) == g) e = i + 1 + lower_bound_ll(k + i + 1, n - i - 1, (g + 1) << 1);
    sum += (long long)s + e + 1;
  }
  s_s[t] = sum; s_p[t] = P; s_n[t] = N;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { s_s[t] += s_s[t + o]; s_p[t] += s_p[t + o]; s_n[t] += s_n[t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    part[3 * blockIdx.x] = s_s[0];
    part[3 * blockIdx.x + 1] = s_p[0];
    part[3 * blockIdx.x + 2] = s_n[0];
  }
}

__global__ __launch_bounds__(64) void val_auc_fold_kernel(const long long* __restrict__ part, int nb, long long* __restrict__ out) {
  if (threadIdx.x != 0) return;
  long long sum = 0, P = 0, N = 0;
  for (int b = 0; b < nb; ++b) { sum += part[3 * b]; P += part[3 * b + 1]; N += part[3 * b + 2]; }
  out[0] = sum - P * (P + 1);
  out[1] = P;
  out[2] = N;
}

BEVBERT_API int bevbert_val_auc(const int64_t* sorted_keys, int64_t n, int64_t* out, void* scratch, hipStream_t stream) {
  BB_REQUIRE(n >= 0 && n < (1ll << 31), "val_auc: n=%lld (the contract is n < 2^31)", (long long)n);
  BB_REQUIRE(out && scratch && (sorted_keys || n == 0), "val_auc: null tensor%s", "");
  int nb = (int)((n + 255) / 256);
  if (nb > VAL_AUC_MAX_WGS) nb = VAL_AUC_MAX_WGS;
  long long* part = static_cast<long long*>(scratch);
  if (nb > 0) {
    hipLaunchKernelGGL(val_auc_partial_kernel, dim3(nb), dim3(256), 0, stream, reinterpret_cast<const long long*>(sorted_keys),
                       (int)n, part);
    BB_CHECK_LAUNCH("val_auc");
  }
  hipLaunchKernelGGL(val_auc_fold_kernel, dim3(1), dim3(64), 0, stream, part, nb, reinterpret_cast<long long*>(out));
  BB_CHECK_LAUNCH("val_auc (fold)");
  return BB_OK;
}
