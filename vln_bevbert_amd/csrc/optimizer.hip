// The split-K gradient folds with their fused norm, and the flat-arena optimiser kernels (K7 fused AdamW, grad-norm, clip
// coefficient, the fp32 -> 16-bit parameter cast).
//
// Reference call sites replaced:
//   clip_grad_norm_ + AdamW.step           pretrain_src/train_r2r.py:295-306, pretrain_src/optim/adamw.py:53-112
#include <math.h>
#include <type_traits>

#include "rowops_common.h"

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

// =============================================================================================
// C ABI
// =============================================================================================
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
