// Fused tail of the single-action-prediction task: pretrain_src/model/pretrain_cmt.py:225-275 (forward_sap) after the
// three prediction heads --
//   fuse weight      fw = sigmoid(fuse_raw)            (0.5 when the model has no sap_fuse_linear)
//   global logits    gl = global_raw * fw,        -inf on visited nodes and beyond gmap_lens
//   local logits     ll = local_raw * (1 - fw),   -inf where the candidate's BEV cell is not navigable
//   fused logits     fu = gl + [ll | sum of ll over visited candidates | 0][src]     (vilmodel-side vpid matching: src)
//   loss             CE(gl, global label) + CE(ll, local label) + CE(fu, global label)
// A label of -100 is F.cross_entropy's ignore_index (the dataset's "no target", pretrain_src/data/dataset.py:132-156):
// a global label of -100 drops the global and the fused term, a local label of -100 the local term.  A dropped term
// adds 0 to the loss and nothing to any gradient; the sample's other terms are unchanged.  Any other label outside
// [0, G) / [0, K) is the caller's error, as it is in torch.
// In PyTorch this is ~35 elementwise / reduction launches forward and as many backward, each on a (B, <= 64) tensor.
// One wave per sample does all of it: lane j owns global-map node j and BEV candidate j.  The kernel also leaves the
// gradients w.r.t. the three head outputs for a unit upstream gradient; sap_loss_grad scales them by dloss[b].
//
// Below it, the other loss-head kernels, each under its own section comment: the row-wise cross-entropy of the MLM head,
// the weighted mean of the step's loss (pretrain_src/train_r2r.py:263), the semantic head's row selection and
// binary cross-entropy (pretrain_cmt.py:391-441), and the soft-target cross-entropy of the MRC head (pretrain_cmt.py:272-297).
#include "common.h"

template <typename T>
__global__ __launch_bounds__(64) void sap_loss_kernel(const T* __restrict__ graw, const T* __restrict__ lraw,
                                                      const T* __restrict__ fraw, const uint8_t* __restrict__ visited,
                                                      const int64_t* __restrict__ gmap_lens,
                                                      const uint8_t* __restrict__ nav_masks,
                                                      const int64_t* __restrict__ cand_idxs, const int64_t* __restrict__ src,
                                                      const uint8_t* __restrict__ vis_c, const int64_t* __restrict__ glabel,
                                                      const int64_t* __restrict__ llabel, float* __restrict__ loss,
                                                      float* __restrict__ dG, float* __restrict__ dL, float* __restrict__ dF,
                                                      int G, int K, int P) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float fw = fraw ? 1.0f / (1.0f + __expf(-io<T>::ld(fraw + b))) : 0.5f;
  const int gt = (int)glabel[b], lt = (int)llabel[b];
  const bool g_on = gt != -100, l_on = lt != -100;          // ignore_index: selects below, never a product with 0
  // global branch
  const bool gv = lane < G;
  const float gr = gv ? io<T>::ld(graw + (size_t)b * G + lane) : 0.f;
  const bool gmasked = !gv || visited[(size_t)b * G + lane] != 0 || lane >= (int)gmap_lens[b];
  const float gl = gmasked ? -INFINITY : gr * fw;
  // local branch
  const bool lv = lane < K;
  const float lr = lv ? io<T>::ld(lraw + (size_t)b * K + lane) : 0.f;
  const bool lmasked = !lv || nav_masks[(size_t)b * P + cand_idxs[(size_t)b * K + lane]] == 0;
  const float ll = lmasked ? -INFINITY : lr * (1.0f - fw);
  const bool vc = lv && vis_c[(size_t)b * K + lane] != 0;
  const float bw = wave_sum(vc ? ll : 0.f);
  // fused logits: ext = [ll (K) | bw | 0]
  const int s = gv ? (int)src[(size_t)b * G + lane] : K + 1;
  const float from_l = __shfl(ll, s < K ? s : 0, 64);
  const float fu = gv ? gl + (s < K ? from_l : (s == K ? bw : 0.f)) : -INFINITY;
  // three log-sum-exps
  const float mg = wave_max(gl), ml = wave_max(ll), mf = wave_max(fu);
  const float eg = __expf(gl - mg), el = __expf(ll - ml), ef = __expf(fu - mf);      // exp(-inf - m) = 0
  const float sg = wave_sum(eg), sl = wave_sum(el), sf = wave_sum(ef);
  const float lse_g = mg + __logf(sg), lse_l = ml + __logf(sl), lse_f = mf + __logf(sf);
  const float gl_t = __shfl(gl, g_on ? gt : 0, 64), ll_t = __shfl(ll, l_on ? lt : 0, 64);
  const float fu_t = __shfl(fu, g_on ? gt : 0, 64);
  if (lane == 0) loss[b] = (g_on ? lse_g - gl_t : 0.f) + (l_on ? lse_l - ll_t : 0.f) + (g_on ? lse_f - fu_t : 0.f);
  // gradients for dloss[b] = 1
  const float pg = eg / sg, pl = el / sl, pf = ef / sf;
  const float dfu = gv && g_on ? pf - (lane == gt ? 1.f : 0.f) : 0.f;
  const float dgl = gv && g_on ? (pg - (lane == gt ? 1.f : 0.f)) + dfu : 0.f;
  float dext = 0.f, dext_bw = 0.f;            // gather's backward: lane k sums the fused gradients routed to candidate k
  for (int j = 0; j < G; ++j) {               // in node order: the summation order is fixed
    const int sj = __shfl(s, j, 64);
    const float dj = __shfl(dfu, j, 64);
    if (sj == lane && lane < K) dext += dj;
    if (sj == K) dext_bw += dj;
  }
  const float dll = lv ? (l_on ? pl - (lane == lt ? 1.f : 0.f) : 0.f) + dext + (vc ? dext_bw : 0.f) : 0.f;
  const float dgr = gmasked ? 0.f : dgl * fw;
  const float dlr = lmasked ? 0.f : dll * (1.0f - fw);
  if (gv) dG[(size_t)b * G + lane] = dgr;
  if (lv) dL[(size_t)b * K + lane] = dlr;
  const float dfw = wave_sum(gmasked ? 0.f : dgl * gr) - wave_sum(lmasked ? 0.f : dll * lr);
  if (lane == 0) dF[b] = dfw * fw * (1.0f - fw);
}

template <typename T>
__global__ __launch_bounds__(64) void sap_loss_grad_kernel(const float* __restrict__ dG, const float* __restrict__ dL,
                                                           const float* __restrict__ dF, const float* __restrict__ dloss,
                                                           T* __restrict__ dgraw, T* __restrict__ dlraw, T* __restrict__ dfraw,
                                                           int G, int K) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float g = dloss[b];
  if (lane < G) io<T>::st(dgraw + (size_t)b * G + lane, dG[(size_t)b * G + lane] * g);
  if (lane < K) io<T>::st(dlraw + (size_t)b * K + lane, dL[(size_t)b * K + lane] * g);
  if (lane == 0 && dfraw) io<T>::st(dfraw + b, dF[b] * g);
}

BEVBERT_API int bevbert_sap_loss_fwd(const void* global_raw, const void* local_raw, const void* fuse_raw,
                                     const uint8_t* visited, const int64_t* gmap_lens, const uint8_t* nav_masks,
                                     const int64_t* cand_idxs, const int64_t* src, const uint8_t* vis_c,
                                     const int64_t* global_labels, const int64_t* local_labels, float* loss, float* dG,
                                     float* dL, float* dF, int B, int G, int K, int P, int dtype, hipStream_t stream) {
  BB_REQUIRE(G >= 1 && G <= 64 && K >= 1 && K <= 62, "sap_loss: G=%d (<= 64) / K=%d (<= 62) out of range", G, K);
  if (B <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(sap_loss_kernel<T>, dim3(B), dim3(64), 0, stream, (const T*)global_raw, (const T*)local_raw,
                       (const T*)fuse_raw, visited, gmap_lens, nav_masks, cand_idxs, src, vis_c, global_labels, local_labels,
                       loss, dG, dL, dF, G, K, P);
  });
  if (!type_ok) return bb_dtype_unsupported("sap_loss", dtype);
  BB_CHECK_LAUNCH("sap_loss_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_sap_loss_bwd(const float* dG, const float* dL, const float* dF, const float* dloss,
                                     void* d_global_raw, void* d_local_raw, void* d_fuse_raw, int B, int G, int K,
                                     int dtype, hipStream_t stream) {
  BB_REQUIRE(G >= 1 && G <= 64 && K >= 1 && K <= 62, "sap_loss: G=%d (<= 64) / K=%d (<= 62) out of range", G, K);
  if (B <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(sap_loss_grad_kernel<T>, dim3(B), dim3(64), 0, stream, dG, dL, dF, dloss, (T*)d_global_raw,
                       (T*)d_local_raw, (T*)d_fuse_raw, G, K);
  });
  if (!type_ok) return bb_dtype_unsupported("sap_loss", dtype);
  BB_CHECK_LAUNCH("sap_loss_bwd");
  return BB_OK;
}

// =============================================================================================
// Row-wise cross-entropy on wide rows (the MLM head: rows = masked tokens, C = vocabulary; pretrain_cmt.py:262-266
// F.cross_entropy(scores, labels, reduction="none") on fp32 copies of the logits).  Reads the head's logits in their
// own dtype, accumulates in fp32: forward = one pass for the maximum, one for the sum (the row stays in L2), loss and
// the log-sum-exp out, the latter as its two halves (lse[row] = the row maximum m, lse[rows + row] = log sum exp(x - m));
// backward writes d logits = (softmax - onehot) * dloss[row] in the logits' dtype.
// =============================================================================================
// A row starts at element row * C: the 4-wide loads begin at the first element whose index is a multiple of 4 (the
// vocabularies of the shipped configurations, 30 522 and 250 002, are not), scalars cover the ragged ends.
struct CeSpan { int head, nvec, tail0; };
__device__ __forceinline__ CeSpan ce_span(int row, int C) {
  const int head = min(C, (int)((4 - (((size_t)row * C) & 3)) & 3));
  const int nvec = (C - head) / 4;
  return {head, nvec, head + 4 * nvec};
}

template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                     float* __restrict__ loss, float* __restrict__ lse, int C) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* x = logits + (size_t)row * C;
  const CeSpan sp = ce_span(row, C);
  __shared__ float sh[4];
  float m = -INFINITY;
  for (int v = tid; v < sp.nvec; v += 256) {
    const float4 q = ld4<T>(x + sp.head + 4 * v);
    m = fmaxf(fmaxf(m, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
  }
  for (int c = tid; c < sp.head; c += 256) m = fmaxf(m, io<T>::ld(x + c));
  for (int c = sp.tail0 + tid; c < C; c += 256) m = fmaxf(m, io<T>::ld(x + c));
  m = wave_max(m);
  if ((tid & 63) == 0) sh[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  float s = 0.f;
  for (int v = tid; v < sp.nvec; v += 256) {
    const float4 q = ld4<T>(x + sp.head + 4 * v);
    s += (__expf(q.x - m) + __expf(q.y - m)) + (__expf(q.z - m) + __expf(q.w - m));
  }
  for (int c = tid; c < sp.head; c += 256) s += __expf(io<T>::ld(x + c) - m);
  for (int c = sp.tail0 + tid; c < C; c += 256) s += __expf(io<T>::ld(x + c) - m);
  s = wave_sum(s);
  if ((tid & 63) == 0) sh[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    const float ls = __logf((sh[0] + sh[1]) + (sh[2] + sh[3]));
    lse[row] = m;                        // the two halves of the log-sum-exp, see ce_bwd_kernel
    lse[gridDim.x + row] = ls;
    loss[row] = (m + ls) - io<T>::ld(x + target[row]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* __restrict__ lse, const float* __restrict__ dloss,
                                                     T* __restrict__ dlogits, int C) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* x = logits + (size_t)row * C;
  T* d = dlogits + (size_t)row * C;
  const CeSpan sp = ce_span(row, C);
  // softmax = exp((x - m) - log s): x - m is exact near the maximum, where the probabilities are large.  exp(x - lse)
  // would carry the rounding of lse = m + log s at the size of m -- 1.5e-5 of every probability at |m| = 300.
  const float m = lse[row], ls = lse[gridDim.x + row], g = dloss[row];
  const int t = (int)target[row];
  for (int v = tid; v < sp.nvec; v += 256) {
    const int c = sp.head + 4 * v;
    const float4 q = ld4<T>(x + c);
    float4 o = make_float4(__expf((q.x - m) - ls) * g, __expf((q.y - m) - ls) * g, __expf((q.z - m) - ls) * g,
                           __expf((q.w - m) - ls) * g);
    if (t == c) o.x -= g;
    if (t == c + 1) o.y -= g;
    if (t == c + 2) o.z -= g;
    if (t == c + 3) o.w -= g;
    st4<T>(d + c, o);
  }
  for (int c = tid; c < sp.head; c += 256)
    io<T>::st(d + c, (__expf((io<T>::ld(x + c) - m) - ls) - (c == t ? 1.f : 0.f)) * g);
  for (int c = sp.tail0 + tid; c < C; c += 256)
    io<T>::st(d + c, (__expf((io<T>::ld(x + c) - m) - ls) - (c == t ? 1.f : 0.f)) * g);
}

BEVBERT_API int bevbert_cross_entropy_fwd(const void* logits, const int64_t* target, float* loss, float* lse, int rows,
                                          int C, int dtype, hipStream_t stream) {
  BB_REQUIRE(C >= 1, "cross_entropy: C=%d", C);
  if (rows <= 0) return BB_OK;
  BB_REQUIRE(((uintptr_t)logits % 16) == 0, "cross_entropy: logits must be 16-byte aligned%s", "");
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ce_fwd_kernel<T>, dim3(rows), dim3(256), 0, stream, (const T*)logits, target, loss, lse, C);
  });
  if (!type_ok) return bb_dtype_unsupported("cross_entropy", dtype);
  BB_CHECK_LAUNCH("cross_entropy_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_cross_entropy_bwd(const void* logits, const int64_t* target, const float* lse, const float* dloss,
                                          void* dlogits, int rows, int C, int dtype, hipStream_t stream) {
  if (rows <= 0) return BB_OK;
  BB_REQUIRE(((uintptr_t)logits % 16) == 0 && ((uintptr_t)dlogits % 16) == 0,
             "cross_entropy: logits / dlogits must be 16-byte aligned%s", "");
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ce_bwd_kernel<T>, dim3(rows), dim3(256), 0, stream, (const T*)logits, target, lse, dloss, (T*)dlogits, C);
  });
  if (!type_ok) return bb_dtype_unsupported("cross_entropy", dtype);
  BB_CHECK_LAUNCH("cross_entropy_bwd");
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

// =============================================================================================
// Soft-target cross-entropy rows (the MRC head, pretrain_cmt.py:272-297: F.kl_div(F.log_softmax(pred.float()), probs,
// reduction="none").sum(1) over rows = masked objects, C = detector classes).  Logits in their own dtype, target rows
// fp32 read through an optional row index (duplicates allowed), statistics in fp32:
//   loss[r] = sum_c xlogy(t, t) - t * ((x - m) - ls)       m = row maximum, ls = log sum exp(x - m); t == 0 adds exactly 0
//   stats   = m (rows) | ls (rows) | S = sum_c t (rows)    m and ls apart for the reason given at ce_bwd_kernel
//   dlogits = (exp((x - m) - ls) * S - t) * dloss[r]       the detector's probabilities do not sum to 1 exactly
// About 100 rows of 1000 columns per step: one wave per row up to SOFT_CE_WAVE_ROW_MAX columns (four rows per workgroup),
// one workgroup per row beyond.  Rows need not start aligned: the ce_span split above.
// =============================================================================================
#define SOFT_CE_WAVE_ROW_MAX 1024

// sum / maximum over the NT threads that share a row (NT = 64: the wave; 256: the workgroup, through sh[4])
template <int NT> __device__ __forceinline__ float row_sum(float v, float* sh) {
  v = wave_sum(v);
  if constexpr (NT == 64) {
    return v;
  } else {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
  }
}
template <int NT> __device__ __forceinline__ float row_max(float v, float* sh) {
  v = wave_max(v);
  if constexpr (NT == 64) {
    return v;
  } else {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  }
}
// f(column, logit) for the columns thread t of NT owns: vectors of four from the first aligned element, scalars at the ends
template <typename T, int NT, typename F>
__device__ __forceinline__ void soft_ce_each(const T* __restrict__ x, const CeSpan sp, int C, int t, F&& f) {
  for (int v = t; v < sp.nvec; v += NT) {
    const int c = sp.head + 4 * v;
    const float4 q = ld4<T>(x + c);
    f(c, q.x); f(c + 1, q.y); f(c + 2, q.z); f(c + 3, q.w);
  }
  for (int c = t; c < sp.head; c += NT) f(c, io<T>::ld(x + c));
  for (int c = sp.tail0 + t; c < C; c += NT) f(c, io<T>::ld(x + c));
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void soft_ce_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ targets,
                                                          const int64_t* __restrict__ idx, float* __restrict__ loss,
                                                          float* __restrict__ stats, int rows, int C) {
  __shared__ float sh[4];
  const int row = NT == 64 ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x, t = threadIdx.x & (NT - 1);
  if (row >= rows) return;                       // NT = 64: whole waves leave, nothing below synchronises the workgroup
  const T* x = logits + (size_t)row * C;
  const float* tg = targets + (size_t)(idx ? idx[row] : row) * C;
  const CeSpan sp = ce_span(row, C);
  float m = -INFINITY;
  soft_ce_each<T, NT>(x, sp, C, t, [&](int, float v) { m = fmaxf(m, v); });
  m = row_max<NT>(m, sh);
  float s = 0.f;
  soft_ce_each<T, NT>(x, sp, C, t, [&](int, float v) { s += __expf(v - m); });
  const float ls = __logf(row_sum<NT>(s, sh));
  float l = 0.f, S = 0.f;
  soft_ce_each<T, NT>(x, sp, C, t, [&](int c, float v) {
    const float p = tg[c];
    S += p;
    if (p != 0.f) l += p * logf(p) - p * ((v - m) - ls);      // a select: a zero target adds exactly 0
  });
  l = row_sum<NT>(l, sh);
  S = row_sum<NT>(S, sh);
  if (t == 0) {
    loss[row] = l;
    stats[row] = m;
    stats[rows + row] = ls;
    stats[2 * rows + row] = S;
  }
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void soft_ce_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ targets,
                                                          const int64_t* __restrict__ idx, const float* __restrict__ stats,
                                                          const float* __restrict__ dloss, T* __restrict__ dlogits, int rows,
                                                          int C) {
  const int row = NT == 64 ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x, t = threadIdx.x & (NT - 1);
  if (row >= rows) return;
  const T* x = logits + (size_t)row * C;
  T* d = dlogits + (size_t)row * C;
  const float* tg = targets + (size_t)(idx ? idx[row] : row) * C;
  const CeSpan sp = ce_span(row, C);
  const float m = stats[row], ls = stats[rows + row], S = stats[2 * rows + row], g = dloss[row];
  for (int v = t; v < sp.nvec; v += NT) {
    const int c = sp.head + 4 * v;
    const float4 q = ld4<T>(x + c);
    st4<T>(d + c, make_float4((__expf((q.x - m) - ls) * S - tg[c]) * g, (__expf((q.y - m) - ls) * S - tg[c + 1]) * g,
                              (__expf((q.z - m) - ls) * S - tg[c + 2]) * g, (__expf((q.w - m) - ls) * S - tg[c + 3]) * g));
  }
  for (int c = t; c < sp.head; c += NT) io<T>::st(d + c, (__expf((io<T>::ld(x + c) - m) - ls) * S - tg[c]) * g);
  for (int c = sp.tail0 + t; c < C; c += NT) io<T>::st(d + c, (__expf((io<T>::ld(x + c) - m) - ls) * S - tg[c]) * g);
}

BEVBERT_API int bevbert_soft_ce_fwd(const void* logits, const float* targets, const int64_t* idx, float* loss, float* stats,
                                    int rows, int C, int dtype, hipStream_t stream) {
  BB_REQUIRE(C >= 1, "soft_ce: C=%d", C);
  if (rows <= 0) return BB_OK;
  BB_REQUIRE(((uintptr_t)logits % 16) == 0, "soft_ce: logits must be 16-byte aligned%s", "");
  if (dtype != BB_F32 && dtype != BB_BF16) return bb_dtype_unsupported("soft_ce", dtype);
  BB_REQUIRE(logits && targets && loss && stats, "soft_ce_fwd: null tensor%s", "");
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    if (C <= SOFT_CE_WAVE_ROW_MAX)
      hipLaunchKernelGGL((soft_ce_fwd_kernel<T, 64>), dim3((rows + 3) / 4), dim3(256), 0, stream, (const T*)logits, targets, idx,
                         loss, stats, rows, C);
    else
      hipLaunchKernelGGL((soft_ce_fwd_kernel<T, 256>), dim3(rows), dim3(256), 0, stream, (const T*)logits, targets, idx, loss,
                         stats, rows, C);
  });
  if (!type_ok) return bb_dtype_unsupported("soft_ce", dtype);
  BB_CHECK_LAUNCH("soft_ce_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_soft_ce_bwd(const void* logits, const float* targets, const int64_t* idx, const float* stats,
                                    const float* dloss, void* dlogits, int rows, int C, int dtype, hipStream_t stream) {
  BB_REQUIRE(C >= 1, "soft_ce: C=%d", C);
  if (rows <= 0) return BB_OK;
  BB_REQUIRE(((uintptr_t)logits % 16) == 0 && ((uintptr_t)dlogits % 16) == 0,
             "soft_ce: logits / dlogits must be 16-byte aligned%s", "");
  if (dtype != BB_F32 && dtype != BB_BF16) return bb_dtype_unsupported("soft_ce", dtype);
  BB_REQUIRE(logits && targets && stats && dloss && dlogits, "soft_ce_bwd: null tensor%s", "");
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    if (C <= SOFT_CE_WAVE_ROW_MAX)
      hipLaunchKernelGGL((soft_ce_bwd_kernel<T, 64>), dim3((rows + 3) / 4), dim3(256), 0, stream, (const T*)logits, targets, idx,
                         stats, dloss, (T*)dlogits, rows, C);
    else
      hipLaunchKernelGGL((soft_ce_bwd_kernel<T, 256>), dim3(rows), dim3(256), 0, stream, (const T*)logits, targets, idx, stats,
                         dloss, (T*)dlogits, rows, C);
  });
  if (!type_ok) return bb_dtype_unsupported("soft_ce", dtype);
  BB_CHECK_LAUNCH("soft_ce_bwd");
  return BB_OK;
}
