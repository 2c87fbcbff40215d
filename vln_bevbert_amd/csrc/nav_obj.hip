// Object grounding of the REVERIE / SOON fine-tune rollout on the device (vln_bevbert_amd/nav_expert.py, ops_rowops.py).
//
// The reference does this per sample in Python (map_nav_src/reverie/agent_obj.py:343-349 _nav_obj_variable, :384-400
// _teacher_object, :516-526 the 'og' record of node_stop_scores, :597-604 pred_objid; reverie/env.py:360-411 _eval_item /
// eval_metrics) with one .item() / torch.argmax sync per sample per step.  Here every piece is one small launch of fixed
// shape: the per-sample lengths are read on the device, nothing is derived on the host, so the launches sit inside a
// captured step.  No atomics; every row is written by exactly one thread or wave.
#include "nav_common.h"

#define NO_IGNORE (-100)

template <typename T> struct no_vec;                 // four elements of T as one load / store
template <> struct no_vec<float> { typedef float4 type; };
template <> struct no_vec<bf16_raw> { typedef uint2 type; };

// The object segment of sample b inside a panorama of L tokens, clamped so that no length can address outside
// pano (B,L,H) or obj (B,Op,H): rows [vl, vl + ol).
__device__ __forceinline__ void no_segment(const int64_t* __restrict__ view_len, const int64_t* __restrict__ obj_len,
                                           int b, int L, int Op, int& vl, int& ol) {
  const int64_t v = view_len[b], o = obj_len[b];
  vl = (int)(v < 0 ? 0 : (v > L ? L : v));
  const int room = min(Op, L - vl);
  ol = (int)(o < 0 ? 0 : (o > room ? room : o));
}

// ----------------------------------------------------------------------------------------------------------------
// (a) obj[b, j, :] = pano[b, view_len[b] + j, :] for j < obj_len[b], else 0; mask[b, j] = j < obj_len[b].
// One block per (j, b); the row moves as raw 4-element vectors (a pure copy: every bit pattern survives).
template <typename T>
__global__ __launch_bounds__(256) void no_rows_fwd_kernel(const T* __restrict__ pano, const int64_t* __restrict__ view_len,
                                                          const int64_t* __restrict__ obj_len, T* __restrict__ obj,
                                                          uint8_t* __restrict__ mask, int L, int Op, int H4) {
  typedef typename no_vec<T>::type V;
  const int j = blockIdx.x, b = blockIdx.y;
  int vl, ol;
  no_segment(view_len, obj_len, b, L, Op, vl, ol);
  const bool on = j < ol;
  V* dst = reinterpret_cast<V*>(obj) + ((size_t)b * Op + j) * H4;
  if (on) {
    const V* src = reinterpret_cast<const V*>(pano) + ((size_t)b * L + vl + j) * H4;
    for (int c = threadIdx.x; c < H4; c += 256) dst[c] = src[c];
  } else {
    V z;
    memset(&z, 0, sizeof(V));
    for (int c = threadIdx.x; c < H4; c += 256) dst[c] = z;
  }
  if (threadIdx.x == 0) mask[(size_t)b * Op + j] = on;
}

// The adjoint in store form: every row l of dpano (B,L,H) is written, with dobj[b, l - view_len[b]] inside the object
// segment and 0 elsewhere.  One block per (l, b).
template <typename T>
__global__ __launch_bounds__(256) void no_rows_bwd_kernel(const T* __restrict__ dobj, const int64_t* __restrict__ view_len,
                                                          const int64_t* __restrict__ obj_len, T* __restrict__ dpano,
                                                          int L, int Op, int H4) {
  typedef typename no_vec<T>::type V;
  const int l = blockIdx.x, b = blockIdx.y;
  int vl, ol;
  no_segment(view_len, obj_len, b, L, Op, vl, ol);
  V* dst = reinterpret_cast<V*>(dpano) + ((size_t)b * L + l) * H4;
  if (l >= vl && l < vl + ol) {
    const V* src = reinterpret_cast<const V*>(dobj) + ((size_t)b * Op + (l - vl)) * H4;
    for (int c = threadIdx.x; c < H4; c += 256) dst[c] = src[c];
  } else {
    V z;
    memset(&z, 0, sizeof(V));
    for (int c = threadIdx.x; c < H4; c += 256) dst[c] = z;
  }
}

static int no_rows_check(const char* name, int B, int L, int Op, int H) {
  BB_REQUIRE(B >= 0 && L >= 1 && Op >= 1 && H >= 4 && H % 4 == 0 && B <= 65535,
             "%s: B=%d L=%d Op=%d H=%d (H a multiple of 4, B <= 65535)", name, B, L, Op, H);
  return BB_OK;
}

BEVBERT_API int bevbert_obj_rows_fwd(const void* pano, const int64_t* view_len, const int64_t* obj_len, void* obj,
                                     uint8_t* mask, int B, int L, int Op, int H, int dtype, hipStream_t stream) {
  if (int rc = no_rows_check("obj_rows_fwd", B, L, Op, H)) return rc;
  BB_REQUIRE(pano && view_len && obj_len && obj && mask, "obj_rows_fwd: null pointer%s", "");
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    if (B > 0)
      hipLaunchKernelGGL(no_rows_fwd_kernel<T>, dim3(Op, B), dim3(256), 0, stream, (const T*)pano, view_len, obj_len,
                         (T*)obj, mask, L, Op, H / 4);
  });
  if (!type_ok) return bb_dtype_unsupported("obj_rows_fwd", dtype);
  BB_CHECK_LAUNCH("obj_rows_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_obj_rows_bwd(const void* dobj, const int64_t* view_len, const int64_t* obj_len, void* dpano, int B,
                                     int L, int Op, int H, int dtype, hipStream_t stream) {
  if (int rc = no_rows_check("obj_rows_bwd", B, L, Op, H)) return rc;
  BB_REQUIRE(dobj && view_len && obj_len && dpano, "obj_rows_bwd: null pointer%s", "");
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    if (B > 0)
      hipLaunchKernelGGL(no_rows_bwd_kernel<T>, dim3(L, B), dim3(256), 0, stream, (const T*)dobj, view_len, obj_len,
                         (T*)dpano, L, Op, H / 4);
  });
  if (!type_ok) return bb_dtype_unsupported("obj_rows_bwd", dtype);
  BB_CHECK_LAUNCH("obj_rows_bwd");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (b) Object supervision and record of one navigation step, one wave per sample.
//   targets: _teacher_object -- -100 when ended or cur is not one of end_vps[b, :n_end[b]], else the first slot whose id
//            is gt_obj[b] (-100 when there is none);
//   og_slot: torch.argmax of obj_logits[b, :obj_len[b]] -- the first maximum, a NaN beats every number and the first NaN
//            wins; -1 for a sample without objects;
//   stop_og: live samples record the id of that slot (-1 = None) under their current node; a revisit overwrites.
// `x2 at j2` is a better arg-max than `x at j` (j == INT_MAX: nothing yet).
__device__ __forceinline__ bool no_better(float x2, int j2, float x, int j) {
  if (j2 == 0x7fffffff) return false;
  if (j == 0x7fffffff) return true;
  const bool n2 = x2 != x2, n = x != x;
  if (n2 || n) return n2 && (!n || j2 < j);
  return x2 > x || (x2 == x && j2 < j);
}

__global__ __launch_bounds__(64) void no_step_kernel(const void* __restrict__ logits_, int bf16, int O,
                                                     const int* __restrict__ obj_ids, const int64_t* __restrict__ obj_len,
                                                     const int* __restrict__ gt_obj, const int* __restrict__ cur_,
                                                     const int* __restrict__ end_vps, const int* __restrict__ n_end, int E,
                                                     const uint8_t* __restrict__ ended, int* __restrict__ stop_og, int N,
                                                     int64_t* __restrict__ targets, int* __restrict__ og_slot) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t row = (size_t)b * O;
  const int64_t o64 = obj_len[b];
  const int ol = (int)(o64 < 0 ? 0 : (o64 > O ? O : o64));
  const int* ids = obj_ids + row;
  const int cur = cur_[b];
  const bool live = ended[b] == 0;
  // arg-max of the valid slots
  float m = 0.f;
  int am = 0x7fffffff;
  for (int j = lane; j < ol; j += 64) {
    const float x = bf16 ? bf16_to_f32(((const bf16_raw*)logits_)[row + j]) : ((const float*)logits_)[row + j];
    if (no_better(x, j, m, am)) { m = x; am = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const int a2 = __shfl_xor(am, o, 64);
    if (no_better(m2, a2, m, am)) { m = m2; am = a2; }
  }
  const int slot = am == 0x7fffffff ? -1 : am;
  // teacher: is cur a goal viewpoint, and the first slot that holds the target object
  const int ne = min(max(n_end[b], 0), E);
  int at_goal = 0, first = 0x7fffffff;
  for (int k = lane; k < ne; k += 64) at_goal |= end_vps[(size_t)b * E + k] == cur;
  const int want = gt_obj[b];
  for (int j = lane; j < ol; j += 64)
    if (ids[j] == want) { first = j; break; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    at_goal |= __shfl_xor(at_goal, o, 64);
    first = min(first, __shfl_xor(first, o, 64));
  }
  if (lane != 0) return;
  targets[b] = (live && at_goal && first != 0x7fffffff) ? first : NO_IGNORE;
  og_slot[b] = slot;
  if (live && (unsigned)cur < (unsigned)N) stop_og[(size_t)b * N + cur] = slot >= 0 ? ids[slot] : -1;
}

BEVBERT_API int bevbert_nav_obj_step(const void* obj_logits, int dtype, int B, int O, const int* obj_ids,
                                     const int64_t* obj_len, const int* gt_obj, const int* cur, const int* end_vps,
                                     const int* n_end, int E, const uint8_t* ended, int* stop_og, int N, int64_t* targets,
                                     int* og_slot, hipStream_t stream) {
  BB_REQUIRE(O >= 1 && E >= 1 && N >= 1, "nav_obj_step: O=%d E=%d N=%d", O, E, N);
  BB_REQUIRE(dtype == BB_F32 || dtype == BB_BF16, "nav_obj_step: dtype %d unsupported", dtype);
  BB_REQUIRE(obj_logits && obj_ids && obj_len && gt_obj && cur && end_vps && n_end && ended && stop_og && targets && og_slot,
             "nav_obj_step: null pointer%s", "");
  if (B <= 0) return BB_OK;
  hipLaunchKernelGGL(no_step_kernel, dim3(B), dim3(64), 0, stream, obj_logits, dtype == BB_BF16, O, obj_ids, obj_len, gt_obj,
                     cur, end_vps, n_end, E, ended, stop_og, N, targets, og_slot);
  BB_CHECK_LAUNCH("nav_obj_step");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (c) pred_objid of the samples that stop this step: the 'og' record of their stop node (-1 = None); other rows keep
// what they hold.  One thread per sample.
__global__ __launch_bounds__(64) void no_pick_kernel(const uint8_t* __restrict__ just_ended,
                                                     const int* __restrict__ stop_node, const int* __restrict__ stop_og,
                                                     int N, int* __restrict__ pred_obj, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B || !just_ended[b]) return;
  const int sn = stop_node[b];
  pred_obj[b] = (unsigned)sn < (unsigned)N ? stop_og[(size_t)b * N + sn] : -1;
}

BEVBERT_API int bevbert_nav_obj_pick(const uint8_t* just_ended, const int* stop_node, const int* stop_og, int N,
                                     int* pred_obj, int B, hipStream_t stream) {
  BB_REQUIRE(N >= 1, "nav_obj_pick: N=%d", N);
  BB_REQUIRE(just_ended && stop_node && stop_og && pred_obj, "nav_obj_pick: null pointer%s", "");
  if (B <= 0) return BB_OK;
  hipLaunchKernelGGL(no_pick_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, just_ended, stop_node, stop_og, N, pred_obj, B);
  BB_CHECK_LAUNCH("nav_obj_pick");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (d) reverie/env.py:360-383 _eval_item per finished trajectory in f64, one thread per sample, then eval_metrics' means in
// sample order.  items row: action_steps, trajectory_steps, trajectory_lengths, success, oracle_success, spl, rgs, rgspl.
#define NO_NM 8
__global__ __launch_bounds__(64) void no_metrics_kernel(const double* __restrict__ dist, int N, int S,
                                                        const int* __restrict__ scan, const int* __restrict__ path,
                                                        const int* __restrict__ path_len, int Lp,
                                                        const int* __restrict__ action_steps, const int* __restrict__ gt,
                                                        const int* __restrict__ gt_len, int Lg,
                                                        const int* __restrict__ goal_vps, const int* __restrict__ n_goal,
                                                        int E, const int* __restrict__ pred_obj,
                                                        const int* __restrict__ gt_obj, double* __restrict__ items, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double* o = items + (size_t)b * NO_NM;
  const int sc = scan[b];
  if ((unsigned)sc >= (unsigned)S) {                   // no such scan: every field NaN, as bevbert_nav_metrics answers
    for (int k = 0; k < NO_NM; ++k) o[k] = __builtin_nan("");
    return;
  }
  const int P = min(max(path_len[b], 1), Lp), G = min(max(gt_len[b], 1), Lg);
  const int* p = path + (size_t)b * Lp;
  const int* g = gt + (size_t)b * Lg;
  const int* gv = goal_vps + (size_t)b * E;
  const int ng = min(max(n_goal[b], 0), E);
  const double* d = dist + (size_t)sc * N * N;
  const double tlen = ne_path_length(d, N, p, P), glen = ne_path_length(d, N, g, G);
  bool last_in = false, any_in = false;
  for (int i = 0; i < P; ++i) {
    bool in = false;
    for (int k = 0; k < ng; ++k) in |= gv[k] == p[i];
    any_in |= in;
    if (i == P - 1) last_in = in;
  }
  const double success = last_in ? 1.0 : 0.0;
  const double rgs = pred_obj[b] == gt_obj[b] ? 1.0 : 0.0;
  const double denom = fmax(fmax(tlen, glen), 0.01);
  o[0] = action_steps[b];
  o[1] = P - 1;
  o[2] = tlen;
  o[3] = success;
  o[4] = any_in ? 1.0 : 0.0;
  o[5] = success * glen / denom;
  o[6] = rgs;
  o[7] = rgs * glen / denom;
}

__global__ __launch_bounds__(64) void no_metrics_mean_kernel(const double* __restrict__ items, int B,
                                                             double* __restrict__ avg) {
  const int k = threadIdx.x;
  if (k >= NO_NM) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += items[(size_t)b * NO_NM + k];
  avg[k] = s / B * (k >= 3 ? 100.0 : 1.0);
}

BEVBERT_API int bevbert_nav_metrics_obj(const double* dist, int N, int S, const int* scan, const int* path,
                                        const int* path_len, int Lp, const int* action_steps, const int* gt,
                                        const int* gt_len, int Lg, const int* goal_vps, const int* n_goal, int E,
                                        const int* pred_obj, const int* gt_obj, int B, double* items, double* avg,
                                        hipStream_t stream) {
  BB_REQUIRE(N >= 1 && S >= 1 && Lp >= 1 && Lg >= 1 && E >= 1, "nav_metrics_obj: N=%d S=%d Lp=%d Lg=%d E=%d", N, S, Lp, Lg, E);
  BB_REQUIRE(dist && scan && path && path_len && action_steps && gt && gt_len && goal_vps && n_goal && pred_obj && gt_obj &&
                 items, "nav_metrics_obj: null pointer%s", "");
  if (B <= 0) return BB_OK;
  hipLaunchKernelGGL(no_metrics_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, dist, N, S, scan, path, path_len, Lp,
                     action_steps, gt, gt_len, Lg, goal_vps, n_goal, E, pred_obj, gt_obj, items, B);
  BB_CHECK_LAUNCH("nav_metrics_obj");
  if (avg) {
    hipLaunchKernelGGL(no_metrics_mean_kernel, dim3(1), dim3(64), 0, stream, items, B, avg);
    BB_CHECK_LAUNCH("nav_metrics_obj_mean");
  }
  return BB_OK;
}
