// Fine-tune supervision on the device (vln_bevbert_amd/nav_expert.py): DAgger expert targets, the action decision of a
// navigation step, the IL loss with ignore_index, and the evaluation metrics of finished trajectories.
//
// The reference does all of this in Python per sample (map_nav_src/r2r/agent.py:371-417,523-612; agent_base.py:148;
// r2r/env.py:309-378; r2r/eval_utils.py).  Graph distances come from the host-built tables of ScanGraphs:
//   dist (S,N,N) f64 = networkx all-pairs Dijkstra lengths, inf when unreachable / padding
//   pred (S,N,N) i16 = predecessor of v on networkx's path from u, -1 = none
// Node ids are scan indices in [0, N); any id outside that range reads as an unreachable node (distance inf).
// Every f64 distance sum is formed in the reference's order, so DTW values and spl keys are bit-equal to numpy's; the
// exp() of nDTW / CLS comes from the device math library.  No atomics: every reduction has a fixed order.
#include "nav_common.h"

#define NE_IGNORE (-100)
#define NE_MAX_P 1024      // DTW rows (prediction length + 1) per wave: one LDS column of f64 + the node sequence
#define NE_WAVES 4

// cal_dtw's table (eval_utils.py:6-14) by one wave: lanes over the reference index in blocks of 64, anti-diagonal
// steps.  At step k lane l computes D[i][j] with i = k - l, j = j0 + l + 1, from its own previous value (up), lane
// l-1's previous value (left) and lane l-1's value one step earlier (diag).  Lane 0 takes left / diag from `edge`, the
// column j0 of the previous block, which lane 63 overwrites in place: it writes row i at step i + 63, after lane 0 read
// rows i and i - 1 (at steps i and i + 1 <= i + 63).  Returns D[P][Lg] on every lane.  edge holds P + 1 doubles.
__device__ double ne_dtw(const double* __restrict__ d, int N, const int* seq, int P, const int* __restrict__ ref, int Lg,
                         double* edge) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; i <= P; i += 64) edge[i] = i == 0 ? 0.0 : NE_INF;
  __builtin_amdgcn_wave_barrier();
  double result = NE_INF;
  for (int j0 = 0; j0 < Lg; j0 += 64) {
    const int j = j0 + lane;
    const bool col = j < Lg;
    const int g = col ? ref[j] : -1;
    const int last = min(63, Lg - 1 - j0);
    double cur = NE_INF, old = NE_INF;
    for (int k = 1; k <= P + last; ++k) {
      const double nb_cur = __shfl_up(cur, 1, 64), nb_old = __shfl_up(old, 1, 64);
      const int i = k - lane;
      if (col && i >= 1 && i <= P) {
        const double left = lane == 0 ? edge[i] : nb_cur;
        const double diag = lane == 0 ? edge[i - 1] : nb_old;
        const double best = fmin(fmin(cur, left), diag);
        const double v = ne_d(d, N, seq[i - 1], g) + best;
        old = cur;
        cur = v;
        if (lane == 63) edge[i] = v;
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) edge[0] = NE_INF;
    __builtin_amdgcn_wave_barrier();
    result = __shfl(cur, last, 64);
  }
  return result;
}

// ----------------------------------------------------------------------------------------------------------------
// (a) imitation / spl: one thread per sample walks the slots in order (first strict minimum).
__global__ __launch_bounds__(64) void ne_expert_simple_kernel(
    const double* __restrict__ dist, int N, int S, const int* __restrict__ scan, const int* __restrict__ cur_,
    const int* __restrict__ cand, const uint8_t* __restrict__ visited, const uint8_t* __restrict__ ended,
    const int* __restrict__ gt, const int* __restrict__ gt_len, int Lg, int B, int C, int t, int policy,
    int64_t* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int sc = scan[b], cur = cur_[b];
  const int gl = min(max(gt_len[b], 0), Lg);
  const int* g = gt + (size_t)b * Lg;
  const int* cb = cand + (size_t)b * C;
  const uint8_t* vb = visited ? visited + (size_t)b * C : nullptr;
  if (ended[b] || (unsigned)sc >= (unsigned)S || gl == 0) {
    out[b] = NE_IGNORE;
    return;
  }
  int a = 0;
  if (policy == 0) {                                   // imitation_learning: the slot of gt[t + 1]
    if (t < gl - 1) {
      const int next = g[t + 1];
      for (int j = 1; j < C; ++j)
        if (cb[j] == next) { a = j; break; }
    }
  } else if (cur != g[gl - 1]) {                       // spl: d[vp][goal] + d[cur][vp]; 0 when arrived
    const double* d = dist + (size_t)sc * N * N;
    const int goal = g[gl - 1];
    double best = NE_INF;
    a = NE_IGNORE;
    for (int j = 1; j < C; ++j) {
      const int vp = cb[j];
      if (vp < 0 || (vb && vb[j])) continue;
      const double k = ne_d(d, N, vp, goal) + ne_d(d, N, cur, vp);
      if (k < best) { best = k; a = j; }
    }
  }
  out[b] = a;
}

// (a) ndtw: one block of NE_WAVES waves per sample; waves take the candidates round-robin; each wave rebuilds
// traj ++ shortest_path(cur, vp)[1:] in LDS from pred, runs the DTW, keeps its first strict minimum; the waves' bests
// are merged by (key, slot).
__global__ __launch_bounds__(64 * NE_WAVES) void ne_expert_kernel(
    const double* __restrict__ dist, const int16_t* __restrict__ pred, int N, int S, const int* __restrict__ scan,
    const int* __restrict__ cur_, const int* __restrict__ cand, const uint8_t* __restrict__ visited,
    const uint8_t* __restrict__ ended, const int* __restrict__ gt, const int* __restrict__ gt_len, int Lg,
    const int* __restrict__ traj, const int* __restrict__ traj_len, int Lt, int C,
    int64_t* __restrict__ out) {
  __shared__ double s_edge[NE_WAVES][NE_MAX_P];
  __shared__ int s_seq[NE_WAVES][NE_MAX_P];
  __shared__ double s_key[NE_WAVES];
  __shared__ int s_idx[NE_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int sc = scan[b], cur = cur_[b];
  const int gl = min(max(gt_len[b], 0), Lg);
  const int* g = gt + (size_t)b * Lg;
  const int* cb = cand + (size_t)b * C;
  const uint8_t* vb = visited ? visited + (size_t)b * C : nullptr;
  if (ended[b] || (unsigned)sc >= (unsigned)S || gl == 0) {
    if (tid == 0) out[b] = NE_IGNORE;
    return;
  }
  const double* d = dist + (size_t)sc * N * N;
  const int goal = g[gl - 1];
  if (cur == goal) {                                   // arrived: stop
    if (tid == 0) out[b] = 0;
    return;
  }
  // ndtw: -nDTW(traj ++ shortest_path(cur, vp)[1:], gt, 3.0)
  const int tl = min(max(traj_len[b], 0), Lt);
  const int16_t* pr = pred + ((size_t)sc * N + ((unsigned)cur < (unsigned)N ? cur : 0)) * N;
  int* seq = s_seq[w];
  for (int i = lane; i < tl; i += 64) seq[i] = traj[(size_t)b * Lt + i];
  double best = NE_INF;
  int besti = NE_IGNORE;
  for (int j = 1 + w; j < C; j += NE_WAVES) {
    const int vp = cb[j];
    if (vp < 0 || (vb && vb[j])) continue;
    // hop count of the path cur -> vp (walk back through pred), then write its nodes after the trajectory
    int h = 0, ok = (unsigned)cur < (unsigned)N && (unsigned)vp < (unsigned)N;
    if (ok) {
      for (int x = vp; x != cur; ++h) {
        x = pr[x];
        if (x < 0 || h >= N) { ok = 0; break; }
      }
    }
    if (!ok || tl + h > NE_MAX_P - 1) continue;        // no path in the reference's table: not a candidate
    if (lane == 0)
      for (int x = vp, i = tl + h - 1; i >= tl; --i, x = pr[x]) seq[i] = x;
    __builtin_amdgcn_wave_barrier();
    const double dtw = ne_dtw(d, N, seq, tl + h, g, gl, s_edge[w]);
    const double key = -exp(-dtw / (3.0 * gl));
    if (key < best) { best = key; besti = j; }
  }
  if (lane == 0) { s_key[w] = best; s_idx[w] = besti; }
  __syncthreads();
  if (tid == 0) {
    double k = s_key[0];
    int a = s_idx[0];
    for (int v = 1; v < NE_WAVES; ++v)
      if (s_key[v] < k || (s_key[v] == k && s_idx[v] != NE_IGNORE && (a == NE_IGNORE || s_idx[v] < a))) {
        k = s_key[v];
        a = s_idx[v];
      }
    out[b] = a;
  }
}

BEVBERT_API int bevbert_nav_expert(const double* dist, const int16_t* pred, int N, int S, const int* scan, const int* cur,
                                   const int* cand, const uint8_t* visited, const uint8_t* ended, const int* gt,
                                   const int* gt_len, int Lg, const int* traj, const int* traj_len, int Lt, int B, int C,
                                   int t, int policy, int64_t* out, hipStream_t stream) {
  BB_REQUIRE(N >= 1 && S >= 1 && C >= 1 && Lg >= 1 && policy >= 0 && policy <= 2, "nav_expert: N=%d S=%d C=%d Lg=%d policy=%d",
             N, S, C, Lg, policy);
  BB_REQUIRE(policy != 2 || (traj && traj_len && pred && Lt >= 1 && Lt + N <= NE_MAX_P - 1),
             "nav_expert: ndtw needs traj / traj_len / pred and Lt + N <= %d (Lt=%d N=%d)", NE_MAX_P - 1, Lt, N);
  BB_REQUIRE(policy != 0 || t >= 0, "nav_expert: imitation needs t >= 0 (t=%d)", t);
  if (B <= 0) return BB_OK;
  if (policy == 2)
    hipLaunchKernelGGL(ne_expert_kernel, dim3(B), dim3(64 * NE_WAVES), 0, stream, dist, pred, N, S, scan, cur, cand,
                       visited, ended, gt, gt_len, Lg, traj, traj_len, Lt, C, out);
  else
    hipLaunchKernelGGL(ne_expert_simple_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, dist, N, S, scan, cur, cand,
                       visited, ended, gt, gt_len, Lg, B, C, t, policy, out);
  BB_CHECK_LAUNCH("nav_expert");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (b) One navigation step's decision, one wave per sample (agent.py:523-534,559-612).
//   softmax of the row; live samples record p[0] as the stop score of their current node (dict semantics: a revisit
//   overwrites the score, the node keeps its first-insertion place);
//   a_t: teacher = target, argmax = first max of the logits, sample = inverse CDF of one uniform draw,
//   expl_sample = the same first max (of the probabilities in the reference: softmax is monotone), replaced with probability P(rand > expl_max_ratio) by a uniform pick
//   among masks (gmap_masks & ~visited);
//   stop: teacher / sample at the goal, else a_t == 0; also on ended, no_vp_left and the last step;
//   just-ended samples pick the first maximum of their stop scores in insertion order.
// Uniform draws: 24 bits of hash(salted(site_key(seed, t)) ^ (4 b + stream)); the salt is the step salt, so a replayed
// graph draws anew.
__global__ __launch_bounds__(64) void ne_action_kernel(
    const void* __restrict__ logits_, int bf16, int C, int feedback, int t, int max_len,
    const int64_t* __restrict__ targets, const int* __restrict__ cand, const int* __restrict__ cur_,
    const int* __restrict__ goal, uint8_t* __restrict__ ended, const uint8_t* __restrict__ no_vp_left,
    const uint8_t* __restrict__ masks, float* __restrict__ stop_scores, int* __restrict__ stop_order,
    int* __restrict__ n_stop, int N, float expl_max_ratio, uint32_t key, const uint32_t* __restrict__ salt,
    int64_t* __restrict__ a_out, int* __restrict__ node_out, uint8_t* __restrict__ just_ended,
    int* __restrict__ stop_node, float* __restrict__ entropy, float* __restrict__ rand_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t row = (size_t)b * C;
  auto ld = [&](int j) -> float {
    return bf16 ? bf16_to_f32(((const bf16_raw*)logits_)[row + j]) : ((const float*)logits_)[row + j];
  };
  // first max of the logits (value, then lowest index)
  float m = -INFINITY;
  int am = 0;
  for (int j = lane; j < C; j += 64) {
    const float x = ld(j);
    if (x > m) { m = x; am = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const int a2 = __shfl_xor(am, o, 64);
    if (m2 > m || (m2 == m && a2 < am)) { m = m2; am = a2; }
  }
  float s = 0.f;
  for (int j = lane; j < C; j += 64) s += __expf(ld(j) - m);
  s = wave_sum(s);
  const float inv = 1.f / s;
  // entropy -sum p log p (p = 0 terms contribute 0, as torch.distributions.Categorical)
  float h = 0.f;
  for (int j = lane; j < C; j += 64) {
    const float p = __expf(ld(j) - m) * inv;
    if (p > 0.f) h -= p * __logf(p);
  }
  h = wave_sum(h);
  if (lane != 0) return;

  const int cur = cur_[b];
  const bool was_ended = ended[b] != 0;
  int* order = stop_order + (size_t)b * N;
  float* sc = stop_scores + (size_t)b * N;
  if (!was_ended && (unsigned)cur < (unsigned)N) {
    const int n = n_stop[b];
    bool seen = false;
    for (int k = 0; k < n; ++k) seen |= order[k] == cur;
    if (!seen && n < N) { order[n] = cur; n_stop[b] = n + 1; }
    sc[cur] = __expf(ld(0) - m) * inv;
  }
  const uint32_t k0 = bb_salted(key, salt);
  const float u0 = (bb_hash32(k0 ^ (4u * b)) >> 8) * (1.f / 16777216.f);
  const float u1 = (bb_hash32(k0 ^ (4u * b + 1u)) >> 8) * (1.f / 16777216.f);
  int64_t a = 0;
  float r = 0.f;
  if (feedback == 0) {
    a = targets[b];
  } else if (feedback == 1) {
    a = am;
  } else if (feedback == 2) {
    r = u0;
    int pick = -1, lastpos = 0;
    float c = 0.f;
    for (int j = 0; j < C; ++j) {
      const float p = __expf(ld(j) - m) * inv;
      if (p > 0.f) lastpos = j;
      c += p;
      if (pick < 0 && u0 < c && p > 0.f) pick = j;
    }
    a = pick >= 0 ? pick : lastpos;
  } else {
    a = am;                        // nav_probs.max(1): the softmax is monotone, so the first max of the logits
    r = u0;
    if (u0 > expl_max_ratio) {
      const uint8_t* mk = masks + row;
      int cnt = 0;
      for (int j = 0; j < C; ++j) cnt += mk[j] != 0;
      if (cnt > 0) {
        int want = min((int)(u1 * cnt), cnt - 1);
        for (int j = 0; j < C; ++j)
          if (mk[j] && want-- == 0) { a = j; break; }
      }
    }
  }
  const bool at_goal = cur == goal[b];
  const bool stop = (feedback == 0 || feedback == 2) ? at_goal : a == 0;
  const bool end_now = stop || was_ended || (no_vp_left && no_vp_left[b]) || t == max_len - 1 || a < 0 || a >= C;
  const int node = end_now ? -1 : cand[row + a];
  a_out[b] = a;
  node_out[b] = node;
  just_ended[b] = end_now && !was_ended;
  int sn = -1;
  if (end_now && !was_ended) {
    float best = -INFINITY;
    for (int k = 0, n = n_stop[b]; k < n; ++k)
      if (sc[order[k]] > best) { best = sc[order[k]]; sn = order[k]; }
  }
  stop_node[b] = sn;
  // agent.py:615 ends every sample whose environment action is None: the stops above, and a live sample whose chosen
  // slot has no viewpoint (slot 0 away from the goal in teacher / sample mode) -- that one stays in place, without a
  // stop-node pick (just_ended = 0)
  if (node < 0) ended[b] = 1;
  entropy[b] = h;
  rand_out[b] = r;
}

BEVBERT_API int bevbert_nav_action(const void* logits, int dtype, int B, int C, int feedback, int t, int max_len,
                                   const int64_t* targets, const int* cand, const int* cur, const int* goal,
                                   uint8_t* ended, const uint8_t* no_vp_left, const uint8_t* masks, float* stop_scores,
                                   int* stop_order, int* n_stop, int N, float expl_max_ratio, uint32_t seed,
                                   int64_t* a_t, int* node, uint8_t* just_ended, int* stop_node, float* entropy,
                                   float* rand, hipStream_t stream) {
  BB_REQUIRE(C >= 1 && N >= 1 && feedback >= 0 && feedback <= 3, "nav_action: C=%d N=%d feedback=%d", C, N, feedback);
  BB_REQUIRE(dtype == BB_F32 || dtype == BB_BF16, "nav_action: dtype %d unsupported", dtype);
  BB_REQUIRE(cand && cur && goal && ended && stop_scores && stop_order && n_stop,
             "nav_action: cand / cur / goal / ended / stop tables are required%s", "");
  BB_REQUIRE(feedback != 0 || targets, "nav_action: teacher needs targets%s", "");
  BB_REQUIRE(feedback != 3 || masks, "nav_action: expl_sample needs masks%s", "");
  if (B <= 0) return BB_OK;
  hipLaunchKernelGGL(ne_action_kernel, dim3(B), dim3(64), 0, stream, logits, dtype == BB_BF16, C, feedback, t, max_len,
                     targets, cand, cur, goal, ended, no_vp_left, masks, stop_scores, stop_order, n_stop, N,
                     expl_max_ratio, bb_stream_key(bb_site_key(seed, (uint64_t)t), BB_STREAM_NAV), bb_step_salt(), a_t,
                     node, just_ended, stop_node, entropy, rand);
  BB_CHECK_LAUNCH("nav_action");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (e) CrossEntropyLoss(ignore_index, reduction='sum') of (B,C) logits.  Forward: one block, wave w takes rows w, w+4,
// ...; out = [lse (B) | per-row loss (B) | total]; the total is summed in row order by one thread.  Rows whose target
// is the ignore index, or outside [0, C), contribute 0.
template <typename T>
__global__ __launch_bounds__(256) void ne_ce_fwd_kernel(const T* __restrict__ x, const int64_t* __restrict__ target,
                                                        float* __restrict__ out, int B, int C, int ignore) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = w; r < B; r += 4) {
    const T* xr = x + (size_t)r * C;
    float m = -INFINITY;
    for (int j = lane; j < C; j += 64) m = fmaxf(m, io<T>::ld(xr + j));
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < C; j += 64) s += __expf(io<T>::ld(xr + j) - m);
    s = wave_sum(s);
    if (lane == 0) {
      const float lse = m + __logf(s);
      const int64_t tg = target[r];
      out[r] = lse;
      out[B + r] = (tg == ignore || tg < 0 || tg >= C) ? 0.f : lse - io<T>::ld(xr + tg);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int r = 0; r < B; ++r) tot += out[B + r];
    out[2 * B] = tot;
  }
}

template <typename T>
__global__ __launch_bounds__(64) void ne_ce_bwd_kernel(const T* __restrict__ x, const int64_t* __restrict__ target,
                                                       const float* __restrict__ lse, const float* __restrict__ dloss,
                                                       T* __restrict__ dx, int C, int ignore) {
  const int r = blockIdx.x;
  const int64_t tg = target[r];
  const bool skip = tg == ignore || tg < 0 || tg >= C;
  const float g = dloss[0], l = lse[r];
  for (int j = threadIdx.x; j < C; j += 64) {
    const size_t i = (size_t)r * C + j;
    io<T>::st(dx + i, skip ? 0.f : (__expf(io<T>::ld(x + i) - l) - (j == tg ? 1.f : 0.f)) * g);
  }
}

BEVBERT_API int bevbert_nav_ce_fwd(const void* logits, const int64_t* target, float* out, int B, int C, int ignore,
                                   int dtype, hipStream_t stream) {
  BB_REQUIRE(C >= 1 && B >= 0, "nav_ce: B=%d C=%d", B, C);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ne_ce_fwd_kernel<T>, dim3(1), dim3(256), 0, stream, (const T*)logits, target, out, B, C, ignore);
  });
  if (!type_ok) return bb_dtype_unsupported("nav_ce", dtype);
  BB_CHECK_LAUNCH("nav_ce_fwd");
  return BB_OK;
}

BEVBERT_API int bevbert_nav_ce_bwd(const void* logits, const int64_t* target, const float* out, const float* dloss,
                                   void* dlogits, int B, int C, int ignore, int dtype, hipStream_t stream) {
  BB_REQUIRE(C >= 1, "nav_ce: C=%d", C);
  if (B <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ne_ce_bwd_kernel<T>, dim3(B), dim3(64), 0, stream, (const T*)logits, target, out, dloss, (T*)dlogits, C,
                       ignore);
  });
  if (!type_ok) return bb_dtype_unsupported("nav_ce", dtype);
  BB_CHECK_LAUNCH("nav_ce_bwd");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (d) _eval_item (env.py:331-357) per finished trajectory, one wave per sample, f64: lane 0 walks the paths in the
// reference's order (sums left to right), the wave runs the DTW.  Then one thread forms eval_metrics' means in
// sample order.  items row: nav_error, oracle_error, action_steps, trajectory_steps, trajectory_lengths, success, spl,
// oracle_success, DTW, nDTW, SDTW, CLS.
#define NE_NM 12
__global__ __launch_bounds__(64) void ne_metrics_kernel(const double* __restrict__ dist, int N, int S,
                                                        const int* __restrict__ scan, const int* __restrict__ path,
                                                        const int* __restrict__ path_len, int Lp,
                                                        const int* __restrict__ action_steps, const int* __restrict__ gt,
                                                        const int* __restrict__ gt_len, int Lg, double margin,
                                                        double* __restrict__ items) {
  __shared__ double s_edge[NE_MAX_P];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int sc = scan[b];
  const int P = min(max(path_len[b], 1), Lp), G = min(max(gt_len[b], 1), Lg);
  const int* p = path + (size_t)b * Lp;
  const int* g = gt + (size_t)b * Lg;
  double* o = items + (size_t)b * NE_NM;
  if ((unsigned)sc >= (unsigned)S) {                   // no such scan: every field NaN (the expert answers -100)
    if (lane < NE_NM) o[lane] = __builtin_nan("");
    return;
  }
  const double* d = dist + (size_t)sc * N * N;
  const double dtw = ne_dtw(d, N, p, P, g, G, s_edge);
  if (lane != 0) return;
  const int goal = g[G - 1];
  int near = p[0];
  double near_d = ne_d(d, N, near, goal);
  for (int i = 0; i < P; ++i) {
    const double x = ne_d(d, N, p[i], goal);
    if (x < near_d) { near = p[i]; near_d = x; }
  }
  const double nav_error = ne_d(d, N, p[P - 1], goal);
  const double oracle_error = ne_d(d, N, near, goal);
  const double tlen = ne_path_length(d, N, p, P), glen = ne_path_length(d, N, g, G);
  const double success = nav_error < margin ? 1.0 : 0.0;
  const double spl = success * glen / fmax(fmax(tlen, glen), 0.01);
  const double ndtw = exp(-dtw / (margin * G));
  // cal_cls: coverage = mean over u in gt of exp(-min_v d[u][v] / margin); expected = coverage * len(gt)
  double cov = 0.0;
  for (int j = 0; j < G; ++j) {
    double mn = NE_INF;
    for (int i = 0; i < P; ++i) mn = fmin(mn, ne_d(d, N, g[j], p[i]));
    cov += exp(-mn / margin);
  }
  cov /= G;
  const double expected = cov * glen;
  const double score = expected / (expected + fabs(expected - tlen));
  o[0] = nav_error;
  o[1] = oracle_error;
  o[2] = action_steps[b];
  o[3] = P - 1;
  o[4] = tlen;
  o[5] = success;
  o[6] = spl;
  o[7] = oracle_error < margin ? 1.0 : 0.0;
  o[8] = dtw;
  o[9] = ndtw;
  o[10] = success * ndtw;
  o[11] = cov * score;
}

// eval_metrics' averaged dict: (item column, scale) per key, means summed in sample order
__global__ __launch_bounds__(64) void ne_metrics_mean_kernel(const double* __restrict__ items, int B,
                                                             double* __restrict__ avg) {
  const int col[11] = {2, 3, 4, 0, 1, 5, 7, 6, 9, 10, 11};
  const int k = threadIdx.x;
  if (k >= 11) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += items[(size_t)b * NE_NM + col[k]];
  avg[k] = s / B * (k >= 5 ? 100.0 : 1.0);
}

BEVBERT_API int bevbert_nav_metrics(const double* dist, int N, int S, const int* scan, const int* path,
                                    const int* path_len, int Lp, const int* action_steps, const int* gt,
                                    const int* gt_len, int Lg, int B, double margin, double* items, double* avg,
                                    hipStream_t stream) {
  BB_REQUIRE(N >= 1 && S >= 1 && Lp >= 1 && Lg >= 1 && Lp < NE_MAX_P, "nav_metrics: N=%d S=%d Lp=%d Lg=%d (Lp < %d)",
             N, S, Lp, Lg, NE_MAX_P);
  if (B <= 0) return BB_OK;
  hipLaunchKernelGGL(ne_metrics_kernel, dim3(B), dim3(64), 0, stream, dist, N, S, scan, path, path_len, Lp, action_steps,
                     gt, gt_len, Lg, margin, items);
  BB_CHECK_LAUNCH("nav_metrics");
  if (avg) {
    hipLaunchKernelGGL(ne_metrics_mean_kernel, dim3(1), dim3(64), 0, stream, items, B, avg);
    BB_CHECK_LAUNCH("nav_metrics_mean");
  }
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (c) Trajectory record: traj[b] += FloydGraph.path(from[b], to[b]) (graph_utils.py:85-93, DeviceGraphMap.path) for the
// live samples, in scan indices.  The agent map's next-hop table point (B,Nm,Nm) (-1 = direct edge, the layout of
// bevbert_gm_state.point) is expanded with an explicit stack instead of recursion: pop (i, j); k = point[i][j];
// k < 0 -> emit j, else push (k, j) then (i, k).  node_scan (B,Nm) maps a map node (registration order) to its scan
// index.  One lane per sample.  A full record, a stack deeper than NE_TR_STACK or more than 4 Nm expansions (a table
// that is not a Floyd next-hop table) set *overflow; the record then stops at its capacity.
#define NE_TR_STACK 128
__global__ __launch_bounds__(64) void ne_traj_kernel(const int* __restrict__ point, int Nm,
                                                     const int* __restrict__ node_scan, const int* __restrict__ from,
                                                     const int* __restrict__ to, const uint8_t* __restrict__ live,
                                                     int* __restrict__ traj, int* __restrict__ traj_len, int Lt,
                                                     int* __restrict__ n_seg, int* __restrict__ overflow, int B) {
  __shared__ int s_stack[64][NE_TR_STACK];
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B || !live[b]) return;
  const int x = from[b], y = to[b];
  n_seg[b] += 1;
  if ((unsigned)x >= (unsigned)Nm || (unsigned)y >= (unsigned)Nm || x == y) return;   // path(x, x) = []
  const int* P = point + (size_t)b * Nm * Nm;
  const int* ns = node_scan + (size_t)b * Nm;
  int* st = s_stack[threadIdx.x];
  int* tr = traj + (size_t)b * Lt;
  int len = traj_len[b], sp = 0, steps = 0, bad = 0;
  st[sp++] = x * Nm + y;
  while (sp > 0) {
    const int e = st[--sp], i = e / Nm, j = e - i * Nm;
    const int k = P[(size_t)i * Nm + j];
    if (++steps > 4 * Nm || k >= Nm) { bad = 1; break; }
    if (k < 0) {
      if (len < Lt) tr[len++] = ns[j];
      else { bad = 1; break; }
    } else {
      if (sp + 2 > NE_TR_STACK) { bad = 1; break; }
      st[sp++] = k * Nm + j;
      st[sp++] = i * Nm + k;
    }
  }
  traj_len[b] = len;
  if (bad) *overflow = 1;
}

BEVBERT_API int bevbert_nav_traj_append(const int* point, int Nm, const int* node_scan, const int* from, const int* to,
                                        const uint8_t* live, int* traj, int* traj_len, int Lt, int* n_seg,
                                        int* overflow, int B, hipStream_t stream) {
  BB_REQUIRE(Nm >= 1 && Lt >= 1 && (int64_t)Nm * Nm < (1ll << 31), "nav_traj_append: Nm=%d Lt=%d", Nm, Lt);
  BB_REQUIRE(point && node_scan && from && to && live && traj && traj_len && n_seg && overflow,
             "nav_traj_append: null pointer%s", "");
  if (B <= 0) return BB_OK;
  hipLaunchKernelGGL(ne_traj_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, point, Nm, node_scan, from, to, live, traj,
                     traj_len, Lt, n_seg, overflow, B);
  BB_CHECK_LAUNCH("nav_traj_append");
  return BB_OK;
}
