// Ghost-node map of the continuous-environment (CE) agent on the device (bevbert_ce/vlnce_baselines:
// models/graph_utils.py:14-75,142-372 GraphMap and its helpers; ss_trainer_BEV.py:317-345 _teacher_action_new,
// :465-475 _discretize_polar_relpos, :477-532 the candidate half of _nav_bev_variable, :534-611 _nav_gmap_variable,
// :1083-1084 the stop-score record, :1110-1179 the action block).  B maps live in dense arrays of fixed capacity
// (bevbert_ce_state): node k of a map is the reference's str(k), ghost g its 'g' + str(g), so there is no host
// dictionary.  Every entry is launch-only with fixed output shapes; no atomics; plain stores only.
//   (a) bevbert_ce_update       identify_node + estimate_cand_pos + update_graph (+ the all-pairs Dijkstra)
//   (b) bevbert_ce_nav_vars     _nav_gmap_variable + get_pos_fts + front_to_ghost_dist
//   (c) bevbert_ce_bev_cands    get_neighbors + _discretize_polar_relpos + the SAP fusion indices
//   (d) bevbert_ce_stop_scores / bevbert_ce_teacher / bevbert_ce_act
//   (e) bevbert_ce_remember / bevbert_ce_bev_select   update_node_pc's store, gather_node_pc's node choice
// Ids in outputs: -1 = [stop] / none, k < N = node k, N + g = ghost g.
#include "common.h"      // bevbert_ce_state: include/bevbert_hip.h

#define CE_MAX_N 64                 // one lane per Dijkstra source, the settled set is a 64-bit mask
#define CE_MAX_G 512                // 1 + N + Gh rows of the padded global map held in LDS
#define CE_MAX_C 16                 // candidates of one step
#define CE_MAX_DIST 30.0            // graph_utils.py:10-11
#define CE_MAX_STEP 10.0
#define CE_TWO_PI 6.283185307179586476925286766559
#define CE_PI 3.14159265358979323846

__device__ __forceinline__ double ce_sq(double x) { return x * x; }
__device__ __forceinline__ double ce_dist3(const double* a, const double* b) {      // calc_position_distance
  return sqrt(ce_sq(b[0] - a[0]) + ce_sq(b[1] - a[1]) + ce_sq(b[2] - a[2]));
}

// calculate_vp_rel_pos_fts(a, b, base_heading, 0, to_clock=True) AS WRITTEN in the CE fork: arcsin(-dx / xz), the
// b[2] > a[2] branch (the discrete fork tests b[1] < a[1] on arcsin(dx / xy)), to_clock (2 pi - heading) and the
// elevation taken from dz (not dy) over the xyz distance.
__device__ __forceinline__ void ce_rel_pos(const double* a, const double* b, double base_heading, double& heading,
                                           double& elevation, double& xz_dist, double& xyz_dist) {
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  xz_dist = fmax(sqrt(dx * dx + dz * dz), 1e-8);
  xyz_dist = fmax(sqrt(dx * dx + dy * dy + dz * dz), 1e-8);
  double h = asin(-dx / xz_dist);
  if (b[2] > a[2]) h = CE_PI - h;
  h -= base_heading;
  heading = CE_TWO_PI - h;
  elevation = asin(dz / xyz_dist);
}

// front_to_ghost_dist: the nearest front of ghost g (strict <, first wins; duplicates in the list change nothing),
// measured to the AUGMENTED ghost position.
__device__ __forceinline__ int ce_front(const bevbert_ce_state& st, int b, int g, double& min_dis) {
  const size_t gi = (size_t)b * st.Gh + g;
  const int* fronts = st.g_fronts + gi * st.P;
  const double* aug = st.g_aug + gi * 3;
  const int n = st.g_npos[gi];
  min_dis = 10000.0;
  int front = -1;
  for (int i = 0; i < n; ++i) {
    const double d = ce_dist3(st.node_pos + ((size_t)b * st.N + fronts[i]) * 3, aug);
    if (d < min_dis) { min_dis = d; front = fronts[i]; }
  }
  return front;
}

// get_pos_fts for one id seen from node cur at (pos, heading): 7 floats (sin / cos heading, sin / cos elevation in
// float32 of the float32-rounded angles, as get_angle_fts gets them; line distance / 30, shortest distance / 30,
// shortest step / 10 rounded from float64).
__device__ __forceinline__ void ce_pos_fts(const bevbert_ce_state& st, int b, int cur, const double* pos, double heading,
                                           int id, float* out) {
  if (id < 0) {                                       // [stop]: angles (0, 0), distances 0
    out[0] = 0.f; out[1] = 1.f; out[2] = 0.f; out[3] = 1.f; out[4] = 0.f; out[5] = 0.f; out[6] = 0.f;
    return;
  }
  double h, e, xz, xyz, sd, ss;
  const double* drow = st.dist + ((size_t)b * st.N + cur) * st.N;
  const int* hrow = st.hops + ((size_t)b * st.N + cur) * st.N;
  if (id >= st.N) {
    const int g = id - st.N;
    ce_rel_pos(pos, st.g_aug + ((size_t)b * st.Gh + g) * 3, heading, h, e, xz, xyz);
    double fd;
    const int f = ce_front(st, b, g, fd);
    sd = f >= 0 ? drow[f] + fd : HUGE_VAL;                 // (a live ghost always has a front)
    ss = (double)((f >= 0 ? hrow[f] : 0) + 1);
  } else {
    ce_rel_pos(pos, st.node_pos + ((size_t)b * st.N + id) * 3, heading, h, e, xz, xyz);
    sd = drow[id];
    ss = (double)hrow[id];
  }
  const double hf = (double)(float)h, ef = (double)(float)e;
  out[0] = (float)sin(hf); out[1] = (float)cos(hf); out[2] = (float)sin(ef); out[3] = (float)cos(ef);
  out[4] = (float)(xyz / CE_MAX_DIST); out[5] = (float)(sd / CE_MAX_DIST); out[6] = (float)(ss / CE_MAX_STEP);
}

// ----------------------------------------------------------------------------------------------------------------
// (a) update.  One workgroup per map.  Thread 0 walks the candidates in order (every decision depends on the one
// before it), all threads copy / add the embeddings, one thread per ghost redraws the training noise, one lane per
// source runs Dijkstra.  Reference behaviours kept, by name:
//   U1  a new node every step: identify_node names the node str(len(node_pos)), there is no re-localization of cur;
//   U2  the prev_vp edge: weight = distance(prev node, cur) in float64, none on the first step of an episode;
//   U3  _localize over the nodes in insertion order with strict < for the minimum (the first of equal distances
//       wins) and acceptance by min_dis <= loc_noise (min_dis > loc_noise rejects);
//   U4  the current node is in node_pos before the candidates are localized, so a candidate within loc_noise of the
//       agent itself is "localized" to cur and adds the zero-length self edge (cur, cur);
//   U5  ghosts: with merge_ghost a candidate is localized among the MEAN positions of the live ghosts in creation
//       order (same rule as U3) and merges, else (or with merge_ghost off: always) it creates ghost g = ghost_cnt++;
//   U6  the ghost mean is np.mean(list, axis=0): the positions summed one after the other from the first, then one
//       division by the count;
//   U7  embedding sum and count: sum = sum + cand_embeds in candidate order, count += 1;
//   U8  fronts: cur is appended on every merge, so two candidates of one step that merge into the same ghost leave
//       cur in its fronts twice;
//   U9  ghost_aug: the augmented position of EVERY live ghost is redrawn at every update: mean + N(0, (a, 0, a))
//       clipped to +-a; the y component gets no noise.  Draws are a pure function of (seed, step salt, step_id, map,
//       ghost id): two 24-bit hashes -> Box-Muller, one normal each for x and z;
//   U10 all-pairs Dijkstra, one lane per source: the closest unsettled node with strict < (the lowest index among
//       equals), relaxation nd = dist[u] + w accepted by strict nd < dist[v], so every distance is the float64 sum of
//       the edge weights in path order from the source -- the order networkx accumulates them in.  hops counts the
//       nodes on the path, both end points included (len(shortest_path[x][y])); pred is the predecessor table the
//       action kernel walks for back_path.
__global__ __launch_bounds__(256) void ce_update_kernel(
    bevbert_ce_state st, const double* __restrict__ pose, const uint8_t* __restrict__ live,
    const int* __restrict__ step_id_p, const int* __restrict__ cand_count, const float* __restrict__ cand_angles,
    const float* __restrict__ cand_distances, int C, const void* __restrict__ avg_pano, const void* __restrict__ pano,
    const int64_t* __restrict__ nav_types, int L, double loc_noise, double aug, uint32_t key,
    const uint32_t* __restrict__ salt, int* __restrict__ cand_slot) {
  __shared__ int s_ok, s_cur, s_k;
  __shared__ int s_row[CE_MAX_C], s_ghost[CE_MAX_C], s_fresh[CE_MAX_C];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = st.N, Gh = st.Gh, P = st.P, H = st.H;
  if (!live[b]) {
    if (tid < C) cand_slot[b * C + tid] = -1;
    return;
  }
  double* npos = st.node_pos + (size_t)b * N * 3;
  double* W = st.edge_w + (size_t)b * N * N;
  if (tid == 0) {
    const int n = st.n_nodes[b];
    s_ok = n < N;
    s_k = 0;
    if (n >= N) {
      *st.overflow = 1;                                          // node capacity: the step is refused, not truncated
      for (int j = 0; j < C; ++j) cand_slot[b * C + j] = -1;
    } else {
      const int cur = n;                                         // U1
      const double* p = pose + (size_t)b * 4;
      const double heading = p[3];
      const int prev = st.prev_vp[b];
      if (prev >= 0) {                                           // U2
        const double w = ce_dist3(npos + prev * 3, p);
        W[prev * N + cur] = w;
        W[cur * N + prev] = w;
      }
      npos[cur * 3 + 0] = p[0]; npos[cur * 3 + 1] = p[1]; npos[cur * 3 + 2] = p[2];
      st.node_step[b * N + cur] = *step_id_p;
      st.n_nodes[b] = n + 1;
      st.cur_vp[b] = cur;
      s_cur = cur;
      int k = cand_count[b];
      k = k < 0 ? 0 : (k > C ? C : k);
      s_k = k;
      int row = 0, gcnt = st.g_cnt[b];
      const bool merge = st.merge[b] != 0;
      for (int j = 0; j < C; ++j) {
        if (j >= k) { cand_slot[b * C + j] = -1; continue; }
        while (row < L && nav_types[(size_t)b * L + row] != 1) ++row;       // cand_embeds = pano_embeds[nav_types == 1]
        s_row[j] = row < L ? row : -1;
        ++row;
        if (s_row[j] < 0) {                                      // fewer nav_types == 1 rows than candidates: refused, flagged
          *st.overflow = 1;
          s_ghost[j] = -1;
          cand_slot[b * C + j] = -1;
          continue;
        }
        // estimate_cand_pos: (heading + ang) % 2 pi with Python's sign convention
        double a = heading + (double)cand_angles[b * C + j];
        a = fmod(a, CE_TWO_PI);
        if (a < 0.0) a += CE_TWO_PI;
        const double d = (double)cand_distances[b * C + j];
        const double cp[3] = {p[0] - d * sin(a), p[1], p[2] - d * cos(a)};
        double min_dis = 10000.0;                                // U3, U4: nodes 0 .. cur, cur included
        int min_vp = -1;
        for (int v = 0; v <= cur; ++v) {
          const double dis = ce_dist3(npos + v * 3, cp);
          if (dis < min_dis) { min_dis = dis; min_vp = v; }
        }
        s_ghost[j] = -1;
        if (min_vp >= 0 && !(min_dis > loc_noise)) {
          const double w = ce_dist3(p, npos + min_vp * 3);
          W[cur * N + min_vp] = w;
          W[min_vp * N + cur] = w;
          cand_slot[b * C + j] = min_vp;
          continue;
        }
        int g = -1;
        if (merge) {                                             // U5
          min_dis = 10000.0;
          for (int q = 0; q < gcnt; ++q) {
            if (!st.g_alive[(size_t)b * Gh + q]) continue;
            const double dis = ce_dist3(st.g_mean + ((size_t)b * Gh + q) * 3, cp);
            if (dis < min_dis) { min_dis = dis; g = q; }
          }
          if (min_dis > loc_noise) g = -1;
        }
        const bool fresh = g < 0;
        if (fresh) {
          if (gcnt >= Gh) { *st.overflow = 1; cand_slot[b * C + j] = -1; s_row[j] = -1; continue; }
          g = gcnt++;
        }
        const size_t gi = (size_t)b * Gh + g;
        const int np_ = fresh ? 0 : st.g_npos[gi];
        if (np_ >= P) { *st.overflow = 1; cand_slot[b * C + j] = -1; s_row[j] = -1; continue; }
        double* gp = st.g_pos + gi * P * 3;
        gp[np_ * 3 + 0] = cp[0]; gp[np_ * 3 + 1] = cp[1]; gp[np_ * 3 + 2] = cp[2];
        st.g_fronts[gi * P + np_] = cur;                         // U8
        st.g_npos[gi] = np_ + 1;
        st.g_alive[gi] = 1;
        double m0 = gp[0], m1 = gp[1], m2 = gp[2];               // U6
        for (int i = 1; i <= np_; ++i) { m0 += gp[i * 3]; m1 += gp[i * 3 + 1]; m2 += gp[i * 3 + 2]; }
        if (np_ > 0) { const double cnt = (double)(np_ + 1); m0 /= cnt; m1 /= cnt; m2 /= cnt; }
        st.g_mean[gi * 3 + 0] = m0; st.g_mean[gi * 3 + 1] = m1; st.g_mean[gi * 3 + 2] = m2;
        s_ghost[j] = g;
        s_fresh[j] = fresh;
        cand_slot[b * C + j] = N + g;
      }
      st.g_cnt[b] = gcnt;
    }
  }
  __syncthreads();
  if (!s_ok) return;
  const int cur = s_cur, k = s_k;
  // U7 + the node embedding (cur_embeds = avg_pano_embeds[i]); candidates in order: two may feed one ghost
  if (st.dtype == BB_F32) {
    const float* avg = (const float*)avg_pano + (size_t)b * H;
    float* ne = (float*)st.node_embeds + ((size_t)b * N + cur) * H;
    for (int h = tid; h < H; h += 256) ne[h] = avg[h];
  } else {
    const bf16_raw* avg = (const bf16_raw*)avg_pano + (size_t)b * H;
    bf16_raw* ne = (bf16_raw*)st.node_embeds + ((size_t)b * N + cur) * H;
    for (int h = tid; h < H; h += 256) ne[h] = avg[h];
  }
  for (int j = 0; j < k; ++j) {
    const int g = s_ghost[j], row = s_row[j];
    if (g < 0 || row < 0) continue;
    float* sum = st.g_sum + ((size_t)b * Gh + g) * H;
    const size_t off = ((size_t)b * L + row) * H;
    for (int h = tid; h < H; h += 256) {
      const float x = st.dtype == BB_F32 ? ((const float*)pano)[off + h] : bf16_to_f32(((const bf16_raw*)pano)[off + h]);
      sum[h] = s_fresh[j] ? x : sum[h] + x;                    // a thread only ever touches its own h: no barrier needed
    }
  }
  // U9
  const int gcnt = st.g_cnt[b];
  const uint32_t kb = bb_hash32(bb_hash32(bb_salted(key, salt) ^ (uint32_t)*step_id_p) ^ (uint32_t)b);
  for (int g = tid; g < gcnt; g += 256) {
    const size_t gi = (size_t)b * Gh + g;
    if (!st.g_alive[gi]) continue;
    double nx = 0.0, nz = 0.0;
    if (aug != 0.0) {
      const uint32_t kg = bb_hash32(kb ^ (uint32_t)g);
      const double u1 = ((double)(bb_hash32(kg ^ 1u) >> 8) + 1.0) * (1.0 / 16777216.0);       // (0, 1]
      const double u2 = (double)(bb_hash32(kg ^ 2u) >> 8) * (1.0 / 16777216.0);               // [0, 1)
      const double r = sqrt(-2.0 * log(u1)) * aug;
      nx = fmin(fmax(r * cos(CE_TWO_PI * u2), -aug), aug);
      nz = fmin(fmax(r * sin(CE_TWO_PI * u2), -aug), aug);
    }
    st.g_aug[gi * 3 + 0] = st.g_mean[gi * 3 + 0] + nx;
    st.g_aug[gi * 3 + 1] = st.g_mean[gi * 3 + 1] + 0.0;
    st.g_aug[gi * 3 + 2] = st.g_mean[gi * 3 + 2] + nz;
  }
  // U10
  if (tid < N) {
    const int n = cur + 1, s = tid;
    double* d = st.dist + ((size_t)b * N + s) * N;
    int* hp = st.hops + ((size_t)b * N + s) * N;
    int* pr = st.pred + ((size_t)b * N + s) * N;
    for (int v = 0; v < N; ++v) { d[v] = HUGE_VAL; hp[v] = 0; pr[v] = -1; }
    if (s < n) {
      d[s] = 0.0;
      hp[s] = 1;
      uint64_t done = 0;
      for (int it = 0; it < n; ++it) {
        int u = -1;
        double best = HUGE_VAL;
        for (int v = 0; v < n; ++v)
          if (!((done >> v) & 1) && d[v] < best) { best = d[v]; u = v; }
        if (u < 0) break;
        done |= (uint64_t)1 << u;
        for (int v = 0; v < n; ++v) {
          const double w = W[u * N + v];
          if (w >= 0.0 && !((done >> v) & 1)) {
            const double nd = best + w;
            if (nd < d[v]) { d[v] = nd; hp[v] = hp[u] + 1; pr[v] = u; }
          }
        }
      }
    }
  }
}

BEVBERT_API int bevbert_ce_update(const bevbert_ce_state* st, const double* pose, const uint8_t* live, const int* step_id,
                                  const int* cand_count, const float* cand_angles, const float* cand_distances, int C,
                                  const void* avg_pano, const void* pano, const int64_t* nav_types, int L,
                                  double loc_noise, double ghost_aug, uint32_t seed, int* cand_slot, hipStream_t stream) {
  BB_REQUIRE(st && st->B >= 0 && st->N >= 1 && st->N <= CE_MAX_N && st->Gh >= 1 && 1 + st->N + st->Gh <= CE_MAX_G &&
                 st->P >= 1 && st->H >= 1,
             "ce_update: B=%d N=%d (<= 64) Gh=%d (1 + N + Gh <= 512) P=%d H=%d", st ? st->B : -1, st ? st->N : -1,
             st ? st->Gh : -1, st ? st->P : -1, st ? st->H : -1);
  BB_REQUIRE(st->dtype == BB_F32 || st->dtype == BB_BF16, "ce_update: dtype %d unsupported", st->dtype);
  BB_REQUIRE(C >= 1 && C <= CE_MAX_C && L >= 1, "ce_update: C=%d (1..16) L=%d", C, L);
  BB_REQUIRE(ghost_aug >= 0.0, "ce_update: ghost_aug %f < 0", ghost_aug);
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(pose && live && step_id && cand_count && cand_angles && cand_distances && avg_pano && pano && nav_types &&
                 cand_slot, "ce_update: null tensor%s", "");
  hipLaunchKernelGGL(ce_update_kernel, dim3(st->B), dim3(256), 0, stream, *st, pose, live, step_id, cand_count,
                     cand_angles, cand_distances, C, avg_pano, pano, nav_types, L, loc_noise, ghost_aug,
                     bb_stream_key(bb_hash32(seed ^ 0x9e3779b9u), BB_STREAM_GHOST), bb_step_salt(), cand_slot);
  BB_CHECK_LAUNCH("ce_update");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (b) navigation variables.  One workgroup per map; the listing ([stop], nodes in creation order, live ghosts in
// creation order) and every listed ghost's nearest front sit in LDS.  Rows past the listing are padding (ids -1, zeros).
__global__ __launch_bounds__(256) void ce_nav_vars_kernel(
    bevbert_ce_state st, const double* __restrict__ pose, const uint8_t* __restrict__ live, int G,
    int64_t* __restrict__ gmap_ids, int64_t* __restrict__ step_ids, uint8_t* __restrict__ visited,
    uint8_t* __restrict__ masks, void* __restrict__ img_fts, float* __restrict__ pos_fts, float* __restrict__ pair,
    uint8_t* __restrict__ no_vp_left) {
  __shared__ int ids[CE_MAX_G], front[CE_MAX_G];
  __shared__ double fdis[CE_MAX_G];
  __shared__ int s_n;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = st.N, Gh = st.Gh, H = st.H;
  const bool on = live[b] != 0;
  const int nn = on ? st.n_nodes[b] : 0, cur = st.cur_vp[b];
  if (tid == 0) {
    int n = 0;
    if (on) {
      ids[n++] = -1;
      for (int k = 0; k < nn; ++k) ids[n++] = k;
      const int gcnt = st.g_cnt[b];
      for (int g = 0; g < gcnt; ++g)
        if (st.g_alive[(size_t)b * Gh + g]) ids[n++] = N + g;
      no_vp_left[b] = n == 1 + nn;
    } else {
      no_vp_left[b] = 0;
    }
    s_n = n;
  }
  __syncthreads();
  const int n = s_n;
  const double* p = pose + (size_t)b * 4;
  for (int j = tid; j < G; j += 256) {
    const size_t o = (size_t)b * G + j;
    const int id = j < n ? ids[j] : -1;
    gmap_ids[o] = id;
    step_ids[o] = (j < n && id >= 0 && id < N) ? st.node_step[b * N + id] : 0;
    visited[o] = j < n && id >= 0 && id < N;
    masks[o] = j < n;
    float f[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    front[j] = -1;
    if (j < n) {
      ce_pos_fts(st, b, cur, p, p[3], id, f);
      if (id >= N) {
        const int f = ce_front(st, b, id - N, fdis[j]);
        front[j] = f >= 0 ? f : 0;
      }
    }
    for (int c = 0; c < 7; ++c) pos_fts[o * 7 + c] = f[c];
  }
  __syncthreads();
  // gmap_pair_dists: the reference fills (j, k) and (k, j) from the pair with j < k, and dist[x][y] is summed from x --
  // the mirrored entry must read the same table element, not its transpose
  const double* D = st.dist + (size_t)b * N * N;
  for (int e = tid; e < G * G; e += 256) {
    int j = e / G, k = e - j * G;
    if (j > k) { const int t = j; j = k; k = t; }
    float v = 0.f;
    if (j >= 1 && j != k && k < n) {
      const int a = ids[j], c = ids[k];
      double d;
      if (c < N) d = D[a * N + c];                               // node, node
      else if (a < N) d = D[a * N + front[k]] + fdis[k];         // node, ghost
      else d = fdis[j] + D[front[j] * N + front[k]] + fdis[k];   // ghost, ghost
      v = (float)(d / CE_MAX_DIST);
    }
    pair[(size_t)b * G * G + e] = v;
  }
  // gmap_img_fts: row 0 and padding 0, nodes their stored embedding, ghosts sum / count
  for (int e = tid; e < G * H; e += 256) {
    const int j = e / H, h = e - j * H;
    float v = 0.f;
    if (j >= 1 && j < n) {
      const int id = ids[j];
      if (id < N) {
        const size_t o = ((size_t)b * N + id) * H + h;
        v = st.dtype == BB_F32 ? ((const float*)st.node_embeds)[o] : bf16_to_f32(((const bf16_raw*)st.node_embeds)[o]);
      } else {
        const size_t gi = (size_t)b * Gh + (id - N);
        v = st.g_sum[gi * H + h] / (float)st.g_npos[gi];
      }
    }
    const size_t o = (size_t)b * G * H + e;
    if (st.dtype == BB_F32) ((float*)img_fts)[o] = v;
    else ((bf16_raw*)img_fts)[o] = f32_to_bf16(v);
  }
}

BEVBERT_API int bevbert_ce_nav_vars(const bevbert_ce_state* st, const double* pose, const uint8_t* live,
                                    int64_t* gmap_ids, int64_t* step_ids, uint8_t* visited, uint8_t* masks,
                                    void* img_fts, float* pos_fts, float* pair_dists, uint8_t* no_vp_left,
                                    hipStream_t stream) {
  BB_REQUIRE(st && st->N >= 1 && st->N <= CE_MAX_N && st->Gh >= 1 && 1 + st->N + st->Gh <= CE_MAX_G,
             "ce_nav_vars: N=%d (<= 64) Gh=%d (1 + N + Gh <= 512)", st ? st->N : -1, st ? st->Gh : -1);
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(pose && live && gmap_ids && step_ids && visited && masks && img_fts && pos_fts && pair_dists && no_vp_left,
             "ce_nav_vars: null tensor%s", "");
  hipLaunchKernelGGL(ce_nav_vars_kernel, dim3(st->B), dim3(256), 0, stream, *st, pose, live, 1 + st->N + st->Gh, gmap_ids,
                     step_ids, visited, masks, img_fts, pos_fts, pair_dists, no_vp_left);
  BB_CHECK_LAUNCH("ce_nav_vars");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (c) BEV candidates.  get_neighbors: [current], the nodes one hop away (len(shortest_path) == 2) in creation order,
// then the live ghosts whose fronts contain the current node, in creation order; (heading, xz distance) rounded to
// float32 as the reference's np.array(..., dtype=np.float32) rows, then _discretize_polar_relpos in float64: rint is
// round-half-to-even like numpy's round, clamp to [0, dim - 1].  One lane per map: a few dozen short steps.
__global__ __launch_bounds__(64) void ce_bev_cands_kernel(
    bevbert_ce_state st, const double* __restrict__ pose, const uint8_t* __restrict__ live, int dim, double res, int K,
    int G, uint8_t* __restrict__ nav_masks, int64_t* __restrict__ cand_idxs, int64_t* __restrict__ cand_ids,
    int* __restrict__ cand_n, float* __restrict__ gpos_fts, int64_t* __restrict__ src, uint8_t* __restrict__ vis_c) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = st.N, Gh = st.Gh, cells = dim * dim;
  for (int c = tid; c < cells; c += 64) nav_masks[(size_t)b * cells + c] = 0;
  for (int j = tid; j < K; j += 64) {
    cand_idxs[(size_t)b * K + j] = 0;
    cand_ids[(size_t)b * K + j] = -1;
    vis_c[(size_t)b * K + j] = 0;
  }
  for (int j = tid; j < G; j += 64) src[(size_t)b * G + j] = j == 0 ? 0 : K + 1;      // K + 1: the zero slot
  __syncthreads();
  if (tid != 0) return;
  if (!live[b]) {
    cand_n[b] = 0;
    for (int c = 0; c < 7; ++c) gpos_fts[b * 7 + c] = 0.f;
    return;
  }
  const double* p = pose + (size_t)b * 4;
  const int cur = st.cur_vp[b], nn = st.n_nodes[b], gcnt = st.g_cnt[b];
  const int ctr = (dim - 1) / 2;
  int n = 0;
  cand_idxs[(size_t)b * K] = ctr * dim + ctr;                    // relpos (0, 0)
  nav_masks[(size_t)b * cells + ctr * dim + ctr] = 1;
  n = 1;
  const int* hrow = st.hops + ((size_t)b * N + cur) * N;
  for (int pass = 0; pass < 2; ++pass) {
    const int cnt = pass == 0 ? nn : gcnt;
    for (int i = 0; i < cnt; ++i) {
      const double* q;
      if (pass == 0) {
        if (hrow[i] != 2) continue;
        q = st.node_pos + ((size_t)b * N + i) * 3;
      } else {
        const size_t gi = (size_t)b * Gh + i;
        if (!st.g_alive[gi]) continue;
        bool has = false;
        for (int f = 0; f < st.g_npos[gi]; ++f) has |= st.g_fronts[gi * st.P + f] == cur;
        if (!has) continue;
        q = st.g_aug + gi * 3;
      }
      if (n >= K) { *st.overflow = 1; continue; }
      double h, e, xz, xyz;
      ce_rel_pos(p, q, p[3], h, e, xz, xyz);
      const double hf = (double)(float)h, df = (double)(float)xz;
      double x = (double)ctr + rint(df * sin(hf) / res), y = (double)ctr - rint(df * cos(hf) / res);
      x = x >= 0.0 ? (x >= (double)dim ? (double)(dim - 1) : x) : 0.0;      // (NaN lands in cell 0, never outside)
      y = y >= 0.0 ? (y >= (double)dim ? (double)(dim - 1) : y) : 0.0;
      const int cell = (int)y * dim + (int)x;
      cand_idxs[(size_t)b * K + n] = cell;
      cand_ids[(size_t)b * K + n] = pass == 0 ? i : N + i;
      vis_c[(size_t)b * K + n] = pass == 0;                      // a candidate that is a visited node: backtrack logit
      nav_masks[(size_t)b * cells + cell] = 1;
      ++n;
    }
  }
  cand_n[b] = n;
  ce_pos_fts(st, b, cur, p, p[3], 0, gpos_fts + b * 7);         // get_pos_fts(..., ['0']): the start node
  // SAP fusion: gmap row j of an unvisited entry (a ghost) reads the local logit of the candidate slot that holds the
  // same ghost (the last such slot), else the backtrack logit K; visited nodes and padding read the zero slot.  The
  // listing is the one of bevbert_ce_nav_vars: [stop], nodes, live ghosts in creation order.
  int j = 1 + nn;
  for (int g = 0; g < gcnt; ++g) {
    if (!st.g_alive[(size_t)b * Gh + g]) continue;
    int64_t s = K;
    for (int c = 1; c < n; ++c)
      if (cand_ids[(size_t)b * K + c] == N + g) s = c;
    if (j < G) src[(size_t)b * G + j] = s;
    ++j;
  }
}

BEVBERT_API int bevbert_ce_bev_cands(const bevbert_ce_state* st, const double* pose, const uint8_t* live, int bev_dim,
                                     double bev_res, int K, uint8_t* nav_masks, int64_t* cand_idxs, int64_t* cand_ids,
                                     int* cand_n, float* gpos_fts, int64_t* src, uint8_t* vis_c, hipStream_t stream) {
  BB_REQUIRE(st && st->N >= 1 && st->N <= CE_MAX_N && st->Gh >= 1 && 1 + st->N + st->Gh <= CE_MAX_G,
             "ce_bev_cands: N=%d (<= 64) Gh=%d (1 + N + Gh <= 512)", st ? st->N : -1, st ? st->Gh : -1);
  BB_REQUIRE(bev_dim >= 1 && bev_dim <= 1024 && bev_res > 0.0 && K >= 1, "ce_bev_cands: dim=%d res=%f K=%d", bev_dim,
             bev_res, K);
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(pose && live && nav_masks && cand_idxs && cand_ids && cand_n && gpos_fts && src && vis_c,
             "ce_bev_cands: null tensor%s", "");
  hipLaunchKernelGGL(ce_bev_cands_kernel, dim3(st->B), dim3(64), 0, stream, *st, pose, live, bev_dim, bev_res, K,
                     1 + st->N + st->Gh, nav_masks, cand_idxs, cand_ids, cand_n, gpos_fts, src, vis_c);
  BB_CHECK_LAUNCH("ce_bev_cands");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (d) per-map scalars: one thread per map.
__global__ void ce_stop_scores_kernel(bevbert_ce_state st, const uint8_t* __restrict__ live, const float* __restrict__ probs0,
                                      int stride) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.B || !live[b]) return;
  st.stop_score[b * st.N + st.cur_vp[b]] = probs0[(size_t)b * stride];      // node_stop_scores[cur_vp] = nav_probs[i, 0]
}

BEVBERT_API int bevbert_ce_stop_scores(const bevbert_ce_state* st, const uint8_t* live, const float* probs0, int stride,
                                       hipStream_t stream) {
  BB_REQUIRE(st && stride >= 1, "ce_stop_scores: stride=%d", stride);
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(live && probs0, "ce_stop_scores: null tensor%s", "");
  hipLaunchKernelGGL(ce_stop_scores_kernel, dim3((st->B + 63) / 64), dim3(64), 0, stream, *st, live, probs0, stride);
  BB_CHECK_LAUNCH("ce_stop_scores");
  return BB_OK;
}

// _teacher_action_new, expert_policy 'spl', from distances the caller measured: < 1.5 m from the goal -> 0 (checked
// first), no ghost left -> -100, else the position in the listing of the live ghost with the first minimal distance.
__global__ void ce_teacher_kernel(bevbert_ce_state st, const uint8_t* __restrict__ live,
                                  const double* __restrict__ cur_dist, const double* __restrict__ ghost_dist,
                                  int64_t* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.B) return;
  int64_t t = -100;
  if (live[b]) {
    if (cur_dist[b] < 1.5) {
      t = 0;
    } else {
      const int gcnt = st.g_cnt[b];
      int rank = 0, best = -1;
      double bd = 0.0;
      for (int g = 0; g < gcnt; ++g) {
        if (!st.g_alive[(size_t)b * st.Gh + g]) continue;
        const double d = ghost_dist[(size_t)b * st.Gh + g];
        if (best < 0 || d < bd) { bd = d; best = rank; }         // np.argmin: the first minimum
        ++rank;
      }
      if (best >= 0) t = 1 + st.n_nodes[b] + best;
    }
  }
  out[b] = t;
}

BEVBERT_API int bevbert_ce_teacher(const bevbert_ce_state* st, const uint8_t* live, const double* cur_dist,
                                   const double* ghost_dist, int64_t* out, hipStream_t stream) {
  BB_REQUIRE(st != nullptr, "ce_teacher: null state%s", "");
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(live && cur_dist && ghost_dist && out, "ce_teacher: null tensor%s", "");
  hipLaunchKernelGGL(ce_teacher_kernel, dim3((st->B + 63) / 64), dim3(64), 0, stream, *st, live, cur_dist, ghost_dist, out);
  BB_CHECK_LAUNCH("ce_teacher");
  return BB_OK;
}

// The action block.  Stop rule: a_t == 0, the last step, or no ghost left -> act 0 at the node with the FIRST maximal
// recorded stop score (np.argmax over node_stop_scores in insertion = creation order).  Else act 4: the chosen row of the
// listing must be a live ghost; front = its nearest front; prev_vp = front; consume_ghost deletes the ghost.  back_path =
// shortest_path[cur][target][1:] as node indices, walked backwards through the predecessor table.
// rec (B, 11 + 4 N) f64: [act (-1 = ended / refused), cur, target node (stop_vp / front_vp), ghost id (-1), path length,
// path (N, padded -1), target position (3), ghost position (3), positions of the path's nodes (N, 3)].
__global__ void ce_act_kernel(bevbert_ce_state st, const uint8_t* __restrict__ live, const int64_t* __restrict__ a_t,
                              const int64_t* __restrict__ gmap_ids, int G, int last_step, int consume,
                              double* __restrict__ rec_) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.B) return;
  const int N = st.N, Gh = st.Gh, R = 11 + 4 * N;
  double* rec = rec_ + (size_t)b * R;
  for (int i = 0; i < R; ++i) rec[i] = (i >= 5 && i < 5 + N) || i < 4 ? -1.0 : 0.0;
  if (!live[b]) return;
  const int cur = st.cur_vp[b], nn = st.n_nodes[b], gcnt = st.g_cnt[b];
  bool any = false;
  for (int g = 0; g < gcnt; ++g) any |= st.g_alive[(size_t)b * Gh + g] != 0;
  const int64_t a = a_t[b];
  int target, ghost = -1, act;
  if (a == 0 || last_step || !any) {
    act = 0;
    target = 0;
    float best = st.stop_score[b * N];
    for (int k = 1; k < nn; ++k) {
      const float s = st.stop_score[b * N + k];
      if (s > best) { best = s; target = k; }
    }
  } else {
    const int64_t id = (a > 0 && a < G) ? gmap_ids[(size_t)b * G + a] : -1;
    if (id < N || id >= N + gcnt || !st.g_alive[(size_t)b * Gh + (id - N)]) {
      *st.overflow = 2;                                        // not a live ghost: the reference raises KeyError here
      return;
    }
    act = 4;
    ghost = (int)id - N;
    double fd;
    target = ce_front(st, b, ghost, fd);
    const double* gp = st.g_aug + ((size_t)b * Gh + ghost) * 3;
    rec[8 + N] = gp[0]; rec[9 + N] = gp[1]; rec[10 + N] = gp[2];
    st.prev_vp[b] = target;
    if (consume) st.g_alive[(size_t)b * Gh + ghost] = 0;         // delete_ghost: the id is never reused
  }
  const int* pr = st.pred + ((size_t)b * N + cur) * N;
  int len = 0;
  for (int v = target; v != cur && v >= 0 && len < N; v = pr[v]) ++len;
  int i = len;
  for (int v = target; v != cur && v >= 0 && i > 0; v = pr[v]) {
    --i;
    rec[5 + i] = (double)v;
    for (int c = 0; c < 3; ++c) rec[11 + N + i * 3 + c] = st.node_pos[((size_t)b * N + v) * 3 + c];
  }
  const double* tp = st.node_pos + ((size_t)b * N + target) * 3;
  rec[0] = act; rec[1] = cur; rec[2] = target; rec[3] = ghost; rec[4] = len;
  rec[5 + N] = tp[0]; rec[6 + N] = tp[1]; rec[7 + N] = tp[2];
}

BEVBERT_API int bevbert_ce_act(const bevbert_ce_state* st, const uint8_t* live, const int64_t* a_t, const int64_t* gmap_ids,
                               int last_step, int consume_ghost, double* rec, hipStream_t stream) {
  BB_REQUIRE(st && st->N >= 1 && st->N <= CE_MAX_N, "ce_act: N=%d (<= 64)", st ? st->N : -1);
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(live && a_t && gmap_ids && rec, "ce_act: null tensor%s", "");
  hipLaunchKernelGGL(ce_act_kernel, dim3((st->B + 63) / 64), dim3(64), 0, stream, *st, live, a_t, gmap_ids,
                     1 + st->N + st->Gh, last_step, consume_ghost, rec);
  BB_CHECK_LAUNCH("ce_act");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (e) the panorama store and the node choice of the BEV.  update_node_pc keeps, per node, what lift made of the step's
// panorama; here a node keeps the lift's INPUTS (grid features, depths, camera matrices) in slot b * N + node of a
// per-episode device store and the existing lift / splat kernels read them in place.
__global__ __launch_bounds__(256) void ce_remember_kernel(bevbert_ce_state st, const uint8_t* __restrict__ live,
                                                          const uint32_t* __restrict__ src, uint32_t* __restrict__ store,
                                                          int64_t row_words) {
  const int b = blockIdx.y;
  if (!live[b]) return;
  const uint32_t* in = src + (size_t)b * row_words;
  uint32_t* out = store + ((size_t)b * st.N + st.cur_vp[b]) * row_words;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < row_words; i += (int64_t)gridDim.x * 256) out[i] = in[i];
}

BEVBERT_API int bevbert_ce_remember(const bevbert_ce_state* st, const uint8_t* live, const void* src, void* store,
                                    int64_t row_bytes, hipStream_t stream) {
  BB_REQUIRE(st && st->N >= 1 && row_bytes > 0 && row_bytes % 4 == 0, "ce_remember: row_bytes=%lld (multiple of 4)",
             (long long)row_bytes);
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(live && src && store, "ce_remember: null tensor%s", "");
  const int64_t words = row_bytes / 4;
  const int gx = (int)((words + 255) / 256 < 256 ? (words + 255) / 256 : 256);
  hipLaunchKernelGGL(ce_remember_kernel, dim3(gx, st->B), dim3(256), 0, stream, *st, live, (const uint32_t*)src,
                     (uint32_t*)store, words);
  BB_CHECK_LAUNCH("ce_remember");
  return BB_OK;
}

// gather_node_pc(cur, order) AS WRITTEN: order == 0 is the current node; otherwise every node, in creation order, with
// len(shortest_path[cur][node]) <= order.  The path counts both end points, so order = 1 (the trainer's call) still
// selects the current node only and the 1-hop neighbours need order = 2.  rows (B,R) = store slots b * N + node, padding
// repeats the map's slot 0 with row_live = 0 (its depths are gathered as 0, which the binning drops); more than R nodes
// raise the overflow flag.
__global__ void ce_bev_select_kernel(bevbert_ce_state st, const uint8_t* __restrict__ live, int order, int R,
                                     int* __restrict__ rows, uint8_t* __restrict__ row_live) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.B) return;
  const int N = st.N;
  int n = 0;
  if (live[b]) {
    const int cur = st.cur_vp[b], nn = st.n_nodes[b];
    const int* hrow = st.hops + ((size_t)b * N + cur) * N;
    for (int k = 0; k < nn; ++k) {
      const bool in = order == 0 ? k == cur : (hrow[k] >= 1 && hrow[k] <= order);
      if (!in) continue;
      if (n >= R) { *st.overflow = 1; break; }
      rows[b * R + n] = b * N + k;
      row_live[b * R + n] = 1;
      ++n;
    }
  }
  for (; n < R; ++n) { rows[b * R + n] = b * N; row_live[b * R + n] = 0; }
}

BEVBERT_API int bevbert_ce_bev_select(const bevbert_ce_state* st, const uint8_t* live, int order, int R, int* rows,
                                      uint8_t* row_live, hipStream_t stream) {
  BB_REQUIRE(st && st->N >= 1 && st->N <= CE_MAX_N && order >= 0 && R >= 1, "ce_bev_select: order=%d R=%d", order, R);
  if (st->B == 0) return BB_OK;
  BB_REQUIRE(live && rows && row_live, "ce_bev_select: null tensor%s", "");
  hipLaunchKernelGGL(ce_bev_select_kernel, dim3((st->B + 63) / 64), dim3(64), 0, stream, *st, live, order, R, rows, row_live);
  BB_CHECK_LAUNCH("ce_bev_select");
  return BB_OK;
}
