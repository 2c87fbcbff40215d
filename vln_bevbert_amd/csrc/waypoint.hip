// Candidate waypoint prediction of the continuous-environment agent (bevbert_ce/vlnce_baselines: waypoint_pred/TRM_net.py,
// waypoint_pred/utils.py:8-64, models/Policy_ViewSelection_BEV.py:166-321 mode 'waypoint', ss_trainer_BEV.py:347-384
// _vp_feature_variable).  Three entries, forward only, no atomics, fixed output shapes, nothing synchronises:
//   (a) bevbert_wp_ring_attn     self-attention over the 12-view ring of the predictor's 2-layer encoder;
//   (b) bevbert_wp_candidates    softmax heat map -> wrapped map -> 5 rounds of arg-max + suppression -> candidate list
//                                (+ the training draw) -> angle / distance / image indices and features;
//   (c) bevbert_wp_pano_inputs   4 x 4 depth pooling, clockwise -> counter-clockwise re-ordering and the padded
//                                panorama-encoder inputs.
#include "common.h"

#define WP_VIEWS 12
#define WP_ANGLES 120
#define WP_DISTS 12
#define WP_CELLS (WP_ANGLES * WP_DISTS)              // 1 440
#define WP_WROWS (WP_ANGLES + 2)                     // the map wrapped by one row on either side
#define WP_WCELLS (WP_WROWS * WP_DISTS)              // 1 464
#define WP_REGION 120                                // 10 angles x 12 distances: the cells that belong to one image
#define WP_KMAX 5
#define WP_L 17                                      // 5 candidates + 12 views: the most a panorama can hold
#define WP_OFFSET 5                                  // HEATMAP_OFFSET: every image points at the middle of its 10 angles

// ----------------------------------------------------------------------------------------------------------------
// (a) Ring attention.  One wave per (sample, head), lane = one of the 64 head dimensions; the 12 q / k / v rows of the
// head sit in registers (36 values per lane).  Query i attends to keys i-1, i, i+1 on the ring (TRM_NEIGHBOR = 1, the
// only predictor there is).  The reference (waypoint_bert.py:66-72,183-184) scores all 12 keys and adds -10000 to the
// other nine: in fp32 exp(-10000 + s - max) is exactly 0 for any finite scores of this model's size, so the softmax over
// the three keys is the same function and the nine products with V are never needed.  Eval only: no dropout, no backward.
template <typename T>
__global__ __launch_bounds__(256) void wp_ring_attn_kernel(const T* __restrict__ qkv, T* __restrict__ out, int pairs,
                                                           int nh, float scale) {
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pair >= pairs) return;                         // whole waves leave together; no barrier follows
  const int b = pair / nh, h = pair - b * nh;
  const size_t H = (size_t)nh * 64;
  const T* base = qkv + (size_t)b * WP_VIEWS * 3 * H + (size_t)h * 64 + lane;
  float q[WP_VIEWS], k[WP_VIEWS], v[WP_VIEWS];
#pragma unroll
  for (int i = 0; i < WP_VIEWS; ++i) {
    const T* row = base + (size_t)i * 3 * H;
    q[i] = io<T>::ld(row);
    k[i] = io<T>::ld(row + H);
    v[i] = io<T>::ld(row + 2 * H);
  }
  T* o = out + (size_t)b * WP_VIEWS * H + (size_t)h * 64 + lane;
#pragma unroll
  for (int i = 0; i < WP_VIEWS; ++i) {
    const int jm = (i + WP_VIEWS - 1) % WP_VIEWS, jp = (i + 1) % WP_VIEWS;
    const float sm = wave_sum(q[i] * k[jm]) * scale, s0 = wave_sum(q[i] * k[i]) * scale,
                sp = wave_sum(q[i] * k[jp]) * scale;
    const float m = fmaxf(sm, fmaxf(s0, sp));
    const float em = expf(sm - m), e0 = expf(s0 - m), ep = expf(sp - m);
    const float inv = 1.0f / (em + e0 + ep);
    io<T>::st(o + (size_t)i * H, (em * v[jm] + e0 * v[i] + ep * v[jp]) * inv);
  }
}

BEVBERT_API int bevbert_wp_ring_attn(const void* qkv, void* out, int B, int nh, float scale, int dtype,
                                     hipStream_t stream) {
  BB_REQUIRE(dtype == BB_F32 || dtype == BB_BF16, "wp_ring_attn: dtype %d unsupported", dtype);
  BB_REQUIRE(B >= 0 && nh >= 1 && (int64_t)B * nh < (1 << 28), "wp_ring_attn: B=%d nh=%d", B, nh);
  if (B == 0) return BB_OK;
  BB_REQUIRE(qkv && out, "wp_ring_attn: null tensor%s", "");
  const int pairs = B * nh;
  const dim3 grid((pairs + 3) / 4), block(256);
  bb_with_type(dtype, [&](auto t) {                     // one of the two: checked above
    using T = decltype(t);
    hipLaunchKernelGGL(wp_ring_attn_kernel<T>, grid, block, 0, stream, (const T*)qkv, (T*)out, pairs, nh, scale);
  });
  BB_CHECK_LAUNCH("wp_ring_attn");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (b) Candidates.  One workgroup of 256 threads per sample; the heat map and the suppressed copy live in LDS.
// `raw` is the classifier output (B,12,120) BEFORE the predictor's roll: raw row r = 10 * image + k, and angle a of the
// rolled map is raw row (a + 5) % 120 -- the roll (TRM_net.py:84-86) and its inverse for the training regions
// (Policy_ViewSelection_BEV.py:232-237) are index arithmetic here.
//
// The reference is reproduced as it executes, including (named, not "fixed"):
//   Q1  nms computes y = ix / 12 with TRUE division (utils.py:55): the suppression centre on the angle axis is the
//       fractional row + col/12, so |r - y| <= 5 covers rows row-4 .. row+5 whenever col > 0 (row-5 .. row+5 for col = 0);
//   Q2  nms' "x" axis is the 12-wide DISTANCE axis and circular_x wraps it with min(|d|, |d + 12|) <= 7, d = col -
//       col_picked (utils.py:25-26): not symmetric, cells with d = 8..11 survive;
//   Q3  the map is wrapped by one row (Policy_ViewSelection_BEV.py:216-220) but nms is not circular in rows: wrapped row 0
//       duplicates angle 119 and, lower index winning ties, is picked first when angle 119 holds the maximum; [:, 1:-1]
//       cuts that pick off, so a sample can end with fewer than 5 candidates, and the duplicate at wrapped row 120
//       competes again in a later round;
//   Q4  the training draw maps image 0 to angle_pointer = 0 although its region holds angles 115..119, 0..4
//       (Policy_ViewSelection_BEV.py:257-261); drawn angles are not de-duplicated.
// Also as there: a pick writes the UNSUPPRESSED probability into the output map and nonzero() lists the non-zero cells
// in row-major order, so a pick whose probability underflowed to 0 is no candidate, and a cell picked twice counts once.
//
// Uniform draws (training): 24 bits of hash(salted(site_key(seed, t)) ^ (8 b + k)), the convention of bevbert_nav_action.
struct WpArgMax { float v; int i; };
__device__ __forceinline__ WpArgMax wp_better(WpArgMax a, WpArgMax b) {      // torch.max: the first index wins ties
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__global__ __launch_bounds__(256) void wp_candidates_kernel(
    const float* __restrict__ raw_, int in_train, uint32_t key, const uint32_t* __restrict__ salt,
    int* __restrict__ cand_count, int* __restrict__ cand_angle_idx, int* __restrict__ cand_dist_idx,
    int* __restrict__ cand_img_idx, float* __restrict__ cand_angle_fts, float* __restrict__ cand_angles,
    float* __restrict__ cand_distances, float* __restrict__ region_probs, float* __restrict__ heat_,
    float* __restrict__ rand_out) {
  __shared__ float P[WP_CELLS];              // softmax over the 1 440 cells, angle-major
  __shared__ float S[WP_WCELLS];             // wrapped map under suppression
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ int picks[WP_KMAX];
  __shared__ int c_angle[WP_KMAX], c_dist[WP_KMAX], c_n;
  __shared__ float rp[WP_KMAX][WP_REGION];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* raw = raw_ + (size_t)b * WP_CELLS;

  // ---- softmax over all cells of the rolled map
  float m = -INFINITY;
  for (int f = tid; f < WP_CELLS; f += 256) {
    const float x = raw[(f + WP_OFFSET * WP_DISTS) % WP_CELLS];
    P[f] = x;
    m = fmaxf(m, x);
  }
  m = wave_max(m);
  if (lane == 0) redf[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
  __syncthreads();
  float s = 0.f;
  for (int f = tid; f < WP_CELLS; f += 256) {
    const float e = expf(P[f] - m);
    P[f] = e;
    s += e;
  }
  s = wave_sum(s);
  if (lane == 0) redf[wave] = s;
  __syncthreads();
  s = (redf[0] + redf[1]) + (redf[2] + redf[3]);
  float* heat = heat_ + (size_t)b * WP_CELLS;
  for (int f = tid; f < WP_CELLS; f += 256) {
    const float p = P[f] / s;
    P[f] = p;
    heat[f] = p;
  }
  __syncthreads();
  for (int c = tid; c < WP_WCELLS; c += 256) {
    const int w = c / WP_DISTS, d = c - w * WP_DISTS;
    S[c] = P[((w + WP_ANGLES - 1) % WP_ANGLES) * WP_DISTS + d];            // Q3: rows 119 | 0..119 | 0
  }
  __syncthreads();

  // ---- max_predictions = 5 rounds of arg-max + suppression, sigma = (7, 5)
  for (int r = 0; r < WP_KMAX; ++r) {
    WpArgMax best = {-INFINITY, 0x7fffffff};
    for (int c = tid; c < WP_WCELLS; c += 256) best = wp_better(best, WpArgMax{S[c], c});
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      best = wp_better(best, WpArgMax{__shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64)});
    if (lane == 0) { redf[wave] = best.v; redi[wave] = best.i; }
    __syncthreads();
    best = WpArgMax{redf[0], redi[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w) best = wp_better(best, WpArgMax{redf[w], redi[w]});
    const int ix = min(max(best.i, 0), WP_WCELLS - 1);      // (a map of NaNs finds no maximum: keep the index in range)
    if (tid == 0) picks[r] = ix;
    const int pr = ix / WP_DISTS, pc = ix - pr * WP_DISTS;
    const int lo = pc == 0 ? pr - 5 : pr - 4, hi = pr + 5;               // Q1
    for (int c = tid; c < WP_WCELLS; c += 256) {
      const int w = c / WP_DISTS, d = c - w * WP_DISTS - pc;
      if (w >= lo && w <= hi && min(abs(d), abs(d + WP_DISTS)) <= 7) S[c] *= 0.f;       // Q2
    }
    __syncthreads();
  }

  // ---- [:, 1:-1] and nonzero(): the surviving picks in row-major order
  if (tid == 0) {
    int f[WP_KMAX], n = 0;
    for (int r = 0; r < WP_KMAX; ++r) {
      const int w = picks[r] / WP_DISTS, d = picks[r] - w * WP_DISTS;
      if (w < 1 || w > WP_ANGLES) continue;                               // Q3: a pick in a wrap row is cut off
      const int cell = (w - 1) * WP_DISTS + d;
      if (!(P[cell] != 0.f)) continue;
      bool dup = false;
      for (int j = 0; j < n; ++j) dup |= f[j] == cell;
      if (dup) continue;
      int j = n++;
      for (; j > 0 && f[j - 1] > cell; --j) f[j] = f[j - 1];
      f[j] = cell;
    }
    c_n = n;
    for (int k = 0; k < WP_KMAX; ++k) {
      c_angle[k] = k < n ? f[k] / WP_DISTS : -1;
      c_dist[k] = k < n ? f[k] % WP_DISTS : -1;
    }
  }
  __syncthreads();
  const int n = c_n;

  // ---- training (waypoint_aug): per candidate one categorical draw from the 120 cells of its image's region
  if (in_train) {
    const uint32_t k0 = bb_salted(key, salt);
    for (int k = wave; k < WP_KMAX; k += 4) {
      float* out = region_probs + ((size_t)b * WP_KMAX + k) * WP_REGION;
      const float u = (bb_hash32(k0 ^ (8u * (uint32_t)b + (uint32_t)k)) >> 8) * (1.f / 16777216.f);
      if (lane == 0) rand_out[b * WP_KMAX + k] = u;
      if (k >= n) {                                   // wave-uniform
        out[lane] = 0.f;
        if (lane + 64 < WP_REGION) out[lane + 64] = 0.f;
        continue;
      }
      const int img = ((c_angle[k] + WP_OFFSET) / 10) % WP_VIEWS;         // clockwise image of the eval candidate
      const float* reg = raw + img * WP_REGION;                           // raw rows 10 img .. 10 img + 9
      const float x0 = reg[lane], x1 = lane + 64 < WP_REGION ? reg[lane + 64] : -INFINITY;
      const float mm = wave_max(fmaxf(x0, x1));
      const float e0 = expf(x0 - mm), e1 = lane + 64 < WP_REGION ? expf(x1 - mm) : 0.f;
      const float ss = wave_sum(e0 + e1);
      rp[k][lane] = out[lane] = e0 / ss;
      if (lane + 64 < WP_REGION) rp[k][lane + 64] = out[lane + 64] = e1 / ss;
    }
    __syncthreads();
    if (tid < n) {
      const int k = tid;
      const float u = (bb_hash32(k0 ^ (8u * (uint32_t)b + (uint32_t)k)) >> 8) * (1.f / 16777216.f);
      int pick = -1, lastpos = 0;
      float c = 0.f;
      for (int j = 0; j < WP_REGION; ++j) {           // inverse CDF, cells in region order
        const float p = rp[k][j];
        if (p > 0.f) lastpos = j;
        c += p;
        if (pick < 0 && u < c && p > 0.f) pick = j;
      }
      const int act = pick >= 0 ? pick : lastpos;
      const int img = ((c_angle[k] + WP_OFFSET) / 10) % WP_VIEWS;
      const int pointer = img != 0 ? (img - 1) * 10 + WP_OFFSET : 0;      // Q4
      c_angle[k] = act / WP_DISTS + pointer;
      c_dist[k] = act % WP_DISTS;
    }
    __syncthreads();
  }

  // ---- per-candidate outputs (Policy_ViewSelection_BEV.py:284-292); the float expressions keep the reference's
  // operation order, one rounding per operation (no contraction)
  if (tid < WP_KMAX) {
    const int k = tid, o = b * WP_KMAX + k;
    const bool live = k < n;
    const int a = c_angle[k], d = c_dist[k];
    cand_angle_idx[o] = live ? a : -1;
    cand_dist_idx[o] = live ? d : -1;
    int img = 12 - (a + WP_OFFSET) / 10;              // counter-clockwise
    if (img == 12) img = 0;
    cand_img_idx[o] = live ? img : -1;
    const float x = __fmul_rn(__fmul_rn(__fdiv_rn((float)a, 120.f), 2.f), 3.14159265358979323846f);    // clockwise
    cand_angle_fts[o * 4 + 0] = live ? sinf(x) : 0.f;
    cand_angle_fts[o * 4 + 1] = live ? cosf(x) : 0.f;
    cand_angle_fts[o * 4 + 2] = 0.f;                  // sin(0)
    cand_angle_fts[o * 4 + 3] = live ? 1.f : 0.f;     // cos(0)
    cand_angles[o] = live ? __fsub_rn(6.283185307179586f, x) : 0.f;
    cand_distances[o] = live ? (float)(d + 1) * 0.25f : 0.f;
    if (k == 0) cand_count[b] = n;
  }
}

BEVBERT_API int bevbert_wp_candidates(const float* logits, int B, int in_train, uint32_t seed, int t, int* cand_count,
                                      int* cand_angle_idx, int* cand_dist_idx, int* cand_img_idx, float* cand_angle_fts,
                                      float* cand_angles, float* cand_distances, float* region_probs, float* heat,
                                      float* rand, hipStream_t stream) {
  BB_REQUIRE(B >= 0 && B < (1 << 24), "wp_candidates: B=%d", B);
  if (B == 0) return BB_OK;
  BB_REQUIRE(logits && cand_count && cand_angle_idx && cand_dist_idx && cand_img_idx && cand_angle_fts && cand_angles &&
                 cand_distances && heat, "wp_candidates: null tensor%s", "");
  BB_REQUIRE(!in_train || (region_probs && rand), "wp_candidates: the training draw needs region_probs and rand%s", "");
  hipLaunchKernelGGL(wp_candidates_kernel, dim3(B), dim3(256), 0, stream, logits, in_train,
                     bb_stream_key(bb_site_key(seed, (uint64_t)t), BB_STREAM_WAYPOINT), bb_step_salt(), cand_count,
                     cand_angle_idx, cand_dist_idx, cand_img_idx, cand_angle_fts, cand_angles, cand_distances,
                     region_probs, heat, rand);
  BB_CHECK_LAUNCH("wp_candidates");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (c) Panorama inputs.  Grid (B, 12 + 17), 128 threads.  Blocks y < 12 write counter-clockwise view y of pano_rgb /
// pano_depth: the predictor takes its views clockwise, so view i comes from input view (12 - i) % 12
// (Policy_ViewSelection_BEV.py:197-205), the depth feature is the 4 x 4 mean (space_pool_depth).  Blocks y >= 12 write
// row y - 12 of the padded encoder inputs (_vp_feature_variable): the candidates in order (features of the view they point
// into, their own angle feature, nav type 1), then the views no candidate points into in ascending index (nav type 0),
// then zeros.
template <typename T>
__global__ __launch_bounds__(128) void wp_pano_inputs_kernel(
    const T* __restrict__ rgb, const T* __restrict__ depth, const int* __restrict__ cand_count,
    const int* __restrict__ cand_img_idx, const float* __restrict__ cand_angle_fts,
    const float* __restrict__ pano_angle_fts, T* __restrict__ pano_rgb, T* __restrict__ pano_depth,
    T* __restrict__ rgb_fts, T* __restrict__ dep_fts, float* __restrict__ loc_fts, int64_t* __restrict__ nav_types,
    int64_t* __restrict__ view_lens) {
  const int b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
  int view = -1, cand = -1;                  // source view (counter-clockwise), candidate slot
  T *orgb, *odep;
  if (y < WP_VIEWS) {
    view = y;
    orgb = pano_rgb + ((size_t)b * WP_VIEWS + y) * 512;
    odep = pano_depth + ((size_t)b * WP_VIEWS + y) * 128;
  } else {
    const int r = y - WP_VIEWS;
    const int n = min(max(cand_count[b], 0), WP_KMAX);
    unsigned taken = 0;
    for (int k = 0; k < n; ++k) {
      const int v = cand_img_idx[b * WP_KMAX + k];
      if ((unsigned)v < WP_VIEWS) taken |= 1u << v;
    }
    const int len = n + WP_VIEWS - __popc(taken);
    if (r < n) {
      cand = r;
      view = cand_img_idx[b * WP_KMAX + r];
      if ((unsigned)view >= WP_VIEWS) view = -1;
    } else if (r < len) {
      int want = r - n;
      for (int v = 0; v < WP_VIEWS; ++v)
        if (!(taken >> v & 1u) && want-- == 0) { view = v; break; }
    }
    orgb = rgb_fts + ((size_t)b * WP_L + r) * 512;
    odep = dep_fts + ((size_t)b * WP_L + r) * 128;
    if (tid < 4) {
      float l = 0.f;
      if (cand >= 0) l = cand_angle_fts[(b * WP_KMAX + cand) * 4 + tid];
      else if (view >= 0) l = pano_angle_fts[view * 4 + tid];
      loc_fts[((size_t)b * WP_L + r) * 4 + tid] = l;
    }
    if (tid == 4) nav_types[(size_t)b * WP_L + r] = cand >= 0 ? 1 : 0;
    if (tid == 5 && r == 0) view_lens[b] = len;
  }
  if (view < 0) {                            // padding row
    st4<T>(orgb + tid * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    io<T>::st(odep + tid, 0.f);
    return;
  }
  const size_t src = (size_t)b * WP_VIEWS + (WP_VIEWS - view) % WP_VIEWS;
  st4<T>(orgb + tid * 4, ld4<T>(rgb + src * 512 + tid * 4));
  const T* dp = depth + (src * 128 + tid) * 16;
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v4 = ld4<T>(dp + q * 4);
    acc += v4.x; acc += v4.y; acc += v4.z; acc += v4.w;
  }
  io<T>::st(odep + tid, acc * 0.0625f);
}

BEVBERT_API int bevbert_wp_pano_inputs(const void* rgb_embeds, const void* depth_embeds, int dtype, int B,
                                       const int* cand_count, const int* cand_img_idx, const float* cand_angle_fts,
                                       const float* pano_angle_fts, void* pano_rgb, void* pano_depth, void* rgb_fts,
                                       void* dep_fts, float* loc_fts, int64_t* nav_types, int64_t* view_lens,
                                       hipStream_t stream) {
  BB_REQUIRE(dtype == BB_F32 || dtype == BB_BF16, "wp_pano_inputs: dtype %d unsupported", dtype);
  BB_REQUIRE(B >= 0 && B < 65536, "wp_pano_inputs: B=%d", B);
  if (B == 0) return BB_OK;
  BB_REQUIRE(rgb_embeds && depth_embeds && cand_count && cand_img_idx && cand_angle_fts && pano_angle_fts && pano_rgb &&
                 pano_depth && rgb_fts && dep_fts && loc_fts && nav_types && view_lens, "wp_pano_inputs: null tensor%s", "");
  const dim3 grid(B, WP_VIEWS + WP_L), block(128);
  bb_with_type(dtype, [&](auto t) {                     // one of the two: checked above
    using T = decltype(t);
    hipLaunchKernelGGL(wp_pano_inputs_kernel<T>, grid, block, 0, stream, (const T*)rgb_embeds, (const T*)depth_embeds, cand_count,
                       cand_img_idx, cand_angle_fts, pano_angle_fts, (T*)pano_rgb, (T*)pano_depth, (T*)rgb_fts, (T*)dep_fts,
                       loc_fts, nav_types, view_lens);
  });
  BB_CHECK_LAUNCH("wp_pano_inputs");
  return BB_OK;
}
