// Training side of the continuous-environment (CE) agent's ghost-node map (csrc/ce_map.hip): what a rollout needs
// besides the forward step so that ss_trainer_BEV.py's rollout('train') can run on the device map.
//   (a) bevbert_ce_tape_record     what the adjoint has to know about one update: the node made, the ghost each
//                                  candidate went to and the panorama row it brought
//   (b) bevbert_ce_embeds_bwd      the adjoint of the map's embedding path: d gmap_img_fts[t] -> d avg_pano_embeds[s],
//                                  d pano_embeds[s] for every step s <= t, in one launch
//   (c) bevbert_ce_sample_action   the action draw of ss_trainer_BEV.py:1097-1100
// In the reference the embeddings are live tensors in GraphMap.node_embeds / ghost_embeds (ss_trainer_BEV.py:1060-1066,
// graph_utils.py:211,229,238,277-281) and autograd carries the loss of step t back to the panorama encoder's pass of
// every earlier step; the device map keeps them in raw arrays, so the path gets its own adjoint here.  Launch-only, fixed
// shapes, no atomics, plain stores.
#include "common.h"

#define CE_MAX_N 64                 // as csrc/ce_map.hip
#define CE_MAX_G 512
#define CE_MAX_C 16

// ----------------------------------------------------------------------------------------------------------------
// (a) One thread per map, after bevbert_ce_update of tape step s.  A map that is not live, or whose update was refused
// (node capacity: cur_vp did not move), records cur = -1 and no candidates.  Node ids only ever grow within an episode,
// so "cur_vp differs from the node recorded last" is "this update made a node"; last_cur (B) is -1 at episode start.
// row[j] = the j-th row of nav_types (B,L) that is 1 (cand_embeds = pano_embeds[nav_types == 1]), kept only for a
// candidate that went to a ghost (cand_slot >= N): a localised (< N) or refused (-1) candidate brought no embedding.
__global__ void ce_tape_record_kernel(const int* __restrict__ cur_vp, const uint8_t* __restrict__ live,
                                      const int* __restrict__ cand_slot, const int64_t* __restrict__ nav_types, int B, int N,
                                      int C, int L, int* __restrict__ last_cur, int* __restrict__ cur_out,
                                      uint8_t* __restrict__ live_out, int* __restrict__ slot_out, int* __restrict__ row_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int cur = cur_vp[b];
  const bool on = live[b] != 0 && cur != last_cur[b];
  cur_out[b] = on ? cur : -1;
  live_out[b] = on;
  if (on) last_cur[b] = cur;
  int row = 0;
  for (int j = 0; j < C; ++j) {
    int r = -1;
    if (on) {
      while (row < L && nav_types[(size_t)b * L + row] != 1) ++row;
      r = row < L ? row : -1;
      ++row;
    }
    const int e = on ? cand_slot[b * C + j] : -1;
    const bool ghost = e >= N && r >= 0;
    slot_out[b * C + j] = ghost ? e : -1;
    row_out[b * C + j] = ghost ? r : -1;
  }
}

BEVBERT_API int bevbert_ce_tape_record(const int* cur_vp, const uint8_t* live, const int* cand_slot, const int64_t* nav_types,
                                       int B, int N, int C, int L, int* last_cur, int* cur_out, uint8_t* live_out,
                                       int* slot_out, int* row_out, hipStream_t stream) {
  BB_REQUIRE(N >= 1 && N <= CE_MAX_N && C >= 1 && C <= CE_MAX_C && L >= 1, "ce_tape_record: N=%d (<= 64) C=%d (1..16) L=%d",
             N, C, L);
  if (B <= 0) return BB_OK;
  BB_REQUIRE(cur_vp && live && cand_slot && nav_types && last_cur && cur_out && live_out && slot_out && row_out,
             "ce_tape_record: null tensor%s", "");
  hipLaunchKernelGGL(ce_tape_record_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, cur_vp, live, cand_slot, nav_types, B, N,
                     C, L, last_cur, cur_out, live_out, slot_out, row_out);
  BB_CHECK_LAUNCH("ce_tape_record");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (b) The adjoint, in gather form.  Forward (ce_nav_vars_kernel): row r of gmap_img_fts[t][b] with id e = gmap_ids[t][b, r]
// is 0 for [stop] / padding, the avg_pano_embeds[s][b] of the step s that made node e, or g_sum / g_npos of ghost e - N:
// the fp32 sum of the pano rows of all its observations so far over their count at step t.
// One wave per TARGET (s, b, k), s <= t: k = 0 is avg_pano_embeds[s][b], k = 1 + j is the panorama row of candidate j of
// step s.  A target finds its element (the node step s made; the ghost candidate j went to), the element's row in
// gmap_ids[t][b] (a node sits at 1 + e; a ghost is searched among the G <= 512 ids, one compare per lane and round), reads
// that ONE row of dG and adds it into its own accumulator row:
//     d_avg[s][b]           += dG[b, r]
//     d_pano[s][b, row(j)]  += dG[b, r] / cnt_t(ghost)            (a division, as autograd's x / count gives)
// Nothing is added for a map that was not live at s or at t, for a candidate that was localised to a node or refused
// (recorded as slot -1), or for a ghost that act consumed before step t (it is not in the listing any more).  Two
// candidates of one step that merged into one ghost own different rows, so no two waves write the same address.
// ORDER: one launch per consumer step t.  The accumulators are fp32 and a row receives the consumer steps one launch after
// the other, in the order the launches are issued: backward of a rollout loss visits the consumer steps from the last to
// the first (autograd runs the node created last first), so row x holds ((0 + c_T-1) + c_T-2) + ... -- descending t.
template <typename T>
__global__ __launch_bounds__(64) void ce_embeds_bwd_kernel(
    const T* __restrict__ dG, int t, int B, int N, int Gh, int C, int L, int H, const int* __restrict__ cur,
    const uint8_t* __restrict__ live, const int* __restrict__ slot, const int* __restrict__ row,
    const int64_t* __restrict__ ids, const int* __restrict__ cnt, float* __restrict__ d_avg, float* __restrict__ d_pano) {
  const int lane = threadIdx.x, G = 1 + N + Gh;
  const int k = blockIdx.x % (C + 1), sb = blockIdx.x / (C + 1), b = sb % B, s = sb / B;
  const size_t tb = (size_t)t * B + b;
  if (!live[tb] || !live[sb]) return;
  const int64_t* idt = ids + tb * G;
  int r = -1;
  float* acc;
  float count = 0.f;                                             // 0: a node row, no division
  if (k == 0) {
    const int e = cur[sb];
    if (e < 0 || e >= N || idt[1 + e] != e) return;
    r = 1 + e;
    acc = d_avg + (size_t)sb * H;
  } else {
    const int e = slot[(size_t)sb * C + k - 1], rw = row[(size_t)sb * C + k - 1];
    if (e < N || e >= N + Gh || rw < 0 || rw >= L) return;
    for (int j0 = 0; j0 < G; j0 += 64) {                         // ids are unique within a listing: at most one lane hits
      const int j = j0 + lane;
      if (j < G && idt[j] == e) r = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r = max(r, __shfl_xor(r, o, 64));
    if (r < 0) return;                                           // consumed before step t
    const int c = cnt[tb * Gh + (e - N)];
    if (c <= 0) return;
    count = (float)c;
    acc = d_pano + ((size_t)sb * L + rw) * H;
  }
  const T* g = dG + ((size_t)b * G + r) * H;
  if ((H & 3) == 0) {
    for (int i = lane * 4; i < H; i += 256) {
      float4 x = ld4<T>(g + i);
      float4 a = *reinterpret_cast<float4*>(acc + i);
      if (count != 0.f) { x.x /= count; x.y /= count; x.z /= count; x.w /= count; }
      add4(a, x);
      *reinterpret_cast<float4*>(acc + i) = a;
    }
  } else {
    for (int i = lane; i < H; i += 64) {
      float x = io<T>::ld(g + i);
      if (count != 0.f) x /= count;
      acc[i] += x;
    }
  }
}

BEVBERT_API int bevbert_ce_embeds_bwd(const void* dG, int dtype, int t, int T, int B, int N, int Gh, int C, int L, int H,
                                      const int* cur, const uint8_t* live, const int* slot, const int* row, const int64_t* ids,
                                      const int* cnt, float* d_avg, float* d_pano, hipStream_t stream) {
  BB_REQUIRE(N >= 1 && N <= CE_MAX_N && Gh >= 1 && 1 + N + Gh <= CE_MAX_G && C >= 1 && C <= CE_MAX_C && L >= 1 && H >= 1,
             "ce_embeds_bwd: N=%d (<= 64) Gh=%d (1 + N + Gh <= 512) C=%d (1..16) L=%d H=%d", N, Gh, C, L, H);
  BB_REQUIRE(T >= 1 && t >= 0 && t < T, "ce_embeds_bwd: step %d outside the tape (%d steps)", t, T);
  if (B <= 0) return BB_OK;
  BB_REQUIRE(dG && cur && live && slot && row && ids && cnt && d_avg && d_pano, "ce_embeds_bwd: null tensor%s", "");
  BB_REQUIRE((long long)(t + 1) * B * (C + 1) < (1ll << 31), "ce_embeds_bwd: %d steps x %d maps is too many targets", t + 1, B);
  const dim3 grid((unsigned)((t + 1) * B * (C + 1)));
  if (!bb_with_type(dtype, [&](auto T_) {
        using T = decltype(T_);
        hipLaunchKernelGGL(ce_embeds_bwd_kernel<T>, grid, dim3(64), 0, stream, (const T*)dG, t, B, N, Gh, C, L, H, cur, live,
                           slot, row, ids, cnt, d_avg, d_pano);
      }))
    return bb_dtype_unsupported("ce_embeds_bwd", dtype);
  BB_CHECK_LAUNCH("ce_embeds_bwd");
  return BB_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// (c) The action draw of a training rollout (ss_trainer_BEV.py:1097-1100): a_t = Categorical(softmax(logits)).sample(),
// replaced by the teacher's action where rand <= sample_ratio (the reference's <=).  One wave per map.  The draw is the
// `sample` branch of ne_action_kernel (csrc/nav_expert.hip) with the same arithmetic: fp32 softmax around the row
// maximum (lane-strided sums, then wave_sum; one reciprocal), the cumulative sum in row order by lane 0, the first j with
// u0 < c and p > 0, else the last positive j.  A teacher value
// of -100 (no ghost left) passes through as it does in the reference; bevbert_ce_act stops such a map.
// Uniform draws: u0 = 24 bits of hash(k ^ 4 b), u1 = 24 bits of hash(k ^ (4 b + 1)), k = salted(bb_stream_key(
// bb_site_key(seed, t), BB_STREAM_CE_ACTION)) -- the counters of the nav draw under a domain of its own.
__global__ __launch_bounds__(64) void ce_sample_action_kernel(
    const void* __restrict__ logits_, int bf16, int C, const int64_t* __restrict__ teacher, float sample_ratio, uint32_t key,
    const uint32_t* __restrict__ salt, int64_t* __restrict__ a_out, float* __restrict__ u0_out, float* __restrict__ u1_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t row = (size_t)b * C;
  auto ld = [&](int j) -> float {
    return bf16 ? bf16_to_f32(((const bf16_raw*)logits_)[row + j]) : ((const float*)logits_)[row + j];
  };
  float m = -INFINITY;
  for (int j = lane; j < C; j += 64) m = fmaxf(m, ld(j));
  m = wave_max(m);
  float s = 0.f;
  for (int j = lane; j < C; j += 64) s += __expf(ld(j) - m);
  s = wave_sum(s);
  const float inv = 1.f / s;
  if (lane != 0) return;
  const uint32_t k0 = bb_salted(key, salt);
  const float u0 = (bb_hash32(k0 ^ (4u * b)) >> 8) * (1.f / 16777216.f);
  const float u1 = (bb_hash32(k0 ^ (4u * b + 1u)) >> 8) * (1.f / 16777216.f);
  int pick = -1, lastpos = 0;
  float c = 0.f;
  for (int j = 0; j < C; ++j) {
    const float p = __expf(ld(j) - m) * inv;
    if (p > 0.f) lastpos = j;
    c += p;
    if (pick < 0 && u0 < c && p > 0.f) pick = j;
  }
  int64_t a = pick >= 0 ? pick : lastpos;
  if (u1 <= sample_ratio) a = teacher[b];
  a_out[b] = a;
  u0_out[b] = u0;
  u1_out[b] = u1;
}

BEVBERT_API int bevbert_ce_sample_action(const void* logits, int dtype, int B, int C, const int64_t* teacher,
                                         float sample_ratio, uint32_t seed, int t, int64_t* a_t, float* u0, float* u1,
                                         hipStream_t stream) {
  BB_REQUIRE(C >= 1, "ce_sample_action: C=%d", C);
  BB_REQUIRE(dtype == BB_F32 || dtype == BB_BF16, "ce_sample_action: dtype %d unsupported", dtype);
  if (B <= 0) return BB_OK;
  BB_REQUIRE(logits && teacher && a_t && u0 && u1, "ce_sample_action: null tensor%s", "");
  hipLaunchKernelGGL(ce_sample_action_kernel, dim3(B), dim3(64), 0, stream, logits, dtype == BB_BF16, C, teacher, sample_ratio,
                     bb_stream_key(bb_site_key(seed, (uint64_t)t), BB_STREAM_CE_ACTION), bb_step_salt(), a_t, u0, u1);
  BB_CHECK_LAUNCH("ce_sample_action");
  return BB_OK;
}
