// K2 backward in one pass (bf16 in / fp32 accumulate): 7 key waves + 1 dQ wave per (batch, head).  ONE kernel body for the
// two generations of its step, attn_bwd7p1_kernel<GEN, DROP, KMASK>; GEN 3 is the production backward of the 441 x 441 BEV
// attention (attn_bwd3()), GEN 2 stays behind BEVBERT_ATTN_BWD3=0 as the A/B arm and the dispatch test's cross-check
// (attn_bwd2()).
//   shared:  the kernel head, the K chunk loads, the whole dQ contraction (DqFrags, dq_load, dq_mma, the resident kres
//            fragments, dq_step with its dQ store), the dQ wave's driver loop, the key waves' prologue (V fragments, mask2,
//            accumulators, keep-bit pointer, zero fill of key-less waves), the launcher, the dispatch and the predicate;
//   GEN 2:   K image stored at once by all waves; the dQ wave's tile_issue / tile_commit (okm masks, shift-and-multiply
//            delta); the key waves from bw[8] on: per-key-tile loop, __syncthreads() per step, dK / dV from the accumulators;
//   GEN 3:   K image stored after each wave's other first loads, s_setprio(3) on the dQ wave; its issue_piece / commit_piece
//            (zero fill on the last tile only, dot2_bf16); the key waves from bw[32] on: soft_bwd, the two-phase step, the
//            bare barrier, dK / dV through LDS.
// The shared parts are always-inline lambdas INSIDE the kernel on purpose: as __device__ functions of the header they moved
// the register allocation of all eight instances (both generations sit at 256 VGPRs with spills).
//
// ---- generation 2 (round 3) ------------------------------------------------------------------------------------------
// The round-2 single-pass kernel (attn_bwd1.hip) gives each of 4 waves 112 keys: 224 accumulator registers per wave,
// one wave per SIMD, every dependent chain (matrix result -> softmax arithmetic -> matrix operand) and every LDS round
// trip fully exposed, and two workgroup barriers around a serial dQ phase per query tile: 17 % of the MFMA peak, 37 %
// of the wave time parked (profiles/r02f_pmc_attn_sq_counters.txt).  Here a workgroup has EIGHT waves, two per SIMD:
//
//   * waves 0..6 ("key waves") own 64 keys each (4 tiles of 16): dK^T / dV^T accumulators [64 d][64 keys] = 128
//     registers, V fragments 32 registers; everything else streams from LDS just in time, so a wave stays at <= 256
//     registers and two waves share a SIMD;
//   * the loop runs over 32-query steps.  Per step a key wave computes S and dP against its keys (Q / dO rows are read
//     once per step and reused over the four key tiles), the softmax backward on the accumulators, dK^T += Q^T dS,
//     dV^T += dO^T P (P / dS never leave their lanes), and writes dS (bf16) into a [key][query] LDS image;
//   * wave 7 ("dQ wave") owns no keys.  During step k it (1) starts the global loads of query tile k+1, (2) computes
//     dQ^T[64 d][32 q] of step k-1 over ALL keys from the previous dS image (A = K^T, B = dS^T, both by transposing LDS
//     reads) and stores it, (3) writes tile k+1 (Q, dO rows, delta = rowsum(dO o O), lse) to LDS.  The dS image and the
//     Q / dO tiles are double buffered, so ONE barrier per step is all the synchronisation there is, and the dQ
//     contraction (1/5 of the flops) runs beside the key waves' vector arithmetic instead of after it;
//   * dropout: keep bits in the lanes <-> keys layout written by attn_drop_bits_kernel, fetched with scalar loads and
//     applied with ONE v_cndmask per element (dS / ks = P keep dP - P delta / ks, ks folded into the output scalings);
//     without dropout -delta enters as the C operand of the dP product and dS = P * dP' is a single multiply;
//   * without an additive key mask the scores need no mask term at all (keys beyond Lk are zero rows of the K image).
//
// ---- generation 3 (round 5) ------------------------------------------------------------------------------------------
// The same workgroup with its step re-cut after the measurements of round 5 (profiles/r05_attention_ablations_and_arms.txt,
// r05a_bwd2_phase_timeline_round3_kernel.txt):
//
//   * the round-3 loop spent 54 % of its wave cycles in s_waitcnt: per key tile it re-read the Q^T / dO^T fragments of the
//     dK / dV products from LDS (64 transposing reads per step) right in front of their use.  Here a step has two
//     phases: PHASE 1 walks the 8 chains (16-query tile, key tile) S / dP -> softmax backward -> packed P, dS as a
//     two-deep software pipeline (the matrix instructions of chain i + 1 in front of the vector arithmetic of chain i),
//     PHASE 2 issues the step's 32 dK / dV matrix instructions back to back, d-tile outermost: each Q^T / dO^T fragment is
//     read ONCE per step (16 transposing reads instead of 64; 48 LDS instructions per wave and step instead of 88);
//   * keep-bit words: the 32 words of a step in 64 scalar registers, requested after the step's last LDS store has landed
//     and right in front of the barrier (scalar loads share lgkmcnt with LDS and return out of order: any LDS wait
//     behind an outstanding scalar load waits for it -- the round-3 loop paid that round trip four times per step);
//   * prologue: every wave issues ALL its first loads (K chunks, V fragments / tile 0) before anything waits;
//   * epilogue: dK / dV leave through LDS as whole 128-byte rows, 16 bytes per lane (the accumulator layout gives sixteen
//     32-byte pieces per store instruction; with one workgroup per CU nothing overlaps that tail);
//   * dQ wave: delta = rowsum(dO o O) on v_dot2c_f32_bf16, zero fill only on the partial tile.
//
// What was measured and NOT kept (same file history, profiles/r05_attention_ablations_and_arms.txt): running phase 2 of waves
// 4 .. 6 one step late under their SIMD partner's phase 1 (+3 % time; every ablation of this kernel removes about its part's
// own issue time -- the parts add up -- although the chip can hide matrix instructions behind the other wave's plain vector
// instructions: scripts/probes/mfma_valu_overlap.hip.  Its packed fp32 lines (soft_bwd) are one suspect: packed fp32 does not
// overlap with v_mfma; the scalar form of those lines spilled 20 - 60 registers at the 256-register limit); staging the
// query tiles from waves 0 .. 3 with wave 7 touching the lines into L2 (the 13 extra live registers made the compiler
// spill the V fragments and the staged chunks: 2 x slower).
//
// Both cover 256 < Lk <= 448 without a per-element bias (the BEV encoder's 441 cells); everything else stays on attn_bwd1.
#include "attn_bwd7p1.h"

template <int GEN, bool DROP, bool KMASK>
__global__ __launch_bounds__(512, 2) void attn_bwd7p1_kernel(AttnArgs a) {
  typedef B2Lds L;
  extern __shared__ __attribute__((aligned(16))) unsigned char b2_smem[];
  bf16_raw* const s_k = reinterpret_cast<bf16_raw*>(b2_smem + L::k_off);
  bf16_raw* const s_ds = reinterpret_cast<bf16_raw*>(b2_smem + L::ds_off);
  bf16_raw* const s_q = reinterpret_cast<bf16_raw*>(b2_smem + L::q_off);
  bf16_raw* const s_do = reinterpret_cast<bf16_raw*>(b2_smem + L::do_off);
  float* const s_stat = reinterpret_cast<float*>(b2_smem + L::stat_off);

  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.x, b = bh / a.nh, h = bh - b * a.nh;
  const bf16_raw* qp = (const bf16_raw*)a.q + (size_t)b * a.bsq + h * ATTN_D;
  const bf16_raw* kp = (const bf16_raw*)a.k + (size_t)b * a.bsk + h * ATTN_D;
  const bf16_raw* vp = (const bf16_raw*)a.v + (size_t)b * a.bsv + h * ATTN_D;
  const bf16_raw* op = (const bf16_raw*)a.o + (size_t)b * a.bso + h * ATTN_D;
  const bf16_raw* dop = (const bf16_raw*)a.dout + (size_t)b * a.bso + h * ATTN_D;
  const float sc2 = a.scale * LOG2E;
  const float inv_ks = DROP ? 1.0f / a.keep_scale : 1.0f;
  const float out_ks = DROP ? a.keep_scale : 1.0f;
  const float dq_scale = a.scale * out_ks;
  const int nsteps = (a.Lq + 31) >> 5;
  // Two places follow each generation's two-file form so that every instance keeps its instruction text: where the dQ
  // wave's test is computed (the order at the top of the kernel follows the statement order), and GEN 2's K stores,
  // written out in place (through k_to_lds they cost it two or three address instructions).
  bool is_dq_wave;
  if constexpr (GEN == 2) is_dq_wave = (w == B2_NKEYW);

  // ---- prologue, all waves: K -> LDS row-major, zero rows beyond Lk.  GEN 2 stores the chunks at once; in GEN 3 they stay
  //      in registers until each wave has issued its other first loads as well
  constexpr int KCH = B2_NK * 8 / 512;            // 16-byte chunks of K per thread (7)
  uint4 kbuf[KCH];
#pragma unroll
  for (int i = 0; i < KCH; ++i) {
    const int c16 = tid + i * 512, row = c16 >> 3, ch = c16 & 7;
    kbuf[i] = make_uint4(0, 0, 0, 0);
    if (row < a.Lk) kbuf[i] = ld_frag_global(kp, a.ldk, row, ch * 8);
  }
  auto k_to_lds = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int c16 = tid + i * 512, row = c16 >> 3, ch = c16 & 7;
      *reinterpret_cast<uint4*>(s_k + row * LDT + ch * 8) = kbuf[i];
    }
  };
  if constexpr (GEN == 2) {
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int c16 = tid + i * 512, row = c16 >> 3, ch = c16 & 7;
      *reinterpret_cast<uint4*>(s_k + row * LDT + ch * 8) = kbuf[i];
    }
  } else {
    is_dq_wave = (w == B2_NKEYW);
  }

  if (is_dq_wave) {
    // =====================================================================================================
    // dQ wave: staging of the 32-query tiles and dQ^T = K^T dS^T one step behind the key waves
    // =====================================================================================================
    const int ldq = (int)a.ldq, ldo = (int)a.ldo;           // 32-bit element offsets: a (batch, head) slice is far below 2^31 elements
    if constexpr (GEN == 3) __builtin_amdgcn_s_setprio(3);   // one wave, 1/5 of the matrix work, on a SIMD it shares with a key wave
    // dQ^T[64 d][32 q] += K^T dS^T over all 448 key rows of the images (rows beyond Lk are zero in both), 14 k-steps of
    // 32 keys.  One wave has nobody to hide its LDS round trips behind and gets a fraction of the LDS issue rate (a lone
    // wave issues an 8-byte LDS read every ~10 cycles at best; r03e timeline: 168 transposing reads per step = 4 300
    // cycles), so (1) the K^T fragments of the upper NRES k-steps live in registers for the whole kernel (the wave owns no
    // accumulators), (2) the reads of k-step ks + 1 are issued before the matrix instructions of k-step ks (explicit
    // two-deep software pipeline).
    constexpr int NKS = 2 * B2_NKEYW, NRES = 3;
    struct DqFrags { bf16x8 ka[4], d0, d1; };
    auto dq_load = [&](DqFrags& f, const bf16_raw* img, int ks) __attribute__((always_inline)) {
      f.d0 = lds_frag_tr(img, B2_LDS_DS, 32 * ks + 8 * g, 32 * ks + 8 * g + 4, 0, lane);
      f.d1 = lds_frag_tr(img, B2_LDS_DS, 32 * ks + 8 * g, 32 * ks + 8 * g + 4, 16, lane);
      if (ks < NKS - NRES) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) f.ka[dt] = lds_frag_tr(s_k, LDT, 32 * ks + 8 * g, 32 * ks + 8 * g + 4, 16 * dt, lane);
      }
    };
    bf16x8 kres[NRES][4];
    auto dq_mma = [&](f32x4 (&acc)[2][4], const DqFrags& f, int ks) __attribute__((always_inline)) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 ka = ks < NKS - NRES ? f.ka[dt] : kres[ks - (NKS - NRES) < 0 ? 0 : ks - (NKS - NRES)][dt];
        acc[0][dt] = mfma16(ka, f.d0, acc[0][dt]);
        acc[1][dt] = mfma16(ka, f.d1, acc[1][dt]);
      }
    };
    // staging: lane owns 16-byte chunks ch = lane + 64 i (i = 0..3): row ch >> 3, dims 8 (ch & 7) .. + 7; a row is covered
    // by 8 neighbouring lanes.  Both generations' pairs are defined (a lambda of an `if constexpr` block would end with
    // it); the pair a generation does not call compiles away.  The call sites choose, not a common wrapper: GEN 3 keeps its
    // text only with the loop over the pieces in the kernel body, GEN 2 only with it inside tile_issue / tile_commit.
    uint4 qreg[4], doreg[4], oreg[4];
    float lreg = INFINITY;
    const int row0 = lane >> 3, dcol = (lane & 7) * 8;      // chunk i of this lane: row row0 + 8 i, dims dcol .. dcol + 7
    // ---- GEN 2: a whole tile per call, per-chunk masks, delta by shift-and-multiply
    uint32_t okm[4];
    const bf16_raw* qlane = qp + dcol;
    const bf16_raw* dolane = dop + dcol;
    const bf16_raw* olane = op + dcol;
    auto tile_issue = [&](int q0) __attribute__((always_inline)) {      // loads only: nothing here may consume a loaded value (that would wait for all of them)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int row = q0 + row0 + 8 * i;
        const bool ok = row < a.Lq;
        row = ok ? row : a.Lq - 1;                          // rows past the end: clamped load, zeroed below
        okm[i] = ok ? 0xffffffffu : 0u;                     // applied when the tile is committed (touching a loaded value
        qreg[i] = *reinterpret_cast<const uint4*>(qlane + row * ldq);      // here would wait for the loads right away)
        doreg[i] = *reinterpret_cast<const uint4*>(dolane + row * ldo);
        oreg[i] = *reinterpret_cast<const uint4*>(olane + row * ldo);
      }
      lreg = INFINITY;                            // padding rows: p = exp2(-inf) = 0
      if (lane < 32 && q0 + lane < a.Lq) lreg = a.lse[((size_t)b * a.nh + h) * a.Lq + q0 + lane];
    };
    auto tile_commit = [&](int buf) __attribute__((always_inline)) {
      bf16_raw* tq = s_q + buf * (32 * LDT);
      bf16_raw* tdo = s_do + buf * (32 * LDT);
      float* st = s_stat + buf * 64;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ch = lane + i * 64, row = ch >> 3, d0 = (ch & 7) * 8;
        const uint32_t m = okm[i];                          // rows past the end are zero filled
        const uint4 qv = make_uint4(qreg[i].x & m, qreg[i].y & m, qreg[i].z & m, qreg[i].w & m);
        const uint4 dv = make_uint4(doreg[i].x & m, doreg[i].y & m, doreg[i].z & m, doreg[i].w & m);
        *reinterpret_cast<uint4*>(tq + row * LDT + d0) = qv;
        *reinterpret_cast<uint4*>(tdo + row * LDT + d0) = dv;
        const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w};
        const uint32_t ow[4] = {oreg[i].x, oreg[i].y, oreg[i].z, oreg[i].w};
        float dsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dsum += __uint_as_float(dw[j] << 16) * __uint_as_float(ow[j] << 16) +
                  __uint_as_float(dw[j] & 0xffff0000u) * __uint_as_float(ow[j] & 0xffff0000u);
        dsum = sum8(dsum);
        if ((lane & 7) == 0) st[32 + row] = dsum * inv_ks;
      }
      if (lane < 32) st[lane] = lreg * LOG2E;
    };
    // ---- GEN 3: chunk by chunk.  (Threading these pieces through dq_step's k-steps -- loads on the first four, commits
    //      on the last four -- measured 13 % SLOWER, r05l: the branches cut its software pipeline into ten basic blocks.)
    auto issue_piece = [&](int i, int q0) __attribute__((always_inline)) {      // loads only
      int row = q0 + row0 + 8 * i;
      row = row < a.Lq ? row : a.Lq - 1;                    // rows past the end: clamped load, zeroed when committed
      qreg[i] = *reinterpret_cast<const uint4*>(qp + dcol + row * ldq);
      doreg[i] = *reinterpret_cast<const uint4*>(dop + dcol + row * ldo);
      oreg[i] = *reinterpret_cast<const uint4*>(op + dcol + row * ldo);
      if (i == 3) {
        lreg = INFINITY;                          // padding rows: p = exp2(-inf) = 0
        if (lane < 32 && q0 + lane < a.Lq) lreg = a.lse[((size_t)b * a.nh + h) * a.Lq + q0 + lane];
      }
    };
    auto commit_piece = [&](int i, int buf, int q0) __attribute__((always_inline)) {
      bf16_raw* tq = s_q + buf * (32 * LDT);
      bf16_raw* tdo = s_do + buf * (32 * LDT);
      float* st = s_stat + buf * 64;
      const int ch = lane + i * 64, row = ch >> 3, d0 = (ch & 7) * 8;
      uint4 qv = qreg[i], dv = doreg[i];
      if (q0 + 32 > a.Lq) {                                 // only the last tile has rows past the end (wave-uniform): zero fill
        const uint32_t m = q0 + row < a.Lq ? 0xffffffffu : 0u;
        qv = make_uint4(qv.x & m, qv.y & m, qv.z & m, qv.w & m);
        dv = make_uint4(dv.x & m, dv.y & m, dv.z & m, dv.w & m);
      }
      *reinterpret_cast<uint4*>(tq + row * LDT + d0) = qv;
      *reinterpret_cast<uint4*>(tdo + row * LDT + d0) = dv;
      // delta = rowsum(dO o O): v_dot2c_f32_bf16 multiplies two packed pairs and accumulates in fp32 (products of bf16
      // values are exact in fp32); the 8 lanes of a row are neighbours: one DPP sum
      float dsum = dot2_bf16(dv.x, oreg[i].x, 0.f);
      dsum = dot2_bf16(dv.y, oreg[i].y, dsum);
      dsum = dot2_bf16(dv.z, oreg[i].z, dsum);
      dsum = dot2_bf16(dv.w, oreg[i].w, dsum);
      dsum = sum8(dsum);
      if ((lane & 7) == 0) st[32 + row] = dsum * inv_ks;
      if (i == 3 && lane < 32) st[lane] = lreg * LOG2E;
    };
    auto dq_step = [&](int q0, int buf) __attribute__((always_inline)) {
      const bf16_raw* img = s_ds + buf * (B2_NK * B2_LDS_DS);
      f32x4 dqacc[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dqacc[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      DqFrags fa, fb;
      dq_load(fa, img, 0);
#pragma unroll
      for (int ks = 0; ks < NKS; ks += 2) {
        dq_load(fb, img, ks + 1);
        __builtin_amdgcn_sched_barrier(0);
        dq_mma(dqacc, fa, ks);
        if (ks + 2 < NKS) dq_load(fa, img, ks + 2);
        __builtin_amdgcn_sched_barrier(0);
        dq_mma(dqacc, fb, ks + 1);
      }
      // lane (query = q0 + 16 qt + c) holds dQ^T[d = 16 dt + 4 g + r][query]
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int qi = q0 + qt * 16 + c;
        if (qi < a.Lq) {
          bf16_raw* dqp = (bf16_raw*)a.dq + (size_t)b * a.bsq + (size_t)qi * a.ldq + h * ATTN_D + 4 * g;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            st4<bf16_raw>(dqp + 16 * dt, make_float4(dqacc[qt][dt][0] * dq_scale, dqacc[qt][dt][1] * dq_scale,
                                                     dqacc[qt][dt][2] * dq_scale, dqacc[qt][dt][3] * dq_scale));
        }
      }
    };

    if constexpr (GEN == 2) {
      tile_issue(0);
      tile_commit(0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) issue_piece(i, 0);
      k_to_lds();
#pragma unroll
      for (int i = 0; i < 4; ++i) commit_piece(i, 0, 0);
    }
    __syncthreads();                                   // K image and tile 0 visible
#pragma unroll
    for (int i = 0; i < NRES; ++i)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int ks = NKS - NRES + i;
        kres[i][dt] = lds_frag_tr(s_k, LDT, 32 * ks + 8 * g, 32 * ks + 8 * g + 4, 16 * dt, lane);
      }
    for (int k = 0; k < nsteps; ++k) {
      const bool more = k + 1 < nsteps;
      if (more) {
        if constexpr (GEN == 2) {
          tile_issue(32 * (k + 1));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) issue_piece(i, 32 * (k + 1));
        }
      }
      if (k > 0) dq_step(32 * (k - 1), (k - 1) & 1);
      if (more) {
        if constexpr (GEN == 2) {
          tile_commit((k + 1) & 1);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) commit_piece(i, (k + 1) & 1, 32 * (k + 1));
        }
      }
      __syncthreads();                                 // closes step k
    }
    dq_step(32 * (nsteps - 1), (nsteps - 1) & 1);
    return;
  }

  // =====================================================================================================
  // key waves
  // =====================================================================================================
  const int key0 = w * 64;
  const bool has_keys = key0 < a.Lk;
  float mask2[4];
  bf16x8 vf[4][2];             // V fragments (B operand of dP), resident
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int key = key0 + kt * 16 + c;
    const int r = key < a.Lk ? key : a.Lk - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) vf[kt][ks] = as_bf16x8(ld_frag_global(vp, a.ldv, r, ks * 32 + g * 8));   // (unused rows: clamped)
    mask2[kt] = 0.f;
    if (KMASK) mask2[kt] = key < a.Lk ? a.key_mask[(size_t)b * a.Lk + key] * LOG2E : -INFINITY;
  }
  if constexpr (GEN == 3) k_to_lds();

  f32x4 dkacc[4][4], dvacc[4][4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dkacc[kt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dvacc[kt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  // keep bits, lanes <-> keys: 32 words (tt, kt, r) per (32-query block, 64-key tile of one wave), see attn_common.h
  bb_cu64p wbits = nullptr;
  const size_t bits_step = (size_t)a.nk64 * 32;         // words per 32-query block
  if (DROP) wbits = (bb_cu64p)(uintptr_t)(a.drop_bits_b + (size_t)bh * (a.nq16 >> 1) * bits_step + (size_t)w * 32);
  if (!has_keys) {      // no keys (Lk <= 384): this wave's rows of both dS images stay zero for the dQ contraction
    for (int i = lane; i < 64 * B2_LDS_DS / 4; i += 64) {
      reinterpret_cast<uint2*>(s_ds + key0 * B2_LDS_DS)[i] = make_uint2(0u, 0u);
      reinterpret_cast<uint2*>(s_ds + (B2_NK + key0) * B2_LDS_DS)[i] = make_uint2(0u, 0u);
    }
  }

  if constexpr (GEN == 2) {
    // ---- key waves, generation 2: one pass over the four key tiles per step
    // keep-bit words travel one key tile ahead of their use (every word is read once: each scalar load is a cache miss
    // with an L2 / HBM round trip; issued right in front of its first use that latency was fully exposed, 1 100 cycles per
    // key tile in the r03h timeline)
    uint64_t bw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bw[i] = (DROP && has_keys) ? wbits[(i >> 2) * 16 + (i & 3)] : 0;
    __syncthreads();                                       // K image and tile 0 visible
    for (int k = 0; k < nsteps; ++k) {
      const int buf = k & 1;
      const bf16_raw* tq = s_q + buf * (32 * LDT);
      const bf16_raw* tdo = s_do + buf * (32 * LDT);
      const float* st = s_stat + buf * 64;
      bf16_raw* img = s_ds + buf * (B2_NK * B2_LDS_DS);
      if (has_keys) {
        // A operands of S / dP: the rows of both query tiles, read once per step
        bf16x8 qa[2][2], da[2][2];
        float nl[2][4];
        f32x4 ndl[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            qa[tt][ks] = lds_frag_rows(tq, tt, ks, lane);
            da[tt][ks] = lds_frag_rows(tdo, tt, ks, lane);
          }
          const float4 l4 = *reinterpret_cast<const float4*>(&st[tt * 16 + g * 4]);
          const float4 d4 = *reinterpret_cast<const float4*>(&st[32 + tt * 16 + g * 4]);
          nl[tt][0] = -l4.x; nl[tt][1] = -l4.y; nl[tt][2] = -l4.z; nl[tt][3] = -l4.w;      // -lse (log2 domain)
          ndl[tt] = (f32x4){-d4.x, -d4.y, -d4.z, -d4.w};                                     // -delta / ks
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const bf16x8 vf0 = vf[kt][0], vf1 = vf[kt][1];
          uint64_t bwn[8];
          if (DROP) {     // next key tile's words (tile 0 of the next step after tile 3; the workspace has nq16 / 2 >= nsteps blocks)
            const int kn = kt == 3 ? (k + 1 < nsteps ? k + 1 : k) : k, ktn = (kt + 1) & 3;
#pragma unroll
            for (int i = 0; i < 8; ++i) bwn[i] = wbits[(size_t)kn * bits_step + (i >> 2) * 16 + ktn * 4 + (i & 3)];
            __builtin_amdgcn_sched_barrier(0);      // the loads stay HERE, ahead of this tile's arithmetic
          }
          const bf16x8 kf0 = lds_frag_rows(s_k, w * 4 + kt, 0, lane), kf1 = lds_frag_rows(s_k, w * 4 + kt, 1, lane);
          // lane (key = key0 + 16 kt + c) holds S[q = 32 k + 16 tt + 4 g + r][key], r = 0..3; the two query tiles are two
          // independent chains (matrix -> exp -> select -> pack) in flight together
          f32x4 sacc[2], dpacc[2];
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            sacc[tt] = mfma16(qa[tt][0], kf0, (f32x4){0.f, 0.f, 0.f, 0.f});
            sacc[tt] = mfma16(qa[tt][1], kf1, sacc[tt]);
            dpacc[tt] = mfma16(da[tt][0], vf0, DROP ? (f32x4){0.f, 0.f, 0.f, 0.f} : ndl[tt]);
            dpacc[tt] = mfma16(da[tt][1], vf1, dpacc[tt]);
          }
          uint2 dsu[2], pdu[2];
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            float dsv[4], pdv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float off = KMASK ? mask2[kt] + nl[tt][r] : nl[tt][r];
              const float p = fast_exp2(fmaf(sacc[tt][r], sc2, off));
              if (DROP) {
                const float pd = keep_select(p, bw[tt * 4 + r]);
                dsv[r] = fmaf(pd, dpacc[tt][r], p * ndl[tt][r]);            // P keep dP - P delta / ks
                pdv[r] = pd;
              } else {
                dsv[r] = p * dpacc[tt][r];                                  // dP' = dP - delta came out of the matrix unit
                pdv[r] = p;
              }
            }
            dsu[tt] = make_uint2(pack_bf16x2(dsv[0], dsv[1]), pack_bf16x2(dsv[2], dsv[3]));
            pdu[tt] = make_uint2(pack_bf16x2(pdv[0], pdv[1]), pack_bf16x2(pdv[2], pdv[3]));
            // dS image [key][query]: this lane's 4 consecutive queries of tile tt at row key
            *reinterpret_cast<uint2*>(img + (key0 + kt * 16 + c) * B2_LDS_DS + 16 * tt + 4 * g) = dsu[tt];
          }
          // B operands of the "contract over queries" products: k-slot (g, j) <-> query 16 (j >> 2) + 4 g + (j & 3)
          const bf16x8 dsb = as_bf16x8(make_uint4(dsu[0].x, dsu[0].y, dsu[1].x, dsu[1].y));
          const bf16x8 pdb = as_bf16x8(make_uint4(pdu[0].x, pdu[0].y, pdu[1].x, pdu[1].y));
          // dK^T += Q^T dS, dV^T += dO^T P right away (A operands: rows d, k-slots = the 32 queries, by transposing reads):
          // these eight matrix instructions run under the next key tile's dependent chain
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const bf16x8 qtf = lds_frag_tr(tq, LDT, 4 * g, 16 + 4 * g, dt * 16, lane);
            const bf16x8 dotf = lds_frag_tr(tdo, LDT, 4 * g, 16 + 4 * g, dt * 16, lane);
            dkacc[kt][dt] = mfma16(qtf, dsb, dkacc[kt][dt]);
            dvacc[kt][dt] = mfma16(dotf, pdb, dvacc[kt][dt]);
          }
          if (DROP) {
#pragma unroll
            for (int i = 0; i < 8; ++i) bw[i] = bwn[i];
          }
        }
      }
      __syncthreads();                                     // closes step k
    }

    // ---- epilogue: dK = scale * ks * dK^T, dV = ks * dV^T
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int key = key0 + kt * 16 + c;
      if (key < a.Lk) {
        bf16_raw* dkp = (bf16_raw*)a.dk + (size_t)b * a.bsk + (size_t)key * a.ldk + h * ATTN_D;
        bf16_raw* dvp = (bf16_raw*)a.dv + (size_t)b * a.bsv + (size_t)key * a.ldv + h * ATTN_D;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          st4<bf16_raw>(dkp + dt * 16 + g * 4,
                        make_float4(dkacc[kt][dt][0] * dq_scale, dkacc[kt][dt][1] * dq_scale, dkacc[kt][dt][2] * dq_scale,
                                    dkacc[kt][dt][3] * dq_scale));
          st4<bf16_raw>(dvp + dt * 16 + g * 4, make_float4(dvacc[kt][dt][0] * out_ks, dvacc[kt][dt][1] * out_ks,
                                                           dvacc[kt][dt][2] * out_ks, dvacc[kt][dt][3] * out_ks));
        }
      }
    }
  } else {
    // ---- key waves, generation 3: two phases per step
    uint64_t bw[32];
    bb_cu64p wnext = wbits;
#pragma unroll
    for (int i = 0; i < 32; ++i) bw[i] = (DROP && has_keys) ? wnext[i] : 0;

    // softmax backward of one chain (key tile x 16-query tile): 4 score elements per lane, P / dS stay in their lanes
    auto soft_bwd = [&](const f32x4& sacc, const f32x4& dpacc, const float (&nl)[4], const f32x4& ndl, float mk,
                        const uint64_t* bwords, uint2& dsu, uint2& pdu) __attribute__((always_inline)) {
      // Two elements per instruction where the operation allows (v_pk_fma_f32 / v_pk_mul_f32: the accumulator quad is two
      // register pairs): scale-and-shift, P delta, and the final multiply-add -- 1.5 instead of 3 instruction slots per
      // element; the exponential and the keep select stay per element.
      uint32_t dsw[2], pdw[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bb_f32x2 s2 = {sacc[2 * j], sacc[2 * j + 1]}, d2 = {dpacc[2 * j], dpacc[2 * j + 1]};
        const bb_f32x2 o2 = {KMASK ? mk + nl[2 * j] : nl[2 * j], KMASK ? mk + nl[2 * j + 1] : nl[2 * j + 1]};
        const bb_f32x2 t2 = s2 * sc2 + o2;
        const bb_f32x2 p2 = {fast_exp2(t2[0]), fast_exp2(t2[1])};
        bb_f32x2 ds2, pd2;
        if (DROP) {
          pd2 = (bb_f32x2){keep_select(p2[0], bwords[2 * j]), keep_select(p2[1], bwords[2 * j + 1])};
          const bb_f32x2 n2 = {ndl[2 * j], ndl[2 * j + 1]};
          ds2 = pd2 * d2 + p2 * n2;                           // P keep dP - P delta / ks
        } else {
          pd2 = p2;
          ds2 = p2 * d2;                                      // dP' = dP - delta came out of the matrix unit
        }
        dsw[j] = pack_bf16x2(ds2[0], ds2[1]);
        pdw[j] = pack_bf16x2(pd2[0], pd2[1]);
      }
      dsu = make_uint2(dsw[0], dsw[1]);
      pdu = make_uint2(pdw[0], pdw[1]);
    };
    __syncthreads();                                       // K image and tile 0 visible

    for (int k = 0; k < nsteps; ++k) {
      const int buf = k & 1;
      const bf16_raw* tq = s_q + buf * (32 * LDT);
      const bf16_raw* tdo = s_do + buf * (32 * LDT);
      const float* st = s_stat + buf * 64;
      bf16_raw* img = s_ds + buf * (B2_NK * B2_LDS_DS);
      if (has_keys) {
        uint2 dsu[4][2], pdu[4][2];
        // ---- phase 1: two-deep software pipeline over the chains i = (tt, kt); a scheduling barrier after each chain keeps
        //      the compiler from hoisting every chain's LDS reads to the top (that version needed 290 registers)
        bf16x8 qa0, qa1, da0, da1, qb0, qb1, db0, db1;
        float nl[4], nlb[4];
        f32x4 ndl, ndlb;
        auto load_rows = [&](int tt, bf16x8& q0, bf16x8& q1, bf16x8& d0, bf16x8& d1, float (&l)[4], f32x4& dl)
                             __attribute__((always_inline)) {
          q0 = lds_frag_rows(tq, tt, 0, lane); q1 = lds_frag_rows(tq, tt, 1, lane);
          d0 = lds_frag_rows(tdo, tt, 0, lane); d1 = lds_frag_rows(tdo, tt, 1, lane);
          const float4 l4 = *reinterpret_cast<const float4*>(&st[tt * 16 + g * 4]);
          const float4 d4 = *reinterpret_cast<const float4*>(&st[32 + tt * 16 + g * 4]);
          l[0] = -l4.x; l[1] = -l4.y; l[2] = -l4.z; l[3] = -l4.w;               // -lse (log2 domain)
          dl = (f32x4){-d4.x, -d4.y, -d4.z, -d4.w};                             // -delta / ks
        };
        auto chain_mma = [&](int kt, const bf16x8& q0, const bf16x8& q1, const bf16x8& d0, const bf16x8& d1, const f32x4& dl,
                             f32x4& sacc, f32x4& dpacc) __attribute__((always_inline)) {
          const bf16x8 kf0 = lds_frag_rows(s_k, w * 4 + kt, 0, lane), kf1 = lds_frag_rows(s_k, w * 4 + kt, 1, lane);
          sacc = mfma16(q0, kf0, (f32x4){0.f, 0.f, 0.f, 0.f});
          sacc = mfma16(q1, kf1, sacc);
          dpacc = mfma16(d0, vf[kt][0], DROP ? (f32x4){0.f, 0.f, 0.f, 0.f} : dl);
          dpacc = mfma16(d1, vf[kt][1], dpacc);
        };
        load_rows(0, qa0, qa1, da0, da1, nl, ndl);
        f32x4 sa, dpa, sb, dpb;
        chain_mma(0, qa0, qa1, da0, da1, ndl, sa, dpa);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int tt = i >> 2, kt = i & 3;
          if (i == 3) load_rows(1, qb0, qb1, db0, db1, nlb, ndlb);
          if (i < 7) {               // chain i + 1's matrix instructions
            const int ktn = (i + 1) & 3;
            if (i + 1 < 4) chain_mma(ktn, qa0, qa1, da0, da1, ndl, (i & 1) ? sa : sb, (i & 1) ? dpa : dpb);
            else chain_mma(ktn, qb0, qb1, db0, db1, ndlb, (i & 1) ? sa : sb, (i & 1) ? dpa : dpb);
          }
          const uint64_t* bcur = bw + tt * 16 + kt * 4;      // chain i's vector arithmetic
          if (tt == 0) soft_bwd((i & 1) ? sb : sa, (i & 1) ? dpb : dpa, nl, ndl, mask2[kt], bcur, dsu[kt][tt], pdu[kt][tt]);
          else soft_bwd((i & 1) ? sb : sa, (i & 1) ? dpb : dpa, nlb, ndlb, mask2[kt], bcur, dsu[kt][tt], pdu[kt][tt]);
          __builtin_amdgcn_sched_barrier(0);
        }
        // ---- phase 2: dK^T += Q^T dS, dV^T += dO^T P, d-tile outermost; A operands rows d, k-slots = the 32 queries (g, j) <->
        //      query 16 (j >> 2) + 4 g + (j & 3), fragments read one d-tile ahead.  Program order: first d-tile's fragments,
        //      THEN the dS image (transposing reads may not be hoisted over LDS stores the compiler cannot prove disjoint)
        bf16x8 fq = lds_frag_tr(tq, LDT, 4 * g, 16 + 4 * g, 0, lane), fdo = lds_frag_tr(tdo, LDT, 4 * g, 16 + 4 * g, 0, lane);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
            *reinterpret_cast<uint2*>(img + (key0 + kt * 16 + c) * B2_LDS_DS + 16 * tt + 4 * g) = dsu[kt][tt];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          bf16x8 fqn = fq, fdon = fdo;
          if (dt < 3) {
            fqn = lds_frag_tr(tq, LDT, 4 * g, 16 + 4 * g, (dt + 1) * 16, lane);
            fdon = lds_frag_tr(tdo, LDT, 4 * g, 16 + 4 * g, (dt + 1) * 16, lane);
          }
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) {
            const bf16x8 dsb = as_bf16x8(make_uint4(dsu[kt][0].x, dsu[kt][0].y, dsu[kt][1].x, dsu[kt][1].y));
            const bf16x8 pdb = as_bf16x8(make_uint4(pdu[kt][0].x, pdu[kt][0].y, pdu[kt][1].x, pdu[kt][1].y));
            dkacc[kt][dt] = mfma16(fq, dsb, dkacc[kt][dt]);
            dvacc[kt][dt] = mfma16(fdo, pdb, dvacc[kt][dt]);
          }
          fq = fqn;
          fdo = fdon;
        }
      }
      // ---- closes step k: this wave's LDS stores have landed (the pointer operand ties the scalar loads below to this
      //      point: loads from the constant address space would otherwise be free to move up), the next step's keep-bit
      //      words are requested, then the bare barrier -- an acquire fence would wait for the scalar loads first
      __builtin_amdgcn_sched_barrier(0);
      if (DROP && has_keys) {
        wnext = wbits + (size_t)(k + 1 < nsteps ? k + 1 : k) * bits_step;
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(wnext) : : "memory");
#pragma unroll
        for (int i = 0; i < 32; ++i) bw[i] = wnext[i];
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");
      }
      __builtin_amdgcn_s_barrier();
      asm volatile("" : : : "memory");
    }

    // ---- epilogue: dK = scale * ks * dK^T, dV = ks * dV^T as whole 128-byte rows.  Each wave transposes through LDS it
    //      owns: its 64 rows of the dS buffer the dQ wave is NOT reading during its last contraction (buffer nsteps & 1,
    //      last read before the final barrier) hold exactly a [32 keys][72] bf16 tile; four passes (dK / dV x key-tile
    //      pair), each 8 ds_write_b64 + 4 ds_read_b128 + 4 global_store_dwordx4.  A wave's LDS operations execute in order.
    if (has_keys) {
      bf16_raw* stg = s_ds + (nsteps & 1) * (B2_NK * B2_LDS_DS) + key0 * B2_LDS_DS;
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int hp = pass & 1;
        const bool is_dk = pass < 2;
        const float sc = is_dk ? dq_scale : out_ks;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const f32x4 v = is_dk ? dkacc[2 * hp + kk][dt] : dvacc[2 * hp + kk][dt];
            *reinterpret_cast<uint2*>(stg + (kk * 16 + c) * 72 + dt * 16 + g * 4) =
                make_uint2(pack_bf16x2(v[0] * sc, v[1] * sc), pack_bf16x2(v[2] * sc, v[3] * sc));
          }
        bf16_raw* dst = (bf16_raw*)(is_dk ? a.dk : a.dv) + (size_t)b * (is_dk ? a.bsk : a.bsv) + h * ATTN_D;
        const int64_t ld = is_dk ? a.ldk : a.ldv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ch = lane + 64 * j, row = ch >> 3, d0 = (ch & 7) * 8;
          const uint4 val = *reinterpret_cast<const uint4*>(stg + row * 72 + d0);
          const int key = key0 + hp * 32 + row;
          if (key < a.Lk) *reinterpret_cast<uint4*>(dst + (size_t)key * ld + d0) = val;
        }
      }
    }
  }
}

// =============================================================================================
// launcher
// =============================================================================================
template <int GEN, bool D_, bool M_>
static int launch_bwd7p1(const AttnArgs& a, hipStream_t st) {
  static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd7p1_kernel<GEN, D_, M_>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, B2Lds::bytes) == hipSuccess;
  BB_REQUIRE(ok, "attention bwd (7+1 waves%s): cannot raise the dynamic LDS limit to %d bytes", GEN == 3 ? ", gen 3" : "",
             B2Lds::bytes);
  hipLaunchKernelGGL((attn_bwd7p1_kernel<GEN, D_, M_>), dim3((unsigned)a.B * a.nh), dim3(512), B2Lds::bytes, st, a);
  BB_CHECK_LAUNCH(GEN == 3 ? "attn_bwd(7+1 waves, gen 3)" : "attn_bwd(7+1 waves)");
  return BB_OK;
}

template <int GEN>
static int attn_bwd7p1(const AttnArgs& a, hipStream_t st) {
  BB_REQUIRE(attn_mfma_operands_aligned(a, true), "attention bwd (MFMA path): " ATTN_MFMA_ALIGN_MSG);
  const bool hd = a.drop_p > 0.f, km = a.key_mask != nullptr;
  if (hd) return km ? launch_bwd7p1<GEN, true, true>(a, st) : launch_bwd7p1<GEN, true, false>(a, st);
  return km ? launch_bwd7p1<GEN, false, true>(a, st) : launch_bwd7p1<GEN, false, false>(a, st);
}

// one predicate under two names: both generations cover the same calls
bool attn_bwd3_supported(const AttnArgs& a) {
  return a.bias == nullptr && a.Lk > 256 && a.Lk <= B2_NK && (a.drop_p <= 0.f || a.drop_bits_b != nullptr);
}
bool attn_bwd2_supported(const AttnArgs& a) { return attn_bwd3_supported(a); }

int attn_bwd2(const AttnArgs& a, hipStream_t st) { return attn_bwd7p1<2>(a, st); }
int attn_bwd3(const AttnArgs& a, hipStream_t st) { return attn_bwd7p1<3>(a, st); }
