// Attention forward with float16 operands (fp16 q, k, v, o; fp32 accumulation): the attention of the CLIP image encoder's
// float16 mode (clip_vit.py), where the reference runs the converted fp16 network.  Inference only: no key mask, no bias,
// no dropout, no log-sum-exp; an entry of its own (bevbert_attn_f16_fwd), outside the dispatch plan of bevbert_attn_fwd.
//
// Formulation and schedule are those of the second-generation bf16 forward (attn_fwd2.hip):
//   S^T = K Q^T  (lane q = l & 15 holds S[q][key = 16 t + 4 g + r]),   O^T = V^T P^T  (P goes D -> B operand in place)
// with v_mfma_f32_16x16x32_f16, 64-key tiles streamed through a double-buffered LDS image, an online softmax with the
// lazy running maximum, workgroups of 4 waves x 32 queries.  Any Lq, Lk >= 1: keys past Lk enter as -inf through the C
// operand of the first Q K^T instruction of their tile, query rows past Lq are computed on a clamped row and not stored.
//
// Rounding:
//   * scores, the running maximum and the row sum are fp32; the row sum adds the UNROUNDED probabilities;
//   * P = exp2(s * scale * log2e - m) is rounded to fp16 to nearest even (v_cvt_pk_f16_f32) for the P V product.  m lags the
//     true maximum by at most F16_THR, so P <= 2^F16_THR = 32, far from fp16's 65504; and a lagging m only makes P LARGER
//     than exp(s - max), so a probability that is a normal fp16 number relative to its row maximum (>= 2^-14) stays one;
//   * O = (sum_j P_j V_j) * (1 / l): the reciprocal is an IEEE fp32 division, the product one fp32 multiply (2 ulp of fp32
//     together, 2^-12 of an fp16 ulp), then ONE rounding to fp16 -- overflow gives inf as IEEE fp16 does, nothing saturates.
#include "attn_mfma_common.h"

#define F16_THR 5.0f
// K / V tiles: [64 rows][64 halves] at a row stride of 72 elements (144 B), the layout attn_fwd2.hip measured as its best
#define FH_LD 72
#define FH_TILE (TK * FH_LD)
#define FH_NW 4       // waves per workgroup, 32 queries each

// the tiles are moved as raw 16-bit words (the staging and the transposing read never interpret them)
typedef bf16_raw h16_raw;
__device__ __forceinline__ int fh_off(int row, int chunk) { return row * FH_LD + (chunk << 3); }
__device__ __forceinline__ f16x8 fh_frag_rows(const h16_raw* tile, int t, int ks, int lane) {
  return as_f16x8(*reinterpret_cast<const uint4*>(tile + fh_off(t * 16 + (lane & 15), ks * 4 + (lane >> 4))));
}
// fragment whose eight k-slots of lane group g are image rows row_lo + (0..3) and row_hi + (0..3), at columns col0 .. +15
__device__ __forceinline__ f16x8 fh_frag_tr(const h16_raw* img, int row_lo, int row_hi, int col0, int lane) {
  const int i = lane & 15, col = col0 + 4 * (i & 3);
  const int rl = row_lo + (i >> 2), rh = row_hi + (i >> 2);
  const uint2 lo = lds_tr16(img + fh_off(rl, col >> 3) + (col & 7));
  const uint2 hi = lds_tr16(img + fh_off(rh, col >> 3) + (col & 7));
  return as_f16x8(make_uint4(lo.x, lo.y, hi.x, hi.y));
}

__global__ __launch_bounds__(64 * FH_NW, 4) void attn_f16_fwd_kernel(AttnArgs a) {
  constexpr int NW = FH_NW;
  constexpr int QT = 2;                      // 16-query tiles per wave
  constexpr int NT = 64 * NW;
  constexpr int CPT = 512 / NT;              // 16-byte chunks of a [64][64] tile per thread
  static_assert(CPT * NT == 512, "the staging loops cover a tile exactly");
  __shared__ __attribute__((aligned(16))) h16_raw s_k[2][FH_TILE];
  __shared__ __attribute__((aligned(16))) h16_raw s_v[2][FH_TILE];
  __shared__ __attribute__((aligned(16))) float s_mask[2][TK];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int blk, h, b;
  attn_decode_block(a, blk, h, b);
  const int qbase = blk * (16 * QT * NW) + w * (16 * QT);
  const h16_raw* qp = (const h16_raw*)a.q + (size_t)b * a.bsq + h * ATTN_D;
  const h16_raw* kp = (const h16_raw*)a.k + (size_t)b * a.bsk + h * ATTN_D;
  const h16_raw* vp = (const h16_raw*)a.v + (size_t)b * a.bsv + h * ATTN_D;
  const float sc2 = a.scale * LOG2E;

  f16x8 qf[QT][2];
  int qrow[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qrow[qt] = qbase + qt * 16 + c;
    const int r = qrow[qt] < a.Lq ? qrow[qt] : a.Lq - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[qt][ks] = as_f16x8(ld_frag_global(qp, a.ldq, r, ks * 32 + g * 8));
  }
  f32x4 oacc[QT][4];
  float m_run[QT], nm[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m_run[qt] = -INFINITY;     // running maximum (log2 domain) shared by the four lanes of a query
    nm[qt] = 0.f;              // -(m_run), 0 while m_run is still -inf
    l_run[qt] = 0.f;           // this lane's share of the row sum
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  uint4 kreg[CPT], vreg[CPT];
  float mreg;
  auto stage_load = [&](int kv0) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int ch = tid + i * NT, row = ch >> 3, d0 = (ch & 7) * 8;
      kreg[i] = vreg[i] = make_uint4(0, 0, 0, 0);                  // rows past the end are zero filled
      if (kv0 + row < a.Lk) {
        kreg[i] = ld_frag_global(kp, a.ldk, kv0 + row, d0);
        vreg[i] = ld_frag_global(vp, a.ldv, kv0 + row, d0);
      }
    }
    mreg = (tid < TK && kv0 + tid < a.Lk) ? 0.f : -INFINITY;       // the C operand of Q K^T: -inf for keys past the end
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int ch = tid + i * NT, row = ch >> 3;
      *reinterpret_cast<uint4*>(s_k[buf] + fh_off(row, ch & 7)) = kreg[i];
      *reinterpret_cast<uint4*>(s_v[buf] + fh_off(row, ch & 7)) = vreg[i];
    }
    if (tid < TK) s_mask[buf][tid] = mreg;
  };
  stage_load(0);
  stage_store(0);
  if (TK < a.Lk) stage_load(TK);
  __syncthreads();

  for (int kv0 = 0, cur = 0; kv0 < a.Lk; kv0 += TK, cur ^= 1) {
    const h16_raw* ck = s_k[cur];
    const h16_raw* cv = s_v[cur];
    const float* cmask = s_mask[cur];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {       // halves of 32 keys: key tiles t = 2 hh, 2 hh + 1
      // ---- S^T = K Q^T (+ -inf past Lk)
      f32x4 sacc[QT][2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * hh + tt;
        const float4 mk = *reinterpret_cast<const float4*>(&cmask[t * 16 + g * 4]);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) sacc[qt][tt] = (f32x4){mk.x, mk.y, mk.z, mk.w};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const f16x8 kf = fh_frag_rows(ck, t, ks, lane);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) sacc[qt][tt] = mfma16h(kf, qf[qt][ks], sacc[qt][tt]);
        }
      }
      // ---- first half: stage tile j+1 into the other buffer (its last readers passed the barrier that closed
      //      iteration j-1) and start the global loads of tile j+2; both overlap the arithmetic below
      if (hh == 0 && kv0 + TK < a.Lk) {
        stage_store(cur ^ 1);
        if (kv0 + 2 * TK < a.Lk) stage_load(kv0 + 2 * TK);
      }
      // ---- t = s * scale * log2e - m_stale
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int r = 0; r < 4; ++r) sacc[qt][tt][r] = fmaf(sacc[qt][tt][r], sc2, nm[qt]);
      // ---- lazy running maximum (decision before this half's P exists): a rescale only when some t exceeds F16_THR
      float lm[QT];
      bool grow = false;
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const f32x4 s0 = sacc[qt][0], s1 = sacc[qt][1];
        lm[qt] = max3f(max3f(s0[0], s0[1], s0[2]), max3f(s0[3], s1[0], s1[1]), fmaxf(s1[2], s1[3]));
        grow |= (lm[qt] > F16_THR) | ((m_run[qt] == -INFINITY) & (lm[qt] > -INFINITY));   // no maximum yet: any finite score sets it
      }
      if (__any(grow)) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          const float m_new = fmaxf(m_run[qt], quad_max(lm[qt]) - nm[qt]);      // lm is relative to the stale maximum
          const float nm_new = (m_new == -INFINITY) ? 0.f : -m_new;
          const float alpha = fast_exp2(m_run[qt] + nm_new);  // exp2(m_old - m_new); first update: exp2(-inf) = 0, O = l = 0
          const float shift = nm_new - nm[qt];
          m_run[qt] = m_new;
          nm[qt] = nm_new;
          l_run[qt] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) oacc[qt][dt] *= alpha;
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sacc[qt][tt][r] += shift;
        }
      }
      // ---- P = exp2(t); row sums of the fp32 values; P rounded to fp16 (nearest even) as the B operand
      f16x8 pb[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        float psum = 0.f;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = fast_exp2(sacc[qt][tt][r]);
            psum += p;
            sacc[qt][tt][r] = p;
          }
        l_run[qt] += psum;
        pb[qt] = pack_pair_f16(sacc[qt][0], sacc[qt][1]);
      }
      // ---- O^T += V^T P^T over this half's 32 keys: k-slot (g, j) <-> key 32 hh + 16 (j >> 2) + 4 g + (j & 3)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f16x8 vf = fh_frag_tr(cv, 32 * hh + 4 * g, 32 * hh + 16 + 4 * g, dt * 16, lane);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) oacc[qt][dt] = mfma16h(vf, pb[qt], oacc[qt][dt]);
      }
    }
    // one barrier per tile: buffer `cur` is free again, buffer `cur^1` is complete.  This wave's LDS traffic has landed,
    // then the bare barrier: no fence, which would wait for the global loads of tile j + 2 first (as in attn_fwd2.hip).
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" : : : "memory");
  }

  // ---- epilogue: normalise in fp32, round once, store O[q][h*64 + dt*16 + g*4 .. +3]
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l = quad_sum(l_run[qt]);
    const float inv = 1.0f / l;
    if (qrow[qt] < a.Lq) {
      _Float16* op = (_Float16*)a.o + (size_t)b * a.bso + (size_t)qrow[qt] * a.ldo + h * ATTN_D;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        st4<_Float16>(op + dt * 16 + g * 4, make_float4(oacc[qt][dt][0] * inv, oacc[qt][dt][1] * inv,
                                                        oacc[qt][dt][2] * inv, oacc[qt][dt][3] * inv));
    }
  }
}

BEVBERT_API int bevbert_attn_f16_fwd(const void* q, const void* k, const void* v, void* o, const int64_t* strides, int B,
                                     int nh, int Lq, int Lk, int head_dim, float scale, hipStream_t stream) {
  BB_REQUIRE(head_dim == ATTN_D, "attn_f16_fwd: head_dim=%d unsupported (the kernel is specialised for 64)", head_dim);
  BB_REQUIRE(q != nullptr && k != nullptr && v != nullptr && o != nullptr && strides != nullptr,
             "attn_f16_fwd: q, k, v, o and strides must not be NULL");
  BB_REQUIRE(B > 0 && nh > 0 && Lq > 0 && Lk > 0, "attn_f16_fwd: empty problem B=%d nh=%d Lq=%d Lk=%d", B, nh, Lq, Lk);
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.o = o;
  a.ldq = strides[0]; a.ldk = strides[1]; a.ldv = strides[2]; a.ldo = strides[3];
  a.bsq = strides[4]; a.bsk = strides[5]; a.bsv = strides[6]; a.bso = strides[7];
  a.B = B; a.nh = nh; a.Lq = Lq; a.Lk = Lk; a.scale = scale;
  const int64_t width = (int64_t)nh * ATTN_D;
  BB_REQUIRE(a.ldq >= width && a.ldk >= width && a.ldv >= width && a.ldo >= width,
             "attn_f16_fwd: row strides below nh * 64 = %ld", (long)width);
  BB_REQUIRE(a.bsq >= 0 && a.bsk >= 0 && a.bsv >= 0 && a.bso >= 0, "attn_f16_fwd: negative batch stride");
  BB_REQUIRE(attn_mfma_operands_aligned(a, false), "attn_f16_fwd: " ATTN_MFMA_ALIGN_MSG);
  a.nblk = (Lq + 32 * FH_NW - 1) / (32 * FH_NW);
  BB_REQUIRE((int64_t)a.nblk * nh * B < (int64_t)1 << 31, "attn_f16_fwd: too many workgroups");
  hipLaunchKernelGGL(attn_f16_fwd_kernel, dim3((unsigned)(a.nblk * nh * B)), dim3(64 * FH_NW), 0, stream, a);
  BB_CHECK_LAUNCH("attn_f16_fwd");
  return BB_OK;
}
