// Panorama inputs of a pre-training batch gathered on the device (vln_bevbert_amd/path_data.py, feature_store.py).
//
// Reference call sites replaced:
//   R2RTextPathData.get_traj_pano_fts      pretrain_src/data/dataset.py:580-622 (per step: 36+ rows of the viewpoint's
//                                          view features re-ordered [candidate views, other views], widened to fp32)
//   mlm/sap/masksem_collate                pretrain_src/data/tasks.py:126-137 (pad_tensors over the flat panorama list)
//   PrefetchLoader.move_to_cuda            pretrain_src/data/loader.py:78-120 (the host -> device copy of the result)
//
// A batch names its panoramas by row of a resident view-feature store (N, n_views, Ds) fp16; the per-viewpoint PanoTable
// (view order, token count, location features, nav types -- none depend on the path) is resident too.  One launch writes
// the four panorama tensors of the batch, padding included: everything beyond a panorama's token count is zero, and a row
// of -1 is a dummy panorama (StaticBatch's padding of the panorama axis): all zeros, length 1.
#include <hip/hip_fp16.h>

#include "common.h"

// One thread per 16-byte piece (8 halves -> two float4 stores) of a token's feature row, or per single element where the
// row cannot be cut into aligned pieces: a token has d8 pieces followed by D - 8 * d8 scalar elements.  The first thread of
// a token also writes its location features and nav type, the first thread of a panorama its length.  No atomics, no
// shared memory: every output element has exactly one writer.
__global__ __launch_bounds__(256) void pd_pano_rows_kernel(
    const __half* __restrict__ store, int64_t view_stride, int n_views, const uint8_t* __restrict__ view_order,
    const int* __restrict__ n_tokens, const float* __restrict__ loc_tab, const uint8_t* __restrict__ nav_tab,
    const int* __restrict__ rows, float* __restrict__ img, float* __restrict__ loc, int64_t* __restrict__ nav,
    int64_t* __restrict__ lens, int N, int Vmax, int L, int Vp, int D, int d8, int64_t total) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int U = d8 + (D - 8 * d8);
  const int u = (int)(gid % U);
  const int64_t tok = gid / U;
  const int v = (int)(tok % Vp);
  const int64_t t = tok / Vp;
  int row = rows[t];
  if (row >= N) row = -1;                   // the host refuses such rows before the launch; never read outside the tables
  const int n = row >= 0 ? min(n_tokens[row], min(Vmax, Vp)) : 0;
  const bool live = v < n;
  const int64_t slot = (int64_t)max(row, 0) * Vmax + min(v, Vmax - 1);
  const __half* src = store;
  if (live) src += ((int64_t)row * n_views + min((int)view_order[slot], n_views - 1)) * view_stride;
  float* dst = img + tok * D;
  if (u < d8) {
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (live) {
      const uint4 raw = *reinterpret_cast<const uint4*>(src + 8 * u);
      const __half2* h = reinterpret_cast<const __half2*>(&raw);
      const float2 a = __half22float2(h[0]), b = __half22float2(h[1]), c = __half22float2(h[2]), d = __half22float2(h[3]);
      lo = make_float4(a.x, a.y, b.x, b.y);
      hi = make_float4(c.x, c.y, d.x, d.y);
    }
    float4* o = reinterpret_cast<float4*>(dst + 8 * u);
    o[0] = lo;
    o[1] = hi;
  } else {
    const int c = 8 * d8 + (u - d8);
    dst[c] = live ? __half2float(src[c]) : 0.f;
  }
  if (u == 0) {
    for (int l = 0; l < L; ++l) loc[tok * L + l] = live ? loc_tab[slot * L + l] : 0.f;
    nav[tok] = live ? (int64_t)nav_tab[slot] : 0;
    if (v == 0) lens[t] = row >= 0 ? (int64_t)n : 1;
  }
}

BEVBERT_API int bevbert_pd_pano_rows(const void* store, int64_t view_stride, int n_views, const uint8_t* view_order,
                                     const int* n_tokens, const float* loc_tab, const uint8_t* nav_tab, const int* rows,
                                     float* img, float* loc, int64_t* nav, int64_t* lens, int N, int Vmax, int L, int Tp,
                                     int Vp, int D, hipStream_t stream) {
  BB_REQUIRE(N >= 1 && n_views >= 1 && Vmax >= 1 && L >= 0 && Tp >= 0 && Vp >= 1 && D >= 1 && view_stride >= D,
             "pd_pano_rows: N=%d n_views=%d Vmax=%d L=%d Tp=%d Vp=%d D=%d view_stride=%lld", N, n_views, Vmax, L, Tp, Vp, D,
             (long long)view_stride);
  BB_REQUIRE(store && view_order && n_tokens && (loc_tab || L == 0) && nav_tab && rows && img && (loc || L == 0) && nav && lens,
             "pd_pano_rows: null pointer");
  if (Tp == 0) return BB_OK;
  // 16-byte pieces need every view row and every output row to start on a 16-byte boundary
  const bool vec = D >= 8 && view_stride % 8 == 0 && D % 4 == 0 && ((uintptr_t)store % 16) == 0 && ((uintptr_t)img % 16) == 0;
  const int d8 = vec ? D / 8 : 0;
  const int64_t total = (int64_t)Tp * Vp * (d8 + (D - 8 * d8));
  BB_REQUIRE((total + 255) / 256 < (int64_t)1 << 31, "pd_pano_rows: too many elements");
  hipLaunchKernelGGL(pd_pano_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const __half*)store,
                     view_stride, n_views, view_order, n_tokens, loc_tab, nav_tab, rows, img, loc, nav, lens, N, Vmax, L, Vp, D,
                     d8, total);
  BB_CHECK_LAUNCH("pd_pano_rows");
  return BB_OK;
}
