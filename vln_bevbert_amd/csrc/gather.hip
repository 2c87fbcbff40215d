// Row gathers and their backward: K6 weighted segment gather (gmap aggregation fwd and bwd), the row gather / scatter of
// the prediction heads, and the embedding-table gradients (leader form and sliced form), all without atomics.
//
// Reference call sites replaced:
//   _aggregate_gmap_features               pretrain_src/model/vilmodel.py:632-666 (Python dict loops -> one CSR gather)
//   BertEmbeddings (backward: index_add)   vilmodel.py:48-77
#include <math.h>
#include <type_traits>

#include "common.h"

// =============================================================================================
// K6: weighted segment gather: out[r] = sum_{e in [rowptr[r], rowptr[r+1])} w[e] * src[idx[e]]
// (gmap node aggregation with the CSR built on the host from the vpid lists; its backward is the same
//  kernel over the transposed CSR).
// =============================================================================================
template <typename T>
__global__ __launch_bounds__(192) void gather_wsum_kernel(const T* __restrict__ src, const int* __restrict__ rowptr,
                                                          const int* __restrict__ idx, const float* __restrict__ w,
                                                          T* __restrict__ out, int H) {
  const int r = blockIdx.x;
  const int e0 = rowptr[r], e1 = rowptr[r + 1];
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = e0; e < e1; ++e) {
      const float ww = w[e];
      const float4 v = ld4<T>(src + (size_t)idx[e] * H + c);
      acc.x += ww * v.x; acc.y += ww * v.y; acc.z += ww * v.z; acc.w += ww * v.w;
    }
    st4<T>(out + (size_t)r * H + c, acc);
  }
}

// table_grad[t] += sum of d[r] over the rows r with ids[r] == t, WITHOUT atomics and in a fixed order (training runs are
// bit-reproducible; the reference's index_add is not).  One workgroup per gradient row r: it returns at once unless r
// is the FIRST row carrying its id (and the id is not padding_idx: nn.Embedding(padding_idx=0) gives the padding row no
// lookup gradient, vilmodel.py:50).  The leader's four waves each scan one contiguous quarter of the rows [r, rows) for
// the same id -- 64 ids per ballot, four ballots' loads in flight -- and add the matching rows of d in ascending row
// order, every lane owning its columns (no LDS list, no barrier inside the scan); the four partial sums are folded as
// (w0 + w1) + (w2 + w3) and the leader alone read-modify-writes the table row.  The result is a pure function of (ids, d).
// rows^2 / 256 id comparisons per launch (5 120 rows: the id vector stays in L2).
#define EG_MAXJ 4          // float4 column groups per lane: H <= 64 lanes * 4 floats * EG_MAXJ = 1024
// TO / ACCUM: the destination rows are fp32 and accumulated into (embedding tables in the gradient arena), or of the
// activations' type -- rows of a zero-initialised activation gradient, the backward of a row gather (bevbert_rows_scatter):
// ACCUM false stores the id's sum, true adds it to what the row holds (a second scatter onto the same tensor).
template <typename T, typename TO = float, bool ACCUM = true>
__global__ __launch_bounds__(256) void embedding_grad_kernel(const int64_t* __restrict__ ids, const T* __restrict__ d,
                                                             TO* __restrict__ table_grad, int rows, int H,
                                                             int padding_idx) {
  __shared__ int s_flag;
  __shared__ float s_part[4][256 * EG_MAXJ];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t id = ids[r];
  if (id == (int64_t)padding_idx) return;
  if (tid == 0) s_flag = 0;
  __syncthreads();
  int hit = 0;
  for (int i = tid; i < r; i += 256) hit |= (ids[i] == id);
  if (hit) s_flag = 1;
  __syncthreads();
  if (s_flag) return;                       // an earlier row leads this id
  float4 acc[EG_MAXJ];
#pragma unroll
  for (int j = 0; j < EG_MAXJ; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int span = rows - r, q = (span + 3) >> 2;
  const int lo = r + wave * q, hi = min(rows, lo + q);
  for (int base = lo; base < hi; base += 256) {
    unsigned long long bal[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {           // four independent loads, then four ballots
      const int i = base + 64 * u + lane;
      bal[u] = __ballot(i < hi && ids[i] == id);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      unsigned long long b = bal[u];
      while (b) {                           // wave-uniform: the matching rows of these 64, in ascending order
        const int row = base + 64 * u + (__ffsll((long long)b) - 1);
        b &= b - 1;
#pragma unroll
        for (int j = 0; j < EG_MAXJ; ++j) {
          const int c = (lane + 64 * j) * 4;
          if (c < H) add4(acc[j], ld4<T>(d + (size_t)row * H + c));
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < EG_MAXJ; ++j) *reinterpret_cast<float4*>(&s_part[wave][(lane + 64 * j) * 4]) = acc[j];
  __syncthreads();
  TO* dst = table_grad + (size_t)id * H;
  for (int c = tid * 4; c < H; c += 1024) {
    const float4 p0 = *reinterpret_cast<const float4*>(&s_part[0][c]), p1 = *reinterpret_cast<const float4*>(&s_part[1][c]);
    const float4 p2 = *reinterpret_cast<const float4*>(&s_part[2][c]), p3 = *reinterpret_cast<const float4*>(&s_part[3][c]);
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ACCUM) t = ld4<TO>(dst + c);
    t.x += (p0.x + p1.x) + (p2.x + p3.x); t.y += (p0.y + p1.y) + (p2.y + p3.y);
    t.z += (p0.z + p1.z) + (p2.z + p3.z); t.w += (p0.w + p1.w) + (p2.w + p3.w);
    st4<TO>(dst + c, t);
  }
}

// out[i, :] = src[ids[i], :]: one workgroup per output row (index_select of activation rows: the masked tokens of the
// MLM head, the candidate cells of the SAP head, the supervised cells of the semantic head)
template <typename T>
__global__ __launch_bounds__(256) void rows_gather_kernel(const T* __restrict__ src, const int64_t* __restrict__ ids,
                                                          T* __restrict__ out, int H) {
  const int64_t id = ids[blockIdx.x];
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4)
    st4<T>(out + (size_t)blockIdx.x * H + c, ld4<T>(src + (size_t)id * H + c));
}

// Small tables (2 .. ~128 rows: navigation types, step ids, token types) with MANY gradient rows: the atomic version
// piles 28 224 rows onto two destination rows.  Here workgroup (t, s) sums the rows of slice s whose id is t and writes
// partials[s][t][:]; the slices are folded into the fp32 table gradient by the step's batched second reduction stage
// (bevbert_multi_finalize): no atomics, a fixed summation order.  The id test is wave-uniform; the loads of a group of
// four rows are issued together.
template <typename T>
__global__ __launch_bounds__(256) void embedding_grad_sliced_kernel(const int64_t* __restrict__ ids, const T* __restrict__ d,
                                                                    float* __restrict__ partials, int rows, int H,
                                                                    int rows_per_slice, int ntab) {
  const int t = blockIdx.x, s = blockIdx.y;
  const int r0 = s * rows_per_slice, r1 = min(rows, r0 + rows_per_slice);
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = r0; r < r1; r += 4) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r + j < r1 && ids[r + j] == t) v[j] = ld4<T>(d + (size_t)(r + j) * H + c);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) add4(acc, v[j]);
    }
    *reinterpret_cast<float4*>(partials + ((size_t)s * ntab + t) * H + c) = acc;
  }
}

// =============================================================================================
// C ABI
// =============================================================================================
BEVBERT_API int bevbert_segment_wsum(const void* src, const int* rowptr, const int* idx, const float* w, void* out,
                                     int out_rows, int H, int dtype, hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0, "segment_wsum: H=%d must be a multiple of 4", H);
  if (out_rows <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gather_wsum_kernel<T>, dim3(out_rows), dim3(192), 0, stream, (const T*)src, rowptr, idx, w, (T*)out, H);
  });
  if (!type_ok) return bb_dtype_unsupported("segment_wsum", dtype);
  BB_CHECK_LAUNCH("segment_wsum");
  return BB_OK;
}

BEVBERT_API int bevbert_rows_gather(const void* src, const int64_t* ids, void* out, int rows, int H, int dtype,
                                    hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0 && H > 0, "rows_gather: H=%d must be a positive multiple of 4", H);
  if (rows <= 0) return BB_OK;
  const int nt = H / 4 >= 256 ? 256 : (H / 4 + 63) / 64 * 64;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(rows_gather_kernel<T>, dim3(rows), dim3(nt), 0, stream, (const T*)src, ids, (T*)out, H);
  });
  if (!type_ok) return bb_dtype_unsupported("rows_gather", dtype);
  BB_CHECK_LAUNCH("rows_gather");
  return BB_OK;
}

BEVBERT_API int bevbert_rows_scatter(const int64_t* ids, const void* d, void* out, int rows, int H, int dtype, int accumulate,
                                     hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0 && H <= 256 * EG_MAXJ, "rows_scatter: H=%d must be a multiple of 4 and <= %d", H, 256 * EG_MAXJ);
  if (rows <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    bb_with_bool(accumulate != 0, [&](auto accum) {
      hipLaunchKernelGGL((embedding_grad_kernel<T, T, decltype(accum)::value>), dim3(rows), dim3(256), 0, stream, ids, (const T*)d, (T*)out, rows, H, -1);
    });
  });
  if (!type_ok) return bb_dtype_unsupported("rows_scatter", dtype);
  BB_CHECK_LAUNCH("rows_scatter");
  return BB_OK;
}

BEVBERT_API int bevbert_embedding_grad(const int64_t* ids, const void* d, float* table_grad, int rows, int H,
                                       int padding_idx, int dtype, hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0 && H <= 256 * EG_MAXJ, "embedding_grad: H=%d must be a multiple of 4 and <= %d", H, 256 * EG_MAXJ);
  if (rows <= 0) return BB_OK;
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(embedding_grad_kernel<T>, dim3(rows), dim3(256), 0, stream, ids, (const T*)d, table_grad, rows, H, padding_idx);
  });
  if (!type_ok) return bb_dtype_unsupported("embedding_grad", dtype);
  BB_CHECK_LAUNCH("embedding_grad");
  return BB_OK;
}

BEVBERT_API int bevbert_embedding_grad_sliced(const int64_t* ids, const void* d, float* partials, int rows, int H,
                                              int table_rows, int rows_per_slice, int dtype, hipStream_t stream) {
  BB_REQUIRE(H % 4 == 0, "embedding_grad_sliced: H=%d must be a multiple of 4", H);
  BB_REQUIRE(table_rows > 0 && rows_per_slice > 0 && rows > 0, "embedding_grad_sliced: empty problem (%d table rows, %d rows)",
             table_rows, rows);
  const int slices = (rows + rows_per_slice - 1) / rows_per_slice;
  BB_REQUIRE(slices <= 65535, "embedding_grad_sliced: %d slices exceed the grid limit", slices);
  const int nt = H / 4 < 256 ? ((H / 4 + 63) / 64) * 64 : 256;
  const dim3 grid(table_rows, slices);
  const bool type_ok = bb_with_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(embedding_grad_sliced_kernel<T>, grid, dim3(nt), 0, stream, ids, (const T*)d, partials, rows, H, rows_per_slice,
                       table_rows);
  });
  if (!type_ok) return bb_dtype_unsupported("embedding_grad_sliced", dtype);
  BB_CHECK_LAUNCH("embedding_grad_sliced");
  return BB_OK;
}
