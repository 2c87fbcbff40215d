// Library GEMMs (hipBLASLt) behind the C ABI, with cached per-shape plans.
//
// The Linear layers of the path stay on the vendor BLAS (north star: hand-written MFMA only for the attention
// contractions).  Going through PyTorch's dispatcher costs ~28 us of HOST time per GEMM (at ~330 GEMMs per training step
// that is 9 ms, and the step is host-bound at batch 64), so the path calls hipBLASLt directly: one hash lookup, one
// attribute write for the bias pointer, one hipblasLtMatmul.  Plans (descriptor + layouts + algorithm) are created on
// first use; the algorithm is the fastest of the library's top `autotune` heuristic candidates, timed once on the real operands
// (beta == 0 products are simply recomputed in place; accumulating plans are timed into a temporary).
//
// Row-major convention of the entry point:
//   C[M x N] = alpha * op(A)[M x K] . op(B)[K x N] (+ bias[N] broadcast over rows),   batch-strided optionally
//   opA == 0: A is stored M x K (lda);  opA == 1: A is stored K x M (lda) and used transposed.  Same for B (K x N / N x K).
// hipBLASLt is column-major, so the call is issued as C^T = op(B)^T . op(A)^T on the same memory.
#include <hipblaslt/hipblaslt.h>
#include <hipblaslt/hipblaslt-ext.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace {

struct Plan {
  hipblasLtMatmulDesc_t desc = nullptr;
  hipblasLtMatrixLayout_t la = nullptr, lb = nullptr, lc = nullptr;
  hipblasLtMatmulAlgo_t algo;
  std::vector<hipblasLtMatmulHeuristicResult_t> cand;   // untimed candidates until the first run
  int64_t ws_limit = 0;
  size_t c_bytes = 0;
  int id = -1;
  int choice = -1, ncand = 0;   // tuning-table row: index of the chosen candidate in the heuristic's list of `ncand`,
                                // or (ncand == -1) the library-wide solution index of an exhaustive search
  std::vector<hipblasLtMatmulHeuristicResult_t> heur;   // the heuristic's list behind an imported exhaustive-search row: what a
                                // failed verification of that row falls back to
  int sel = -1;                 // position of the chosen algorithm in `cand` while candidates are kept
  hipblasOperation_t ta = HIPBLAS_OP_N, tb = HIPBLAS_OP_N;
  hipDataType tin = HIP_R_16BF, tout = HIP_R_16BF;
  std::string key;
  bool ok = false, tuned = false, has_bias = false, accumulate = false;
  bool verified = false;        // the chosen algorithm has passed the reproducibility screening (tune_plan)
};

hipblasLtHandle_t g_handle = nullptr;
std::mutex g_mu;
std::unordered_map<std::string, Plan> g_plans;
// imported tuning table: problem key -> (choice, ncand); only honoured when the heuristic returns the same ncand
std::unordered_map<std::string, std::pair<int, int>> g_tuning;

hipDataType hip_dtype(int dt) { return dt == BB_F32 ? HIP_R_32F : (dt == BB_BF16 ? HIP_R_16BF : HIP_R_16F); }

bool layout(hipblasLtMatrixLayout_t* l, hipDataType t, uint64_t rows, uint64_t cols, int64_t ld, int batch,
            int64_t stride) {
  if (hipblasLtMatrixLayoutCreate(l, t, rows, cols, ld) != HIPBLAS_STATUS_SUCCESS) return false;
  if (batch > 1) {
    int32_t bc = batch;
    if (hipblasLtMatrixLayoutSetAttribute(*l, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &bc, sizeof(bc)) != HIPBLAS_STATUS_SUCCESS) return false;
    if (hipblasLtMatrixLayoutSetAttribute(*l, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &stride, sizeof(stride)) != HIPBLAS_STATUS_SUCCESS) return false;
  }
  return true;
}

}  // namespace

namespace {

std::vector<Plan*> g_plan_list;   // plan id -> plan (ids are handed to the host so that the per-call path is 8 arguments)

struct Problem {
  int M, N, K, opA, opB;
  int64_t lda, ldb, ldc;
  int batch;
  int64_t sa, sb, sc;
  int in_dtype, out_dtype, bias_dtype;   // bias_dtype < 0: no bias
  int accumulate;                        // C += product (beta = 1) instead of C = product
};

int make_plan(const Problem& q, int64_t workspace_bytes, int autotune) {
  char keybuf[256];
  snprintf(keybuf, sizeof(keybuf), "%d.%d.%d.%d.%d.%ld.%ld.%ld.%d.%ld.%ld.%ld.%d.%d.%d.%d", q.M, q.N, q.K, q.opA, q.opB,
           (long)q.lda, (long)q.ldb, (long)q.ldc, q.batch, (long)q.sa, (long)q.sb, (long)q.sc, q.in_dtype,
           q.out_dtype, q.bias_dtype, q.accumulate);
  const std::string key(keybuf);
  if (g_handle == nullptr && hipblasLtCreate(&g_handle) != HIPBLAS_STATUS_SUCCESS) {
    bb_set_error("gemm: hipblasLtCreate failed");
    return BB_ELAUNCH;
  }
  auto it = g_plans.find(key);
  if (it != g_plans.end()) return it->second.id;
  Plan p;
  const hipDataType tin = hip_dtype(q.in_dtype), tout = hip_dtype(q.out_dtype);
  bool good = hipblasLtMatmulDescCreate(&p.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F) == HIPBLAS_STATUS_SUCCESS;
  // column-major view: first operand comes from B, second from A (see the header comment)
  const hipblasOperation_t ta = q.opB ? HIPBLAS_OP_T : HIPBLAS_OP_N, tb = q.opA ? HIPBLAS_OP_T : HIPBLAS_OP_N;
  p.ta = ta; p.tb = tb; p.tin = tin; p.tout = tout;
  good = good && hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &ta, sizeof(ta)) == HIPBLAS_STATUS_SUCCESS;
  good = good && hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &tb, sizeof(tb)) == HIPBLAS_STATUS_SUCCESS;
  if (q.bias_dtype >= 0) {
    const hipblasLtEpilogue_t ep = HIPBLASLT_EPILOGUE_BIAS;
    const hipDataType bt = hip_dtype(q.bias_dtype);
    good = good && hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &ep, sizeof(ep)) == HIPBLAS_STATUS_SUCCESS;
    good = good && hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bt, sizeof(bt)) == HIPBLAS_STATUS_SUCCESS;
  }
  // first operand: opB == 0 -> view (N x K, ld ldb) used as is; opB == 1 -> view (K x N, ld ldb) used transposed
  good = good && (q.opB ? layout(&p.la, tin, q.K, q.N, q.ldb, q.batch, q.sb) : layout(&p.la, tin, q.N, q.K, q.ldb, q.batch, q.sb));
  // second operand: opA == 0 -> view (K x M, ld lda); opA == 1 -> view (M x K, ld lda) used transposed
  good = good && (q.opA ? layout(&p.lb, tin, q.M, q.K, q.lda, q.batch, q.sa) : layout(&p.lb, tin, q.K, q.M, q.lda, q.batch, q.sa));
  good = good && layout(&p.lc, tout, q.N, q.M, q.ldc, q.batch, q.sc);
  const int want = autotune > 1 ? (autotune > 64 ? 64 : autotune) : 1;
  p.cand.resize(want);
  int found = 0;
  if (good) {
    hipblasLtMatmulPreference_t pref = nullptr;
    good = hipblasLtMatmulPreferenceCreate(&pref) == HIPBLAS_STATUS_SUCCESS;
    const uint64_t wsb = (uint64_t)workspace_bytes;
    good = good && hipblasLtMatmulPreferenceSetAttribute(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &wsb, sizeof(wsb)) == HIPBLAS_STATUS_SUCCESS;
    good = good && hipblasLtMatmulAlgoGetHeuristic(g_handle, p.desc, p.la, p.lb, p.lc, p.lc, pref, want, p.cand.data(),
                                                   &found) == HIPBLAS_STATUS_SUCCESS;
    if (pref) hipblasLtMatmulPreferenceDestroy(pref);
  }
  p.cand.resize(good && found > 0 ? found : 0);
  p.ok = !p.cand.empty();
  p.tuned = p.cand.size() <= 1;
  p.key = key;
  p.ncand = (int)p.cand.size();
  p.choice = p.ok ? 0 : -1;
  const auto imported = g_tuning.find(key);
  if (p.ok && imported != g_tuning.end() && imported->second.second == -1 && imported->second.first >= 0) {
    // the pick of an exhaustive search (all solutions of the library, not only the heuristic's): by solution index
    std::vector<int> idx{imported->second.first};
    std::vector<hipblasLtMatmulHeuristicResult_t> one;
    const float alpha = 1.f, beta0 = q.accumulate ? 1.f : 0.f;
    size_t ws = 0;
    if (hipblaslt_ext::getAlgosFromIndex(g_handle, idx, one) == HIPBLAS_STATUS_SUCCESS && one.size() == 1 &&
        hipblaslt_ext::matmulIsAlgoSupported(g_handle, p.desc, &alpha, p.la, p.lb, &beta0, p.lc, p.lc, one[0].algo, ws) ==
            HIPBLAS_STATUS_SUCCESS && (int64_t)ws <= workspace_bytes) {
      one[0].workspaceSize = ws;
      one[0].state = HIPBLAS_STATUS_SUCCESS;
      p.heur = p.cand;
      p.cand = one;
      p.choice = imported->second.first;
      p.ncand = -1;
      p.tuned = true;
    }
  } else if (p.ok && !p.tuned && imported != g_tuning.end() && imported->second.second == p.ncand &&
             imported->second.first >= 0 && imported->second.first < p.ncand) {
    p.choice = imported->second.first;       // a previous run timed this problem on this library: reuse its pick
    p.tuned = true;
  }
  p.sel = p.ncand == -1 ? 0 : p.choice;
  p.has_bias = q.bias_dtype >= 0;
  p.accumulate = q.accumulate != 0;
  p.c_bytes = (size_t)(q.batch > 1 ? q.batch * q.sc : q.M * q.ldc) * (q.out_dtype == BB_F32 ? 4 : 2);
  p.ws_limit = workspace_bytes;
  if (p.ok && p.tuned &&
      (p.cand[p.sel].state != HIPBLAS_STATUS_SUCCESS || (int64_t)p.cand[p.sel].workspaceSize > workspace_bytes)) {
    p.ok = false;                 // the only / the recorded candidate is not usable here
    p.choice = -1;
  }
  if (p.ok) p.algo = p.cand[p.sel].algo;
  if (p.tuned && p.ncand >= 0 && p.ncand <= 1) {      // nothing to choose from: the library's only algorithm is used as it is
    p.verified = true;
    p.cand.clear();
    p.cand.shrink_to_fit();
  }                                   // table rows keep their candidates until the first run has verified the choice
  p.id = (int)g_plan_list.size();
  Plan* stored = &g_plans.emplace(key, std::move(p)).first->second;   // unordered_map nodes are address-stable
  g_plan_list.push_back(stored);
  if (!stored->ok) {
    bb_set_error("gemm: hipBLASLt has no algorithm for M=%d N=%d K=%d opA=%d opB=%d dtype %d->%d", q.M, q.N, q.K, q.opA,
                 q.opB, q.in_dtype, q.out_dtype);
  }
  return stored->id;
}

// Order-independent checksum of a buffer (integer adds commute): two runs of a GEMM that differ in ANY output bit give
// different sums.  Used to screen out library algorithms whose result depends on the order in which workgroups
// accumulate (split-K / stream-K reductions through atomics): training on this path is bit-reproducible (DESIGN.md
// section 2), and a single such kernel in the tuned table breaks that -- observed in round 4 as ~40 differing gradient
// elements out of 238 M between two identical MLM steps on one box (the 30 522-deep decoder input-gradient GEMM).
__global__ __launch_bounds__(256) void gemm_checksum_kernel(const uint32_t* __restrict__ p, size_t nwords,
                                                            unsigned long long* __restrict__ out) {
  unsigned long long h = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256)
    h += (unsigned long long)p[i] * (0x9E3779B97F4A7C15ull ^ (unsigned long long)i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, h);
}

bool g_screen = true;          // BEVBERT_GEMM_DETERMINISTIC=0 turns the screening off (A/B)
bool g_screen_read = false;

// true when `reps` launches of the candidate leave the same bits in C.  C must be a buffer the launches may overwrite
// (the real output for beta = 0 plans, a temporary for accumulating ones: it is zeroed before each launch).
bool reproducible(Plan& p, const hipblasLtMatmulAlgo_t& algo, const void* A, const void* B, void* C, void* workspace,
                  int64_t workspace_bytes, hipStream_t stream, unsigned long long* sums_dev, int reps = 3) {
  const float alpha = 1.f, beta0 = p.accumulate ? 1.f : 0.f;
  unsigned long long sums[4] = {0, 0, 0, 0};
  (void)hipMemsetAsync(sums_dev, 0, sizeof(sums), stream);
  for (int r = 0; r < reps; ++r) {
    if (p.accumulate) (void)hipMemsetAsync(C, 0, p.c_bytes, stream);
    if (hipblasLtMatmul(g_handle, p.desc, &alpha, B, p.la, A, p.lb, &beta0, C, p.lc, C, p.lc, &algo, workspace,
                        workspace_bytes, stream) != HIPBLAS_STATUS_SUCCESS)
      return false;
    const size_t nwords = p.c_bytes / 4;
    const int nb = (int)((nwords + 255) / 256 < 2048 ? (nwords + 255) / 256 : 2048);
    hipLaunchKernelGGL(gemm_checksum_kernel, dim3(nb > 0 ? nb : 1), dim3(256), 0, stream, (const uint32_t*)C, nwords, sums_dev + r);
  }
  if (hipMemcpyAsync(sums, sums_dev, sizeof(sums), hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
  (void)hipStreamSynchronize(stream);
  for (int r = 1; r < reps; ++r)
    if (sums[r] != sums[0]) return false;
  return true;
}

// time the candidates once on the real operands and keep the fastest REPRODUCIBLE one.  beta == 0: the product is simply
// recomputed in place; accumulate plans are timed into a temporary so that C is not touched.
int g_rejected = 0;             // candidates dropped by the screening so far (bevbert_gemm_rejected_count)

void tune_plan(Plan& p, const void* A, const void* B, void* C, void* workspace, int64_t workspace_bytes,
               hipStream_t stream, int only = -1) {
  const float alpha = 1.f, beta0 = p.accumulate ? 1.f : 0.f;
  void* scratch = nullptr;
  void* const C_real = C;
  // Time in isolation: the candidate list contains stream-K kernels whose workgroups spin on flags written by peer
  // workgroups.  Exercised while another stream holds part of the chip with a kernel of the same kind, two partially
  // resident grids can wait for each other's unscheduled peers (observed: a run with concurrent weight-gradient and
  // forward timing passes on three streams never returned from hipEventSynchronize).  Nothing else is in flight after
  // this call, and the host thread stays here until the choice is made.
  (void)hipDeviceSynchronize();
  if (p.accumulate) {
    if (hipMalloc(&scratch, p.c_bytes) != hipSuccess || hipMemsetAsync(scratch, 0, p.c_bytes, stream) != hipSuccess) {
      if (scratch) (void)hipFree(scratch);
      if (!p.tuned) p.algo = p.cand[0].algo;      // cannot time: keep the heuristic's first choice / the table's
      p.tuned = true;
      p.verified = true;
      return;
    }
    C = scratch;
  }
  if (!g_screen_read) {
    const char* e = getenv("BEVBERT_GEMM_DETERMINISTIC");
    g_screen = !(e != nullptr && e[0] == '0');
    g_screen_read = true;
  }
  static const bool exhaustive = [] { const char* e = getenv("BEVBERT_LT_EXHAUSTIVE"); return e != nullptr && e[0] == '1'; }();
  bool all_algos = false;
  if (only < 0 && exhaustive) {
    // every solution the library has for this operand layout / type combination (hipblaslt-bench --algo_method all),
    // filtered by matmulIsAlgoSupported on THIS problem: the heuristic's top picks favour large tiles, which leave most
    // of the 256 CUs idle on the 5 120-row problems of the text stream
    std::vector<hipblasLtMatmulHeuristicResult_t> all;
    if (hipblaslt_ext::getAllAlgos(g_handle, hipblaslt_ext::GemmType::HIPBLASLT_GEMM, p.ta, p.tb, p.tin, p.tin, p.tout, p.tout,
                                   HIPBLAS_COMPUTE_32F, all) == HIPBLAS_STATUS_SUCCESS) {
      std::vector<hipblasLtMatmulHeuristicResult_t> usable;
      for (auto& r : all) {
        size_t ws = 0;
        if (hipblaslt_ext::matmulIsAlgoSupported(g_handle, p.desc, &alpha, p.la, p.lb, &beta0, p.lc, p.lc, r.algo, ws) !=
            HIPBLAS_STATUS_SUCCESS || (int64_t)ws > workspace_bytes)
          continue;
        r.workspaceSize = ws;
        r.state = HIPBLAS_STATUS_SUCCESS;
        usable.push_back(r);
      }
      if (!usable.empty()) {
        p.cand.swap(usable);
        all_algos = true;
      }
    }
  }
  unsigned long long* sums_dev = nullptr;
  if (g_screen && hipMalloc(&sums_dev, 4 * sizeof(unsigned long long)) != hipSuccess) sums_dev = nullptr;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  float best_ms = 1e30f;
  int best = -1;
  std::vector<std::pair<float, int>> timed;
  for (size_t i = 0; i < p.cand.size(); ++i) {
    if (only >= 0 && (int)i != only) continue;
    if (p.cand[i].state != HIPBLAS_STATUS_SUCCESS || (int64_t)p.cand[i].workspaceSize > workspace_bytes) continue;
    bool run_ok = true;
    const int warm = all_algos ? 1 : 2, reps = all_algos ? 3 : 10;   // exhaustive: a quick first pass over hundreds of kernels
    for (int rep = 0; rep < reps && run_ok; ++rep) {
      if (rep == warm) (void)hipEventRecord(e0, stream);
      run_ok = hipblasLtMatmul(g_handle, p.desc, &alpha, B, p.la, A, p.lb, &beta0, C, p.lc, C, p.lc, &p.cand[i].algo,
                               workspace, workspace_bytes, stream) == HIPBLAS_STATUS_SUCCESS;
    }
    if (!run_ok) continue;
    (void)hipEventRecord(e1, stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    timed.emplace_back(ms / (reps - warm), (int)i);
  }
  if (all_algos && timed.size() > 8) {             // second pass: the eight fastest, timed like the heuristic candidates
    std::sort(timed.begin(), timed.end());
    timed.resize(8);
    for (auto& t : timed) {
      bool run_ok = true;
      for (int rep = 0; rep < 10 && run_ok; ++rep) {
        if (rep == 2) (void)hipEventRecord(e0, stream);
        run_ok = hipblasLtMatmul(g_handle, p.desc, &alpha, B, p.la, A, p.lb, &beta0, C, p.lc, C, p.lc, &p.cand[t.second].algo,
                                 workspace, workspace_bytes, stream) == HIPBLAS_STATUS_SUCCESS;
      }
      (void)hipEventRecord(e1, stream);
      (void)hipEventSynchronize(e1);
      float ms = 1e30f;
      if (run_ok) (void)hipEventElapsedTime(&ms, e0, e1);
      t.first = run_ok ? ms / 8.f : 1e30f;
    }
  }
  // fastest first; the first one whose output bits repeat wins (screening in this order costs three extra launches for
  // the typical problem, whose fastest candidate is a plain data-parallel kernel)
  std::sort(timed.begin(), timed.end());
  for (const auto& t : timed) {
    if (sums_dev != nullptr && !reproducible(p, p.cand[t.second].algo, A, B, C, workspace, workspace_bytes, stream, sums_dev)) {
      ++g_rejected;
      continue;
    }
    best_ms = t.first;
    best = t.second;
    break;
  }
  if (sums_dev) (void)hipFree(sums_dev);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (scratch) (void)hipFree(scratch);
  if (only >= 0) {                // verification of a table row: keep it, or fall back to a full timing pass
    if (best == only) {
      p.verified = true;
      p.cand.clear();
      p.cand.shrink_to_fit();
      p.heur.clear();
      return;
    }
    if (p.ncand == -1 && !p.heur.empty()) {      // the imported exhaustive-search pick does not repeat / launch here: time
      p.cand.swap(p.heur);                       // the heuristic's candidates instead of giving the problem up
      p.heur.clear();
      p.ncand = (int)p.cand.size();
    }
    tune_plan(p, A, B, C_real, workspace, workspace_bytes, stream, -1);
    return;
  }
  p.verified = true;
  p.tuned = true;
  if (best < 0) {                 // no candidate is usable (invalid state / workspace too small / launch failure)
    p.ok = false;
    p.choice = -1;
    p.cand.clear();
    return;
  }
  p.algo = p.cand[best].algo;
  if (all_algos) {
    p.choice = hipblaslt_ext::getIndexFromAlgo(p.algo);      // library-wide solution index (stable for one library version)
    p.ncand = -1;
  } else {
    p.choice = best;
  }
  p.cand.clear();
  p.cand.shrink_to_fit();
}

// Cin: addend of an accumulating plan when it is NOT the output buffer (D = A.B + Cin, beta = 1); null -> in place
int run_plan(Plan& p, const void* A, const void* B, void* C, const void* bias, float alpha, void* workspace,
             int64_t workspace_bytes, hipStream_t stream, const void* Cin = nullptr) {
  if (!p.ok) {
    bb_set_error("gemm: plan %d has no algorithm", p.id);
    return BB_EUNSUPPORTED;
  }
  BB_REQUIRE((bias != nullptr) == p.has_bias, "gemm: plan %d was made %s a bias", p.id, p.has_bias ? "with" : "without");
  BB_REQUIRE(workspace_bytes >= p.ws_limit, "gemm: plan %d needs the %ld-byte workspace it was planned with", p.id, (long)p.ws_limit);
  if (p.has_bias &&
      hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof(bias)) != HIPBLAS_STATUS_SUCCESS) {
    bb_set_error("gemm: cannot set the bias pointer");
    return BB_ELAUNCH;
  }
  if (!p.tuned || !p.verified) {
    // first use (never inside a graph capture: the warm-up steps come first): time the candidates -- or, for a choice
    // imported from the shipped table, check that this algorithm's output bits repeat, else time them all
    tune_plan(p, A, B, C, workspace, workspace_bytes, stream, p.tuned ? p.sel : -1);
    if (!p.ok) {
      bb_set_error("gemm: none of the library's candidates for plan %d can run", p.id);
      return BB_EUNSUPPORTED;
    }
  }
  const float beta0 = p.accumulate ? 1.f : 0.f;
  const hipblasStatus_t st = hipblasLtMatmul(g_handle, p.desc, &alpha, B, p.la, A, p.lb, &beta0, Cin ? Cin : C, p.lc, C,
                                             p.lc, &p.algo, workspace, workspace_bytes, stream);
  if (st != HIPBLAS_STATUS_SUCCESS) {
    bb_set_error("gemm: hipblasLtMatmul failed with status %d (plan %d)", (int)st, p.id);
    return BB_ELAUNCH;
  }
  return BB_OK;
}

int check_problem(const Problem& q) {
  BB_REQUIRE(q.M > 0 && q.N > 0 && q.K > 0 && q.batch >= 1, "gemm: empty problem M=%d N=%d K=%d batch=%d", q.M, q.N, q.K, q.batch);
  BB_REQUIRE(q.in_dtype == BB_F32 || q.in_dtype == BB_BF16 || q.in_dtype == BB_F16, "gemm: input dtype %d unsupported", q.in_dtype);
  BB_REQUIRE(q.out_dtype == BB_F32 || q.out_dtype == q.in_dtype, "gemm: output dtype %d unsupported", q.out_dtype);
  BB_REQUIRE(q.bias_dtype < 0 || q.bias_dtype == BB_F32 || q.bias_dtype == q.out_dtype, "gemm: bias dtype %d unsupported", q.bias_dtype);
  return BB_OK;
}

}  // namespace

// Plan a GEMM: returns a plan id >= 0 (also for problems the library cannot run: bevbert_gemm_run then returns
// BB_EUNSUPPORTED), or a negative error code.  bias_dtype < 0: no bias epilogue.
BEVBERT_API int bevbert_gemm_plan(int M, int N, int K, int opA, int opB, int64_t lda, int64_t ldb, int64_t ldc,
                                  int batch, int64_t stride_a, int64_t stride_b, int64_t stride_c, int in_dtype,
                                  int out_dtype, int bias_dtype, int accumulate, int64_t workspace_bytes,
                                  int autotune) {
  const Problem q{M, N, K, opA, opB, lda, ldb, ldc, batch, stride_a, stride_b, stride_c, in_dtype, out_dtype,
                  bias_dtype < 0 ? -1 : bias_dtype, accumulate != 0};
  const int rc = check_problem(q);
  if (rc != BB_OK) return rc;
  std::lock_guard<std::mutex> lock(g_mu);
  return make_plan(q, workspace_bytes, autotune);
}

BEVBERT_API int bevbert_gemm_run(int plan, const void* A, const void* B, void* C, const void* bias, void* workspace,
                                 int64_t workspace_bytes, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(g_mu);
  BB_REQUIRE(plan >= 0 && plan < (int)g_plan_list.size(), "gemm: unknown plan id %d", plan);
  return run_plan(*g_plan_list[plan], A, B, C, bias, 1.f, workspace, workspace_bytes, stream);
}

// D = A.B + Cin with an accumulating plan (beta = 1) and a separate addend: the input-gradient GEMM of a Linear whose
// input also feeds a residual connection folds the residual's gradient in, instead of a separate elementwise add.
BEVBERT_API int bevbert_gemm_run_add(int plan, const void* A, const void* B, const void* Cin, void* D, const void* bias,
                                     void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(g_mu);
  BB_REQUIRE(plan >= 0 && plan < (int)g_plan_list.size(), "gemm: unknown plan id %d", plan);
  BB_REQUIRE(g_plan_list[plan]->accumulate && Cin != nullptr, "gemm_run_add: needs an accumulating plan and an addend");
  return run_plan(*g_plan_list[plan], A, B, D, bias, 1.f, workspace, workspace_bytes, stream, Cin);
}

// One-shot form: plan (cached by problem) + run.
BEVBERT_API int bevbert_gemm(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int opA,
                             int opB, int64_t lda, int64_t ldb, int64_t ldc, int batch, int64_t stride_a,
                             int64_t stride_b, int64_t stride_c, int in_dtype, int out_dtype, int bias_dtype,
                             float alpha, void* workspace, int64_t workspace_bytes, int autotune,
                             hipStream_t stream) {
  const Problem q{M, N, K, opA, opB, lda, ldb, ldc, batch, stride_a, stride_b, stride_c, in_dtype, out_dtype,
                  bias != nullptr ? bias_dtype : -1, 0};
  const int rc = check_problem(q);
  if (rc != BB_OK) return rc;
  std::lock_guard<std::mutex> lock(g_mu);
  const int id = make_plan(q, workspace ? workspace_bytes : 0, autotune);
  if (id < 0) return id;
  return run_plan(*g_plan_list[id], A, B, C, bias, alpha, workspace, workspace_bytes, stream);
}

// Tuning table: one line "<problem key> <choice> <ncand>" per autotuned plan, after a header naming the library version.
// export returns the number of bytes the text needs (incl. the terminating 0) and fills buf when cap is large enough;
// import replaces the table used by plans created afterwards (a table from another hipBLASLt version is ignored: -3).
static int lt_version() {
  int v = 0, ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return -1;   // hipblasLtCreate aborts without a device
  if (g_handle == nullptr && hipblasLtCreate(&g_handle) != HIPBLAS_STATUS_SUCCESS) return -1;
  if (hipblasLtGetVersion(g_handle, &v) != HIPBLAS_STATUS_SUCCESS) return -1;
  return v;
}

BEVBERT_API int64_t bevbert_gemm_tuning_export(char* buf, int64_t cap) {
  std::lock_guard<std::mutex> lock(g_mu);
  std::string text = "# bevbert gemm tuning v1 hipblaslt " + std::to_string(lt_version()) + "\n";
  std::unordered_map<std::string, std::pair<int, int>> rows = g_tuning;   // keep imported rows of shapes not seen in this run
  for (const auto& kv : g_plans)
    if (kv.second.ok && kv.second.tuned && (kv.second.ncand > 1 || kv.second.ncand == -1))
      rows[kv.first] = {kv.second.choice, kv.second.ncand};
  for (const auto& kv : rows)
    text += kv.first + " " + std::to_string(kv.second.first) + " " + std::to_string(kv.second.second) + "\n";
  if (buf != nullptr && cap > (int64_t)text.size()) memcpy(buf, text.c_str(), text.size() + 1);
  return (int64_t)text.size() + 1;
}

BEVBERT_API int bevbert_gemm_tuning_import(const char* text) {
  BB_REQUIRE(text != nullptr, "gemm_tuning_import: NULL text");
  std::lock_guard<std::mutex> lock(g_mu);
  BB_REQUIRE(lt_version() >= 0, "gemm_tuning_import: no GPU / hipBLASLt handle");
  const std::string want = "# bevbert gemm tuning v1 hipblaslt " + std::to_string(lt_version());
  std::string all(text);
  size_t pos = all.find('\n');
  if (pos == std::string::npos || all.compare(0, pos, want) != 0) {
    bb_set_error("gemm_tuning_import: table is not for this hipBLASLt (%s)", want.c_str());
    return BB_EUNSUPPORTED;
  }
  g_tuning.clear();
  int n = 0;
  while (pos != std::string::npos && pos + 1 < all.size()) {
    const size_t end = all.find('\n', pos + 1);
    const std::string line = all.substr(pos + 1, end == std::string::npos ? std::string::npos : end - pos - 1);
    pos = end;
    char key[256];
    int choice = -1, ncand = 0;
    if (sscanf(line.c_str(), "%255s %d %d", key, &choice, &ncand) == 3 && key[0] != '#') {
      g_tuning[key] = {choice, ncand};
      ++n;
    }
  }
  return n;
}

// candidates the reproducibility screening has rejected so far (algorithms whose output bits changed between launches)
BEVBERT_API int bevbert_gemm_rejected_count(void) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_rejected;
}

BEVBERT_API int bevbert_gemm_plan_count(void) {
  std::lock_guard<std::mutex> lock(g_mu);
  return (int)g_plans.size();
}
