// C-ABI glue: error channel, version, and the attention entry points that pick between the exact (fp32 arithmetic)
// kernels and the MFMA (bf16) kernels.  Declarations: include/bevbert_hip.h.
#include <stdarg.h>

#include "attn_common.h"

static thread_local char g_err[512] = "";

void bb_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

BEVBERT_API const char* bevbert_last_error(void) { return g_err; }
// A failed stream capture (hipErrorStreamCaptureInvalidated and friends) leaves its code in the runtime's sticky
// last-error slot: the NEXT launch check of any library in the process (PyTorch checks hipGetLastError after every
// kernel launch) would report it as its own.  Callers that recover from a failed capture drain the slot here; returns
// the number of stale errors dropped.
BEVBERT_API int bevbert_hip_error_reset(void) {
  int n = 0;
  while (hipGetLastError() != hipSuccess && n < 16) ++n;
  return n;
}

// Zero ``bytes`` bytes of device memory on the stream: a memset command (a memset node in a captured step) instead of a fill
// kernel that takes CUs from the work it runs beside -- the 0.96 GB gradient arena is cleared with it every step.
BEVBERT_API int bevbert_zero(void* p, int64_t bytes, hipStream_t stream) {
  BB_REQUIRE(p != nullptr && bytes >= 0, "zero: null pointer or negative size");
  if (bytes == 0) return BB_OK;
  hipError_t e = hipMemsetAsync(p, 0, (size_t)bytes, stream);
  if (e != hipSuccess) {
    bb_set_error("zero: hipMemsetAsync failed: %s", hipGetErrorString(e));
    return BB_ELAUNCH;
  }
  return BB_OK;
}

BEVBERT_API int bevbert_version(void) { return 600; }  // 0.6.0: bevbert_pd_pano_rows (csrc/path_data.hip), entry point added

static const uint32_t* g_step_salt = nullptr;
const uint32_t* bb_step_salt() { return g_step_salt; }
BEVBERT_API int bevbert_set_step_salt(const void* device_word) {
  g_step_salt = static_cast<const uint32_t*>(device_word);
  return BB_OK;
}
// Slot array of the fused gradient norm (bevbert_multi_accum's NORM tasks, bevbert_sumsq_tasks): like the salt, a pointer
// read on the host at launch time and passed to the kernel as an argument.
static float* g_fold_norm_slots = nullptr;
static int g_fold_norm_capacity = 0;
float* bb_fold_norm_slots(int* capacity) {
  *capacity = g_fold_norm_capacity;
  return g_fold_norm_slots;
}
BEVBERT_API int bevbert_set_fold_norm_slots(float* slots, int capacity) {
  BB_REQUIRE(capacity >= 0 && capacity <= (1 << 20), "set_fold_norm_slots: capacity %d outside [0, 2^20]", capacity);
  g_fold_norm_slots = capacity > 0 ? slots : nullptr;
  g_fold_norm_capacity = g_fold_norm_slots ? capacity : 0;
  return BB_OK;
}
BEVBERT_API const char* bevbert_arch(void) { return "gfx950"; }

int attn_simple_fwd(const AttnArgs& a, int dtype, hipStream_t st);
int attn_simple_bwd(const AttnArgs& a, int dtype, hipStream_t st);
int attn_delta(const AttnArgs& a, float* delta, int dtype, hipStream_t st);
int attn_mfma_fwd(const AttnArgs& a, hipStream_t st);
int attn_mfma_bwd(const AttnArgs& a, hipStream_t st);
int attn_mfma_bwd1(const AttnArgs& a, hipStream_t st);
bool attn_mfma_bwd1_supported(const AttnArgs& a);
int attn_fwd2(const AttnArgs& a, hipStream_t st);
int attn_fwd2_f16(const AttnArgs& a, hipStream_t st);
bool attn_fwd2_supported(const AttnArgs& a);
int attn_drop_bits(const AttnArgs& a, uint64_t* bits_f, uint64_t* bits_b, uint32_t* bits_l, hipStream_t st);
int attn_fwd4(const AttnArgs& a, const uint32_t* bits_l, hipStream_t st);
bool attn_fwd4_supported(const AttnArgs& a, int ncu, bool forced);
int attn_fwd4_workgroups();
int attn_bwd2(const AttnArgs& a, hipStream_t st);
bool attn_bwd2_supported(const AttnArgs& a);
int attn_bwd3(const AttnArgs& a, hipStream_t st);
int attn_f32_fwd(const AttnArgs& a, hipStream_t st);
int attn_f32_bwd(const AttnArgs& a, hipStream_t st);
bool attn_f32_supported(const AttnArgs& a, int dtype, bool bwd);
bool attn_bwd3_supported(const AttnArgs& a);
int attn_small_fwd(const AttnArgs& a, hipStream_t st);
bool attn_small_fwd_supported(const AttnArgs& a);
int attn_small_bwd(const AttnArgs& a, hipStream_t st);
bool attn_small_bwd_supported(const AttnArgs& a);
int attn_small_bwd2(const AttnArgs& a, hipStream_t st);
bool attn_small_bwd2_supported(const AttnArgs& a);
int attn_short_fwd(const AttnArgs& a, bool bits_ready, hipStream_t st);
bool attn_short_fwd_supported(const AttnArgs& a, bool bits_ready);
int attn_short_bwd(const AttnArgs& a, hipStream_t st);
bool attn_short_bwd_supported(const AttnArgs& a);

// The keep-bit workspace of a call holds the matrix three times: [forward layout | backward layout | per-lane layout of
// attn_fwd4.hip], see attn_fwd2.hip
static int64_t bits_words_one(int B, int nh, int Lq, int Lk) {
  return (int64_t)B * nh * ((Lq + 127) / 128 * 8) * ((Lk + 63) / 64) * 16;
}

// =============================================================================================
// Kernel selection: attn_plan_fwd / attn_plan_bwd are the whole rule -- pure functions of the argument block, the dtype,
// the impl and the environment switches (AttnKnobs, read per call); the *_supported() predicates of the kernel files
// speak about shapes and operands only.  bevbert_attn_plan() evaluates the same functions without launching.
// =============================================================================================
#define ATTN_KERNELS(X)                                                                                             \
  X(attn_short_fwd) X(attn_small_fwd) X(attn_fwd4) X(attn_fwd2) X(attn_mfma_fwd) X(attn_f32_fwd) X(attn_simple_fwd) \
  X(attn_short_bwd) X(attn_small_bwd2) X(attn_small_bwd) X(attn_bwd3) X(attn_bwd2) X(attn_mfma_bwd1)                \
  X(attn_mfma_bwd) X(attn_f32_bwd) X(attn_simple_bwd)
#define X(name) AK_##name,
enum AttnKernel { ATTN_KERNELS(X) };
#undef X
#define X(name) #name,
static const char* const ATTN_KERNEL_NAMES[] = {ATTN_KERNELS(X)};
#undef X

struct AttnKnobs {
  bool fwd_gen1;    // BEVBERT_ATTN_FWD=1
  bool bwd_gen1;    // BEVBERT_ATTN_BWD=1
  bool bwd_split;   // BEVBERT_ATTN_BWD=split
  bool bwd3;        // BEVBERT_ATTN_BWD3 (=0 switches off)
  bool small;       // BEVBERT_ATTN_SMALL=1
  bool small_bwd2;  // BEVBERT_ATTN_SMALL_BWD (=0 switches off)
  bool short_on;    // BEVBERT_ATTN_SHORT (=0 switches off)
  bool f32_simple;  // BEVBERT_ATTN_F32=simple
  int fwd4;         // BEVBERT_ATTN_FWD4: 0 off, 1 every supported shape, anything else / unset: the occupancy rule
  int ncu;          // workgroups of the persistent forward: the device's CU count, or BEVBERT_FWD4_WGS
};

// ncu > 0: plan for a device with that many CUs (touches no device); otherwise this device's (attn_fwd4.hip)
static AttnKnobs attn_read_knobs(int ncu) {
  const auto first = [](const char* name) { const char* v = getenv(name); return v ? v[0] : '\0'; };
  const char* fwd4 = getenv("BEVBERT_ATTN_FWD4");
  AttnKnobs kn;
  kn.fwd_gen1 = first("BEVBERT_ATTN_FWD") == '1';
  kn.bwd_gen1 = first("BEVBERT_ATTN_BWD") == '1';
  kn.bwd_split = first("BEVBERT_ATTN_BWD") == 's';
  kn.bwd3 = first("BEVBERT_ATTN_BWD3") != '0';
  kn.small = first("BEVBERT_ATTN_SMALL") == '1';
  kn.small_bwd2 = first("BEVBERT_ATTN_SMALL_BWD") != '0';
  kn.short_on = first("BEVBERT_ATTN_SHORT") != '0';
  kn.f32_simple = first("BEVBERT_ATTN_F32") == 's';
  kn.fwd4 = fwd4 ? atoi(fwd4) : -1;
  kn.ncu = ncu > 0 ? ncu : attn_fwd4_workgroups();
  return kn;
}

// impl: 0 = auto (bf16 -> MFMA, f32 -> exact), 1 = force exact kernels, 2 = force MFMA (bf16 only),
//       3 = MFMA with the two-kernel backward even where the single-pass backward applies (tests, A/B measurements)
static int pick_impl(int dtype, int impl) {
  if (impl == 0) return dtype == BB_BF16 ? 2 : 1;
  return impl;
}

// Small score matrices with dropout (text 80 x 80, panoramas 36 x 36, the global map): their kernels are bound by
// launch latency, the inline hash of the round-2 forward hides in it, and that forward leaves the keep bits behind
// for the backward anyway -- a separate bit-generation launch per site only adds launches (35 of 71 per three steps).
// (Lk > 256: the 7+1-wave backward wants the backward-layout bits, which only bevbert_attn_drop_bits writes)
static bool attn_scores_small(const AttnArgs& a) { return (int64_t)a.Lq * a.Lk < 32768 && a.Lk <= 256; }

// Should the caller fill the keep-bit workspace ahead of the forward (bevbert_attn_drop_bits, bits_ready = 1)?  Not for
// small score matrices, and not for attn_small.hip (opt-in), which hashes inline whatever the query count.
static bool attn_bits_ahead(const AttnArgs& a, const AttnKnobs& kn) {
  return !attn_scores_small(a) && !(kn.small && attn_small_fwd_supported(a));
}

struct AttnPlan {
  AttnKernel kernel;
  bool gen_bits;   // attn_drop_bits has to fill the workspace before the kernel runs
};

static AttnPlan attn_plan_fwd(const AttnArgs& a, int dtype, int impl, bool bits_ready, const AttnKnobs& kn) {
  const int im = pick_impl(dtype, impl);
  if (im == 2 || im == 3) {
    // BEVBERT_ATTN_FWD=1: the round-2 forward (hashes the dropout mask inline) for A/B measurements and as the on-GPU
    // cross-check of the second-generation kernel
    if (kn.fwd_gen1) return {AK_attn_mfma_fwd, false};
    // round 6: key sequences up to 96 without a graph bias (text, panoramas, global map, BEV <- text): attn_short.hip, one
    // round of workgroups per launch; BEVBERT_ATTN_SHORT=0 falls through to the kernels of rounds 2-5
    if (!kn.small && kn.short_on && attn_short_fwd_supported(a, bits_ready)) return {AK_attn_short_fwd, false};
    // BEVBERT_ATTN_SMALL=1 (read per call): short key sequences without a graph bias go to the one-tile-set kernels of
    // attn_small.hip.  Measured (r03y, B = 64, 80 x 80, p = 0.1): 17.6 us against 12.3 + 5.9 us (tiled forward + bit
    // generation), backward 30.6 against 27.7 us -- no gain, so the tiled kernels stay the default.
    if (kn.small && attn_small_fwd_supported(a)) return {AK_attn_small_fwd, false};
    // small score matrices whose bits nobody made ahead (attn_scores_small) and the graph bias of the global map (a few
    // dozen nodes): the round-2 forward
    const bool hash_inline = a.drop_p > 0.f && attn_scores_small(a) && !bits_ready;
    if (hash_inline || !attn_fwd2_supported(a)) return {AK_attn_mfma_fwd, false};
    const bool gen_bits = a.drop_p > 0.f && !bits_ready;
    // BEV self-attention (441 x 441) at the workload's batch: the persistent forward, by its occupancy rule (attn_fwd4.hip)
    if (kn.fwd4 != 0 && attn_fwd4_supported(a, kn.ncu, kn.fwd4 == 1)) return {AK_attn_fwd4, gen_bits};
    // everything else without a bias: BEV self-attention at small batches, text -> BEV (80 x 441), inference
    return {AK_attn_fwd2, gen_bits};
  }
  // exact arithmetic: fp32 tensors on the fp32 matrix instructions (attn_f32.hip); bf16 storage / BEVBERT_ATTN_F32=simple on
  // the wave-per-row kernels
  if (!kn.f32_simple && attn_f32_supported(a, dtype, false)) return {AK_attn_f32_fwd, false};
  return {AK_attn_simple_fwd, false};
}

static AttnKernel attn_plan_bwd(const AttnArgs& a, int dtype, int impl, const AttnKnobs& kn) {
  const int im = pick_impl(dtype, impl);
  if (im == 2 || im == 3) {
    // one pass over the scores when all keys of a (batch, head) fit one workgroup (attn_bwd1.hip); BEVBERT_ATTN_BWD=split
    // forces the two-kernel path (A/B measurements), and so does impl 3
    if (kn.bwd_split || im == 3) return AK_attn_mfma_bwd;
    // BEVBERT_ATTN_BWD=1: the round-2 single-pass kernel where the 7+1-wave kernel (attn_bwd7p1.hip) would run
    if (!kn.bwd_gen1) {
      // round 6: query and key sequences up to 96 without a graph bias (80 x 80 text, 36 x 36 panoramas, 17 x 80 / 80 x 17
      // map <-> text): attn_short.hip
      if (!kn.small && kn.short_on && attn_short_bwd_supported(a)) return AK_attn_short_bwd;
      // query and key sequences up to 96 (80 x 80 text, 36 x 36 panoramas, 17 x 80 / 80 x 17 map <-> text): independent
      // query-owner / key-owner waves, attn_small.hip.  BEVBERT_ATTN_SMALL_BWD=0 keeps the single-pass kernel (A/B).
      if (kn.small_bwd2 && attn_small_bwd2_supported(a)) return AK_attn_small_bwd2;
      // BEVBERT_ATTN_SMALL=1: the one-wave backward for short key sequences and any query count (BEV <- text, 441 x 80)
      if (kn.small && attn_small_bwd_supported(a)) return AK_attn_small_bwd;
      // BEV self-attention and text -> BEV (256 < Lk <= 448, no bias): the 7+1-wave kernel.  BEVBERT_ATTN_BWD3=0: its
      // round-3 loop (attn_bwd7p1.hip, GEN 2) where the round-5 one (GEN 3) would run -- A/B measurements and the on-GPU
      // cross-check
      if (kn.bwd3 && attn_bwd3_supported(a)) return AK_attn_bwd3;
      if (attn_bwd2_supported(a)) return AK_attn_bwd2;
    }
    // BEV <- text (441 x 80), the global map with its graph bias, whatever the kernels above left
    if (attn_mfma_bwd1_supported(a)) return AK_attn_mfma_bwd1;
    return AK_attn_mfma_bwd;   // keys beyond 448 (a bias: 128), dropout without keep bits
  }
  if (!kn.f32_simple && attn_f32_supported(a, dtype, true)) return AK_attn_f32_bwd;
  return AK_attn_simple_bwd;
}

// Which kernel the last bevbert_attn_fwd / _bwd call of this thread was dispatched to: test / bench introspection
static thread_local const char* g_attn_path[2] = {"", ""};
BEVBERT_API const char* bevbert_attn_last_path(int backward) { return g_attn_path[backward ? 1 : 0]; }

static int fill_common(AttnArgs& a, const void* q, const void* k, const void* v, const float* key_mask,
                       const float* bias, const int64_t* strides, int B, int nh, int Lq, int Lk, int head_dim,
                       float scale, float drop_p, uint64_t seed, uint64_t offset) {
  BB_REQUIRE(head_dim == ATTN_D, "attention: head_dim=%d unsupported (kernels are specialised for 64)", head_dim);
  BB_REQUIRE(B > 0 && nh > 0 && Lq > 0 && Lk > 0, "attention: empty problem B=%d nh=%d Lq=%d Lk=%d", B, nh, Lq, Lk);
  BB_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "attention: dropout p=%f", drop_p);
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.key_mask = key_mask; a.bias = bias;
  a.ldq = strides[0]; a.ldk = strides[1]; a.ldv = strides[2]; a.ldo = strides[3];
  a.bsq = strides[4]; a.bsk = strides[5]; a.bsv = strides[6]; a.bso = strides[7];
  a.B = B; a.nh = nh; a.Lq = Lq; a.Lk = Lk; a.scale = scale;
  a.drop_p = drop_p; a.keep_scale = 1.0f / (1.0f - drop_p); a.drop_thr = bb_drop_threshold(drop_p); a.drop_key = bb_site_key(seed, offset); a.salt = bb_step_salt();
  a.Lk2 = (Lk + 1) & ~1;
  a.nq16 = (Lq + 127) / 128 * 8;
  a.nk64 = (Lk + 63) / 64;
  BB_REQUIRE((double)B * nh * Lq * a.Lk2 < 4294967296.0, "attention: more than 2^32 score elements per launch");
  return BB_OK;
}

static int check_dtype(const char* who, int dtype, int impl) {
  BB_REQUIRE(dtype == BB_F32 || dtype == BB_BF16, "%s: dtype %d unsupported", who, dtype);
  const int im = pick_impl(dtype, impl);
  BB_REQUIRE((im != 2 && im != 3) || dtype == BB_BF16, "%s: the MFMA path takes bf16 tensors", who);
  return BB_OK;
}

BEVBERT_API int bevbert_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                                 const float* key_mask, const float* bias, const int64_t* strides, int B, int nh,
                                 int Lq, int Lk, int head_dim, float scale, int dtype, int impl, float drop_p,
                                 uint64_t seed, uint64_t offset, uint64_t* drop_bits, int bits_ready,
                                 hipStream_t stream) {
  AttnArgs a;
  int rc = fill_common(a, q, k, v, key_mask, bias, strides, B, nh, Lq, Lk, head_dim, scale, drop_p, seed, offset);
  if (rc != BB_OK) return rc;
  a.o = o; a.lse = lse; a.drop_bits = drop_bits;
  a.drop_bits_b = drop_bits ? drop_bits + bits_words_one(B, nh, Lq, Lk) : nullptr;
  if ((rc = check_dtype("attn_fwd", dtype, impl)) != BB_OK) return rc;
  const AttnPlan plan = attn_plan_fwd(a, dtype, impl, bits_ready != 0, attn_read_knobs(0));
  uint32_t* bits_l = drop_bits ? reinterpret_cast<uint32_t*>(drop_bits + 2 * bits_words_one(B, nh, Lq, Lk)) : nullptr;
  if (plan.gen_bits && (rc = attn_drop_bits(a, a.drop_bits, a.drop_bits_b, bits_l, stream)) != BB_OK) return rc;
  g_attn_path[0] = ATTN_KERNEL_NAMES[plan.kernel];
  switch (plan.kernel) {
    case AK_attn_short_fwd: return attn_short_fwd(a, bits_ready != 0, stream);
    case AK_attn_small_fwd: return attn_small_fwd(a, stream);
    case AK_attn_fwd4: return attn_fwd4(a, bits_l, stream);
    case AK_attn_fwd2: return attn_fwd2(a, stream);
    case AK_attn_mfma_fwd: return attn_mfma_fwd(a, stream);
    case AK_attn_f32_fwd: return attn_f32_fwd(a, stream);
    default: return attn_simple_fwd(a, dtype, stream);
  }
}

BEVBERT_API int bevbert_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                 const float* lse, float* delta_ws, void* dq, void* dk, void* dv, float* dbias,
                                 const float* key_mask, const float* bias, const int64_t* strides, int B, int nh,
                                 int Lq, int Lk, int head_dim, float scale, int dtype, int impl, float drop_p,
                                 uint64_t seed, uint64_t offset, const uint64_t* drop_bits, hipStream_t stream) {
  AttnArgs a;
  int rc = fill_common(a, q, k, v, key_mask, bias, strides, B, nh, Lq, Lk, head_dim, scale, drop_p, seed, offset);
  if (rc != BB_OK) return rc;
  a.drop_bits = const_cast<uint64_t*>(drop_bits);
  a.drop_bits_b = drop_bits ? a.drop_bits + bits_words_one(B, nh, Lq, Lk) : nullptr;
  if ((rc = check_dtype("attn_bwd", dtype, impl)) != BB_OK) return rc;
  BB_REQUIRE(lse != nullptr && delta_ws != nullptr, "attn_bwd: lse and the (B,nh,Lq) delta workspace are required");
  a.o = const_cast<void*>(o); a.dout = dout; a.lse = const_cast<float*>(lse); a.delta = delta_ws;
  a.dq = dq; a.dk = dk; a.dv = dv; a.dbias = dbias;
  const AttnKernel kernel = attn_plan_bwd(a, dtype, impl, attn_read_knobs(0));
  // the MFMA kernels compute delta themselves (the dQ kernel publishes it for the dK/dV kernel), and so does the exact
  // kernel on bf16 storage, where sum_d dO O would carry the rounding of the stored O (attn_simple.hip)
  if ((kernel == AK_attn_f32_bwd || (kernel == AK_attn_simple_bwd && dtype == BB_F32)) &&
      (rc = attn_delta(a, delta_ws, dtype, stream)) != BB_OK)
    return rc;
  g_attn_path[1] = ATTN_KERNEL_NAMES[kernel];
  switch (kernel) {
    case AK_attn_short_bwd: return attn_short_bwd(a, stream);
    case AK_attn_small_bwd2: return attn_small_bwd2(a, stream);
    case AK_attn_small_bwd: return attn_small_bwd(a, stream);
    case AK_attn_bwd3: return attn_bwd3(a, stream);
    case AK_attn_bwd2: return attn_bwd2(a, stream);
    case AK_attn_mfma_bwd1: return attn_mfma_bwd1(a, stream);
    case AK_attn_mfma_bwd: return attn_mfma_bwd(a, stream);
    case AK_attn_f32_bwd: return attn_f32_bwd(a, stream);
    default: return attn_simple_bwd(a, dtype, stream);
  }
}

// float16 operands: the forward-only instance of attn_fwd2.hip, outside the dispatch plan (no mask, bias, dropout or lse)
BEVBERT_API int bevbert_attn_f16_fwd(const void* q, const void* k, const void* v, void* o, const int64_t* strides, int B,
                                     int nh, int Lq, int Lk, int head_dim, float scale, hipStream_t stream) {
  BB_REQUIRE(q != nullptr && k != nullptr && v != nullptr && o != nullptr && strides != nullptr,
             "attn_f16_fwd: q, k, v, o and strides must not be NULL");
  AttnArgs a;
  int rc = fill_common(a, q, k, v, nullptr, nullptr, strides, B, nh, Lq, Lk, head_dim, scale, 0.f, 0, 0);
  if (rc != BB_OK) return rc;
  a.o = o;
  const int64_t width = (int64_t)nh * ATTN_D;
  BB_REQUIRE(a.ldq >= width && a.ldk >= width && a.ldv >= width && a.ldo >= width,
             "attn_f16_fwd: row strides below nh * 64 = %ld", (long)width);
  BB_REQUIRE(a.bsq >= 0 && a.bsk >= 0 && a.bsv >= 0 && a.bso >= 0, "attn_f16_fwd: negative batch stride");
  return attn_fwd2_f16(a, stream);
}

// An argument block with the shape and the presence flags of a call and operands that pass every alignment check
// (null pointers, zero strides): what the plan functions look at, for the two entries below that launch nothing.
static void fill_shape_only(AttnArgs& a, int B, int nh, int Lq, int Lk, bool has_key_mask, bool has_bias, float drop_p,
                            bool has_bits, bool want_dbias) {
  alignas(16) static char present[16];
  memset(&a, 0, sizeof(a));
  a.B = B; a.nh = nh; a.Lq = Lq; a.Lk = Lk; a.drop_p = drop_p;
  if (has_key_mask) a.key_mask = reinterpret_cast<const float*>(present);
  if (has_bias) a.bias = reinterpret_cast<const float*>(present);
  if (has_bits) a.drop_bits = a.drop_bits_b = reinterpret_cast<uint64_t*>(present);
  if (want_dbias) a.dbias = reinterpret_cast<float*>(present);
}

BEVBERT_API int bevbert_attn_bits_ahead(int Lq, int Lk, int has_bias) {
  AttnArgs a;
  fill_shape_only(a, 1, 1, Lq, Lk, false, has_bias != 0, 0.f, false, false);
  return attn_bits_ahead(a, attn_read_knobs(1)) ? 1 : 0;     // no rule here looks at the CU count
}

BEVBERT_API const char* bevbert_attn_plan(int B, int nh, int Lq, int Lk, int dtype, int impl, int has_key_mask,
                                          int has_bias, float drop_p, int has_bits, int bits_ready, int want_dbias,
                                          int ncu, int backward) {
  if (check_dtype("attn_plan", dtype, impl) != BB_OK) return "";
  AttnArgs a;
  fill_shape_only(a, B, nh, Lq, Lk, has_key_mask != 0, has_bias != 0, drop_p, has_bits != 0, want_dbias != 0);
  const AttnKnobs kn = attn_read_knobs(ncu);
  return ATTN_KERNEL_NAMES[backward ? attn_plan_bwd(a, dtype, impl, kn) : attn_plan_fwd(a, dtype, impl, bits_ready != 0, kn).kernel];
}

// Size of the keep-bit matrix of an attention call (64-bit words), see attn_common.h.
BEVBERT_API int64_t bevbert_attn_drop_bits_words(int B, int nh, int Lq, int Lk) {
  return 3 * bits_words_one(B, nh, Lq, Lk);
}

// Fill the keep-bit workspace of one attention call ahead of its forward (any stream: the mask is a pure function of
// (seed, offset, step salt, element index)); pass bits_ready = 1 to bevbert_attn_fwd afterwards.
BEVBERT_API int bevbert_attn_drop_bits(uint64_t* drop_bits, int B, int nh, int Lq, int Lk, float drop_p, uint64_t seed,
                                       uint64_t offset, hipStream_t stream) {
  BB_REQUIRE(drop_bits != nullptr && drop_p > 0.f && drop_p < 1.f, "attn_drop_bits: workspace and 0 < p < 1 required");
  AttnArgs a;
  const int64_t st[8] = {64, 64, 64, 64, 64, 64, 64, 64};
  int rc = fill_common(a, nullptr, nullptr, nullptr, nullptr, nullptr, st, B, nh, Lq, Lk, ATTN_D, 1.f, drop_p, seed, offset);
  if (rc != BB_OK) return rc;
  const int64_t one = bits_words_one(B, nh, Lq, Lk);
  return attn_drop_bits(a, drop_bits, drop_bits + one, reinterpret_cast<uint32_t*>(drop_bits + 2 * one), stream);
}
