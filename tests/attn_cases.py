"""Inputs, fp64 reference, gates and the case table of tests/test_gpu_attention_edges.py, on the CPU: the GPU test runs the
attention kernels on exactly these tensors, and tests/test_attn_refs_host.py pins the closed-form gradients to autograd,
measures what a bf16 / fp32 restatement needs of the gates, shows that one wrong key at a tile edge leaves them, and holds the
case table to the dispatch plan.  Nothing here touches the library.

Layout: q, do (B, Lq, nh * 64); k, v (B, Lk, nh * 64); key_mask (B, Lk) and bias (B, Lq, Lk) additive fp32; keep
(B, nh, Lq, Lk) bool; lse and the per-head quantities (B, nh, Lq[, Lk])."""
import collections
import math

import torch

D = 64
SCALE = 1.0 / math.sqrt(D)
U24, U18, U8 = 2.0 ** -24, 2.0 ** -18, 2.0 ** -8
C16 = 4.0         # bf16 kernels: units of 2^-8 b_x.  emulate_bf16 needs 0.91 on the CPU (host test), the kernels 0.90
C32 = 114.0       # fp32 kernels: units of 2^-24 b_x = 4 x the 28.3 torch's fp32 composition needs on the CPU (host test)
QUANTITIES = ("o", "lse", "dq", "dk", "dv", "dbias")
MASKS = (None, "holes", "holes_inf")
MUTATIONS = ("drop", "mask", "keep", "swap_v")
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}


def make_inputs(B, nh, Lq, Lk, dtype, mask, bias, seed):
    """(q, k, v, do, key_mask, bias): q and k are 1.5 randn (raw scores with a standard deviation of about 2.25), v and do
    randn, all already rounded to ``dtype``.  mask "holes" keeps each key with probability 0.6 independently per sample (key 0
    always), masked value -10000; "holes_inf" the same with -inf: no row is fully masked.  bias: 0.5 randn(B, Lq, Lk)."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * Lq + Lk)
    H = nh * D
    q = (1.5 * torch.randn(B, Lq, H, generator=g)).to(dtype)
    k = (1.5 * torch.randn(B, Lk, H, generator=g)).to(dtype)
    v = torch.randn(B, Lk, H, generator=g).to(dtype)
    do = torch.randn(B, Lq, H, generator=g).to(dtype)
    km = None
    if mask is not None:
        assert mask in ("holes", "holes_inf"), mask
        kept = torch.rand(B, Lk, generator=g) < 0.6
        kept[:, 0] = True
        km = torch.zeros(B, Lk).masked_fill(~kept, -10000.0 if mask == "holes" else float("-inf"))
    b = 0.5 * torch.randn(B, Lq, Lk, generator=g) if bias else None
    return q, k, v, do, km, b


def _heads(t):
    B, L, H = t.shape
    return t.reshape(B, L, H // D, D).permute(0, 2, 1, 3)


def _rows(t):
    B, nh, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, nh * D)


def reference(q, k, v, do, scale, key_mask=None, bias=None, keep=None, p=0.0):
    """float64, gradients in closed form.  Returns a dict with o, lse, dq, dk, dv, dbias (per head) and the bound tensors
    b_o ... b_lse the gates are made of (module docstring of the GPU test)."""
    Q, K, V, DO = (_heads(t.double()) for t in (q, k, v, do))
    S = scale * (Q @ K.transpose(-1, -2))
    if key_mask is not None:
        S = S + key_mask.double()[:, None, None, :]
    if bias is not None:
        S = S + bias.double()[:, None]
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    ks = torch.ones_like(P) if keep is None else keep.double() / (1.0 - p)
    Pd = P * ks
    O = Pd @ V
    dPd = DO @ V.transpose(-1, -2)
    delta = (O * DO).sum(-1, keepdim=True)
    dS = P * (ks * dPd - delta)
    e_S = P * (ks * dPd.abs() + delta.abs() + (O.abs() * DO.abs()).sum(-1, keepdim=True))
    live = torch.ones_like(S[:, :1, :1]) if key_mask is None else (key_mask == 0).double()[:, None, None, :]
    reach = scale * (Q.abs() @ K.abs().transpose(-1, -2))
    return {
        "o": _rows(O), "lse": lse, "dq": _rows(scale * (dS @ K)), "dk": _rows(scale * (dS.transpose(-1, -2) @ Q)),
        "dv": _rows(Pd.transpose(-1, -2) @ DO), "dbias": dS,
        "b_o": _rows(Pd @ V.abs()), "b_dv": _rows(Pd.transpose(-1, -2) @ DO.abs()),
        "b_dq": _rows(scale * (e_S @ K.abs())), "b_dk": _rows(scale * (e_S.transpose(-1, -2) @ Q.abs())),
        "b_dbias": e_S, "b_lse": 1.0 + (reach * live).amax(-1),
    }


def gates(ref, kind):
    """Elementwise bounds of |got - want| per quantity.  kind "bf16": the MFMA kernels (C16 units of 2^-8 b_x, plus the
    rounding of a bf16 result; dbias is an fp32 result); "f32": the exact kernels on fp32 tensors (C32 units of 2^-24 b_x);
    "exact16": the exact kernels on bf16 storage (the fp32 gate plus the rounding of the bf16 results).  lse: 2^-18 b_lse --
    a 64-term fp32 dot product errs by at most 64 x 2^-24 sum |q||k|, one more such unit covers exp2, log2 and the row sum."""
    assert kind in ("bf16", "f32", "exact16"), kind
    unit = C16 * U8 if kind == "bf16" else C32 * U24
    out = {"lse": U18 * ref["b_lse"], "dbias": unit * ref["b_dbias"]}
    for name in ("o", "dq", "dk", "dv"):
        out[name] = unit * ref["b_" + name] + (0.0 if kind == "f32" else U8 * ref[name].abs())
    return out


def units(got, ref, kind):
    """Worst |got - want| per quantity in the units of its gate (what C16 / C32 would have to be), the output-rounding term
    taken off first; lse in units of 2^-18 b_lse."""
    unit = U8 if kind == "bf16" else U24
    out = {}
    for name in QUANTITIES:
        if name not in got or got[name] is None:
            continue
        err = (got[name].double() - ref[name]).abs()
        if name == "lse":
            out[name] = float((err / (U18 * ref["b_lse"])).max())
            continue
        if name != "dbias" and kind != "f32":
            err = (err - U8 * ref[name].abs()).clamp_min(0.0)
        b = unit * ref["b_" + name]
        out[name] = float(torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300)).max())
    return out


def compose_f32(q, k, v, do, scale, key_mask=None, bias=None, keep=None, p=0.0, bf16=False):
    """Torch's own fp32 composition of the closed form (bf16 = False: the measure of C32), or emulate_bf16."""
    f = torch.float32
    r = (lambda t: t.bfloat16().to(f)) if bf16 else (lambda t: t)
    Q, K, V, DO = (_heads(t.to(f)) for t in (q, k, v, do))
    S = (Q @ K.transpose(-1, -2)) * f_(scale)
    if key_mask is not None:
        S = S + key_mask.to(f)[:, None, None, :]
    if bias is not None:
        S = S + bias.to(f)[:, None]
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    ks = torch.ones_like(P) if keep is None else keep.to(f) / f_(1.0 - p)
    Pd = r(P * ks)
    O = r(Pd @ V)
    dPd = DO @ V.transpose(-1, -2)
    delta = (O * DO).sum(-1, keepdim=True)
    dS32 = P * (ks * dPd - delta)
    dS = r(dS32)
    return {"o": _rows(O), "lse": lse, "dq": _rows(r((dS @ K) * f_(scale))), "dk": _rows(r((dS.transpose(-1, -2) @ Q) * f_(scale))),
            "dv": _rows(r(Pd.transpose(-1, -2) @ DO)), "dbias": dS32}


def f_(x):
    return torch.tensor(x, dtype=torch.float32)


def emulate_bf16(q, k, v, do, scale, key_mask=None, bias=None, keep=None, p=0.0):
    """The fp32 composition with P (after dropout), dS and the results rounded to bf16: what a correct MFMA kernel does, short of
    its fast exp2 and its running maximum.  dbias stays the unrounded fp32 dS."""
    return compose_f32(q, k, v, do, scale, key_mask, bias, keep, p, bf16=True)


def mutate(kind, j, q, k, v, do, scale, key_mask=None, bias=None, keep=None, p=0.0):
    """The fp64 reference of a kernel that goes wrong at key j in one way: "drop" leaves key j out; "mask" reads key j's mask
    entry from j + 1; "keep" uses key j's keep bit for j + 1; "swap_v" swaps the v rows of j and j + 1.  The gradients are
    those of the mutated forward with respect to the operands as the caller holds them, which is what a kernel with the same
    slip in both directions writes."""
    assert kind in MUTATIONS, kind
    Lk = k.shape[1]
    if kind == "drop":
        km = torch.zeros(k.shape[0], Lk) if key_mask is None else key_mask.clone()
        km[:, j] = float("-inf")
        return reference(q, k, v, do, scale, km, bias, keep, p)
    if kind == "mask":
        km = key_mask.clone()
        km[:, j] = key_mask[:, j + 1]
        return reference(q, k, v, do, scale, km, bias, keep, p)
    if kind == "keep":
        kp = keep.clone()
        kp[..., j + 1] = keep[..., j]
        return reference(q, k, v, do, scale, key_mask, bias, kp, p)
    perm = torch.arange(Lk)
    perm[j], perm[j + 1] = j + 1, j
    out = reference(q, k, v[:, perm], do, scale, key_mask, bias, keep, p)
    for name in ("dv", "b_dv"):
        out[name] = out[name][:, perm]
    return out


def boundary_indices(Lk):
    """Keys at which a tile of 16, 64 or 128 keys ends or begins, and the last two: every j of them with a key j + 1."""
    return sorted({j for j in (0, 15, 16, 63, 64, 127, 128, Lk - 2, Lk - 1) if 0 <= j and j + 1 < Lk})


# ----------------------------------------------------------------------------- the case table
# Every environment switch the attention sources read (AttnKnobs in capi.hip, and the workgroup count of attn_fwd4.hip):
# tests clear all of them before they set their own; tests/test_host_logic.py holds the sources and README.md to this list.
ATTN_KNOBS = ("BEVBERT_ATTN_FWD", "BEVBERT_ATTN_BWD", "BEVBERT_ATTN_BWD3", "BEVBERT_ATTN_SMALL", "BEVBERT_ATTN_SMALL_BWD",
              "BEVBERT_ATTN_SHORT", "BEVBERT_ATTN_FWD4", "BEVBERT_ATTN_F32", "BEVBERT_FWD4_WGS")
Case = collections.namedtuple("Case", "B nh Lq Lk dtype impl mask bias p bits knobs fwd bwd")
_A = "attn_"
SHORT0, SMALL1, FWD1, BWD1, BWD3_0 = ({"BEVBERT_ATTN_SHORT": "0"}, {"BEVBERT_ATTN_SMALL": "1"}, {"BEVBERT_ATTN_FWD": "1"},
                                      {"BEVBERT_ATTN_BWD": "1"}, {"BEVBERT_ATTN_BWD3": "0"})
SIMPLE = {"BEVBERT_ATTN_F32": "simple"}


def _fwd4(wgs, **more):
    return dict({"BEVBERT_ATTN_FWD4": "1", "BEVBERT_FWD4_WGS": str(wgs)}, **more)


def _c(Lq, Lk, mask, p, fwd, bwd, knobs=None, bias=False, bits=None, dtype="bf16", impl=2, B=2, nh=2):
    """bits: the keep-bit workspace of the call, "none" = no pointer, "empty" = passed with bits_ready = 0, "ready" = filled
    ahead by bevbert_attn_drop_bits; by default "empty" wherever a bf16 MFMA call has dropout."""
    if bits is None:
        bits = "empty" if p > 0 and dtype == "bf16" and impl != 1 else "none"
    return Case(B, nh, Lq, Lk, dtype, impl, mask, bias, p, bits, dict(knobs or {}), _A + fwd, _A + bwd)


N, H_, I_ = None, "holes", "holes_inf"
CASES = [
    # --- attn_short_fwd + attn_short_bwd: the default up to 96 x 96, every 16-tile count on both axes
    _c(1, 1, N, 0.0, "short_fwd", "short_bwd"),
    _c(16, 16, N, 0.1, "short_fwd", "short_bwd"),
    _c(17, 17, H_, 0.1, "short_fwd", "short_bwd"),
    _c(32, 33, I_, 0.1, "short_fwd", "short_bwd"),
    _c(33, 32, H_, 0.0, "short_fwd", "short_bwd"),
    _c(48, 49, H_, 0.1, "short_fwd", "short_bwd"),
    _c(49, 48, I_, 0.0, "short_fwd", "short_bwd"),
    _c(80, 81, I_, 0.1, "short_fwd", "short_bwd"),
    _c(81, 80, N, 0.1, "short_fwd", "short_bwd"),
    _c(96, 96, H_, 0.1, "short_fwd", "short_bwd"),
    _c(17, 15, I_, 0.1, "short_fwd", "short_bwd"),
    _c(96, 64, N, 0.0, "short_fwd", "short_bwd"),
    _c(1, 65, H_, 0.1, "short_fwd", "short_bwd"),
    _c(17, 95, I_, 0.1, "short_fwd", "short_bwd", bits="ready"),
    _c(96, 1, N, 0.1, "short_fwd", "short_bwd"),
    _c(1, 96, I_, 0.0, "short_fwd", "short_bwd"),
    # --- attn_short_fwd beyond 96 queries; the backward is the single-pass kernel in its 64- and 128-key forms
    _c(97, 64, H_, 0.1, "short_fwd", "mfma_bwd1"),
    _c(129, 65, I_, 0.1, "short_fwd", "mfma_bwd1"),
    _c(97, 96, N, 0.0, "short_fwd", "mfma_bwd1"),
    _c(129, 17, H_, 0.1, "short_fwd", "mfma_bwd1", bits="ready"),
    # --- attn_small_fwd (opt-in) + attn_small_bwd2: tile counts 2, 3, 5, 6
    _c(1, 1, N, 0.1, "small_fwd", "small_bwd2", SMALL1),
    _c(31, 16, H_, 0.1, "small_fwd", "small_bwd2", SMALL1),
    _c(32, 17, I_, 0.1, "small_fwd", "small_bwd2", SMALL1),
    _c(33, 32, N, 0.0, "small_fwd", "small_bwd2", SMALL1),
    _c(31, 33, H_, 0.1, "small_fwd", "small_bwd2", SMALL1),
    _c(32, 48, I_, 0.0, "small_fwd", "small_bwd2", SMALL1),
    _c(33, 49, H_, 0.1, "small_fwd", "small_bwd2", SMALL1),
    _c(1, 80, N, 0.1, "small_fwd", "small_bwd2", SMALL1),
    _c(32, 81, I_, 0.1, "small_fwd", "small_bwd2", SMALL1),
    _c(33, 96, H_, 0.0, "small_fwd", "small_bwd2", SMALL1),
    # --- attn_small_fwd + attn_small_bwd: more than 96 queries
    _c(97, 16, H_, 0.1, "small_fwd", "small_bwd", SMALL1),
    _c(129, 33, I_, 0.1, "small_fwd", "small_bwd", SMALL1),
    _c(300, 96, N, 0.0, "small_fwd", "small_bwd", SMALL1),
    _c(97, 96, H_, 0.1, "small_fwd", "small_bwd", SMALL1),
    # --- BEVBERT_ATTN_SHORT=0 up to 96 x 96: attn_small_bwd2 behind the tiled forwards
    _c(16, 1, N, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    _c(17, 16, H_, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    _c(48, 17, I_, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    _c(49, 32, N, 0.0, "fwd2", "small_bwd2", SHORT0),
    _c(80, 33, H_, 0.1, "fwd2", "small_bwd2", SHORT0, bits="ready"),
    _c(81, 48, I_, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    _c(96, 49, H_, 0.0, "fwd2", "small_bwd2", SHORT0),
    _c(16, 80, I_, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    _c(17, 81, N, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    _c(96, 96, I_, 0.1, "fwd2", "small_bwd2", SHORT0, bits="ready"),
    _c(1, 96, H_, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    _c(31, 63, H_, 0.1, "fwd2", "small_bwd2", SHORT0, bits="ready"),
    _c(32, 64, N, 0.0, "fwd2", "small_bwd2", SHORT0),
    _c(33, 65, I_, 0.1, "fwd2", "small_bwd2", SHORT0, bits="ready"),
    _c(64, 63, I_, 0.1, "mfma_fwd", "small_bwd2", SHORT0),
    # --- attn_fwd2 + attn_mfma_bwd1 up to 256 keys: the 128- and 256-key forms of the backward
    _c(127, 127, H_, 0.1, "fwd2", "mfma_bwd1", bits="ready"),
    _c(128, 128, N, 0.0, "fwd2", "mfma_bwd1"),
    _c(129, 129, I_, 0.1, "fwd2", "mfma_bwd1", bits="ready"),
    _c(1, 255, H_, 0.1, "fwd2", "mfma_bwd1", bits="ready"),
    _c(31, 256, I_, 0.0, "fwd2", "mfma_bwd1"),
    _c(257, 129, N, 0.1, "fwd2", "mfma_bwd1"),
    _c(128, 256, H_, 0.1, "fwd2", "mfma_bwd1"),
    # --- attn_mfma_bwd1 beyond 256 keys (BEVBERT_ATTN_BWD=1)
    _c(63, 257, H_, 0.1, "fwd2", "mfma_bwd1", BWD1),
    _c(64, 447, I_, 0.1, "fwd2", "mfma_bwd1", BWD1),
    _c(65, 448, N, 0.0, "fwd2", "mfma_bwd1", BWD1),
    # --- attn_fwd2 + attn_bwd3 / attn_bwd2: 256 < Lk <= 448
    _c(1, 257, H_, 0.1, "fwd2", "bwd3"),
    _c(63, 320, I_, 0.1, "fwd2", "bwd3"),
    _c(64, 447, N, 0.1, "fwd2", "bwd3"),
    _c(65, 448, H_, 0.0, "fwd2", "bwd3"),
    _c(32, 447, I_, 0.0, "fwd2", "bwd3"),
    _c(33, 448, N, 0.1, "fwd2", "bwd3"),
    _c(1, 257, I_, 0.1, "fwd2", "bwd2", BWD3_0),
    _c(63, 320, N, 0.0, "fwd2", "bwd2", BWD3_0),
    _c(64, 447, H_, 0.1, "fwd2", "bwd2", BWD3_0),
    _c(65, 448, I_, 0.1, "fwd2", "bwd2", BWD3_0),
    # --- attn_fwd4 (forced, 1 and 3 workgroups): 448-query items, more than one per head at 449 and 897 queries
    _c(257, 257, H_, 0.1, "fwd4", "bwd3", _fwd4(1)),
    _c(448, 320, N, 0.0, "fwd4", "bwd3", _fwd4(3)),
    _c(449, 448, I_, 0.1, "fwd4", "bwd3", _fwd4(1)),
    _c(897, 385, H_, 0.1, "fwd4", "bwd3", _fwd4(3)),
    _c(449, 320, H_, 0.1, "fwd4", "bwd2", _fwd4(3, BEVBERT_ATTN_BWD3="0")),
    _c(449, 257, N, 0.0, "fwd4", "bwd2", _fwd4(1, BEVBERT_ATTN_BWD3="0")),
    # --- beyond 448 keys: attn_fwd2 + the two-kernel backward
    _c(127, 449, H_, 0.1, "fwd2", "mfma_bwd"),
    _c(128, 513, I_, 0.1, "fwd2", "mfma_bwd"),
    _c(33, 513, N, 0.0, "fwd2", "mfma_bwd"),
    _c(32, 449, I_, 0.0, "fwd2", "mfma_bwd"),
    # --- impl 3: the two-kernel backward where the single-pass kernels apply
    _c(65, 65, H_, 0.1, "short_fwd", "mfma_bwd", impl=3),
    _c(129, 257, I_, 0.1, "fwd2", "mfma_bwd", impl=3),
    _c(129, 257, N, 0.0, "fwd2", "mfma_bwd", impl=3),
    # --- attn_mfma_fwd with a graph bias; per-head dbias from attn_mfma_bwd1 (Lk <= 128) and attn_mfma_bwd
    _c(1, 1, N, 0.0, "mfma_fwd", "mfma_bwd1", bias=True),
    _c(17, 17, H_, 0.1, "mfma_fwd", "mfma_bwd1", bias=True),
    _c(64, 64, I_, 0.1, "mfma_fwd", "mfma_bwd1", bias=True),
    _c(65, 65, H_, 0.0, "mfma_fwd", "mfma_bwd1", bias=True),
    _c(130, 128, N, 0.1, "mfma_fwd", "mfma_bwd1", bias=True),
    _c(1, 65, I_, 0.1, "mfma_fwd", "mfma_bwd1", bias=True),
    _c(64, 129, H_, 0.1, "mfma_fwd", "mfma_bwd", bias=True),
    _c(130, 200, I_, 0.0, "mfma_fwd", "mfma_bwd", bias=True),
    _c(17, 129, N, 0.1, "mfma_fwd", "mfma_bwd", bias=True, bits="none"),
    # --- attn_mfma_fwd without a bias (BEVBERT_ATTN_FWD=1, or dropout without a workspace)
    _c(65, 63, H_, 0.1, "mfma_fwd", "short_bwd", FWD1),
    _c(17, 449, I_, 0.1, "mfma_fwd", "mfma_bwd", bits="none"),
    _c(130, 449, N, 0.0, "mfma_fwd", "mfma_bwd", FWD1),
    _c(64, 200, H_, 0.1, "mfma_fwd", "mfma_bwd1"),
    _c(130, 128, I_, 0.0, "mfma_fwd", "mfma_bwd1", FWD1),
    # --- fp32 tensors: attn_f32_*
    _c(1, 1, N, 0.0, "f32_fwd", "f32_bwd", dtype="f32", impl=0),
    _c(63, 64, H_, 0.1, "f32_fwd", "f32_bwd", dtype="f32", impl=0),
    _c(64, 65, I_, 0.1, "f32_fwd", "f32_bwd", dtype="f32", impl=0),
    _c(65, 63, N, 0.1, "f32_fwd", "f32_bwd", dtype="f32", impl=0),
    _c(129, 257, H_, 0.0, "f32_fwd", "f32_bwd", dtype="f32", impl=0),
    _c(257, 129, I_, 0.1, "f32_fwd", "f32_bwd", dtype="f32", impl=0, bias=True),
    _c(1, 257, I_, 0.0, "f32_fwd", "f32_bwd", dtype="f32", impl=0),
    _c(257, 1, N, 0.1, "f32_fwd", "f32_bwd", dtype="f32", impl=0),
    _c(64, 129, H_, 0.1, "f32_fwd", "f32_bwd", dtype="f32", impl=0, bias=True),
    # --- attn_simple_*: fp32 tensors by the knob, bf16 storage by impl 1
    _c(1, 1, N, 0.0, "simple_fwd", "simple_bwd", SIMPLE, dtype="f32", impl=0),
    _c(64, 65, H_, 0.1, "simple_fwd", "simple_bwd", SIMPLE, dtype="f32", impl=0),
    _c(65, 130, I_, 0.1, "simple_fwd", "simple_bwd", SIMPLE, dtype="f32", impl=0, bias=True),
    _c(130, 64, N, 0.1, "simple_fwd", "simple_bwd", SIMPLE, dtype="f32", impl=0),
    _c(1, 64, H_, 0.0, "simple_fwd", "simple_bwd", impl=1),
    _c(64, 1, N, 0.1, "simple_fwd", "simple_bwd", impl=1),
    _c(65, 65, I_, 0.1, "simple_fwd", "simple_bwd", impl=1, bias=True),
    _c(130, 130, H_, 0.1, "simple_fwd", "simple_bwd", impl=1),
    _c(130, 65, N, 0.0, "simple_fwd", "simple_bwd", impl=1),
]

# the lengths each kernel's cases have to contain (the launch code's switches; the issue's table)
_SHORT_AXIS = (1, 16, 17, 32, 33, 48, 49, 80, 81, 96)
REQUIRED = {
    "attn_short_fwd": {"Lk": (1, 15, 16, 17, 33, 64, 65, 95, 96), "Lq": (1, 17, 96, 97, 129)},
    "attn_small_fwd": {"Lk": (1, 16, 17, 32, 33, 48, 49, 80, 81, 96), "Lq": (1, 31, 32, 33, 97)},
    "attn_fwd2": {"Lk": (63, 64, 65, 127, 128, 129, 255, 256, 257, 447, 448, 449, 513), "Lq": (1, 31, 32, 33, 127, 128, 129, 257)},
    "attn_fwd4": {"pairs": ((257, 257), (448, 320), (449, 448), (897, 385)), "wgs": ("1", "3")},
    "attn_mfma_fwd": {"Lk": (1, 17, 63, 64, 65, 128, 129, 200, 449), "Lq": (1, 17, 64, 65, 130)},
    "attn_short_bwd": {"Lk": _SHORT_AXIS, "Lq": _SHORT_AXIS},
    "attn_small_bwd2": {"Lk": _SHORT_AXIS, "Lq": _SHORT_AXIS},
    "attn_small_bwd": {"Lq": (97, 129, 300), "Lk": (16, 33, 96)},
    "attn_mfma_bwd1": {"Lk": (64, 65, 128, 129, 256, 257, 447, 448), "bias_Lk": (1, 17, 64, 65, 128)},
    "attn_bwd3": {"Lk": (257, 320, 447, 448), "Lq": (1, 63, 64, 65, 449)},
    "attn_bwd2": {"Lk": (257, 320, 447, 448), "Lq": (1, 63, 64, 65, 449)},
    "attn_mfma_bwd": {"Lk": (449, 513), "bias_Lk": (129, 200), "impl3": ((65, 65), (129, 257))},
    "attn_f32_fwd": {"Lk": (1, 63, 64, 65, 129, 257), "Lq": (1, 63, 64, 65, 129, 257)},
    "attn_f32_bwd": {"Lk": (1, 63, 64, 65, 129, 257), "Lq": (1, 63, 64, 65, 129, 257)},
    "attn_simple_fwd": {"Lk": (1, 64, 65, 130), "Lq": (1, 64, 65, 130), "both_dtypes": True},
    "attn_simple_bwd": {"Lk": (1, 64, 65, 130), "Lq": (1, 64, 65, 130), "both_dtypes": True},
}


def case_id(c):
    knobs = ",".join(f"{k.replace('BEVBERT_', '')}={v}" for k, v in sorted(c.knobs.items()))
    return (f"{c.fwd[5:]}+{c.bwd[5:]}-{c.Lq}x{c.Lk}-{c.dtype}-impl{c.impl}-{c.mask or 'nomask'}-{'bias' if c.bias else 'nobias'}"
            f"-p{c.p}-{c.bits}{'-' + knobs if knobs else ''}")


def gate_kind(c):
    return "f32" if c.dtype == "f32" else ("exact16" if c.impl == 1 else "bf16")


def plan_row(c):
    """The case as a row of ATTN_PLAN_ROWS (tests/test_host_logic.py), for attn_plan."""
    return (c.B, c.Lq, c.Lk, c.dtype, c.impl, c.bias, c.p, c.bits, c.knobs)
