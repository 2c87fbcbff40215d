"""Inputs, bound, cases and a CPU emulation for the float16 attention forward (csrc/attn_fwd2.hip, bevbert_attn_f16_fwd), shared
by tests/test_gpu_attn_f16.py (the kernel) and tests/test_clip_vit_f16_host.py (the emulation, on the same tensors).  Nothing
here touches the library.

The bound is the one the bf16 MFMA kernels are held to (tests/attn_cases.py) with the unit changed from 2^-8 to 2^-11:

    |o - o64| <= C16 * 2^-11 * sum_j p_ij |v_jd|  +  half an fp16 ulp of o64

o64 = the fp64 softmax-attention of the fp16-rounded inputs.  The first term covers the fp16 rounding of P (2^-11 relative per
probability: ONE unit, the rest is head room for the fp32 score / exponential / accumulation errors, as for bf16, whose
kernels needed 0.90 of their 4); the second the single rounding of the result.  No flush term: the inputs keep every
probability at or above 2^-12 of its row maximum (asserted by both tests), fp16 is normal down to 2^-14, and the kernel's
lagging maximum only scales P up."""
import math

import torch

from tests.attn_cases import D, SCALE, reference      # noqa: F401  (re-exported: the fp64 reference of the bf16 tests)

C16 = 4.0
U11 = 2.0 ** -11
P_FLOOR = 2.0 ** -12          # every probability / its row maximum stays at or above this
SEED = 23
# Lq = Lk lengths: below, at and past the 16-key MFMA tile, the 64-key LDS tile (1, 2, 3 tiles: double buffer and prefetch both
# turn over at 129), the 32-query wave and the 128-query workgroup (more than one block at 129); 197 is the encoder's own, 577
# ViT-B/16 at 384 pixels (ten tiles).  Cross shapes: one query, one key, and Lq != Lk with a partial tile on both axes.
SELF_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 197, 257, 577)
CROSS_SHAPES = ((1, 197), (197, 1), (65, 130))
B, NH = 2, 2
NH_WIDE = 12                  # one case with the encoder's head count


def cases():
    """(Lq, Lk, nh, packed): every shape once with packed strided views (self shapes: the q | k | v column slices of one
    (B, L, 3 nh 64) tensor, what ops.attention_self passes; cross shapes: q and the k | v slices of one (B, Lk, 2 nh 64)
    tensor) and once with separate contiguous tensors; the encoder's head count once, packed."""
    shapes = [(L, L) for L in SELF_LENGTHS] + list(CROSS_SHAPES)
    return [(Lq, Lk, NH, packed) for Lq, Lk in shapes for packed in (True, False)] + [(197, 197, NH_WIDE, True)]


def case_id(c):
    return f"{c[0]}x{c[1]}-nh{c[2]}-{'packed' if c[3] else 'separate'}"


def make_inputs(Lq, Lk, nh, seed=SEED):
    """fp16 (q, k, v): q and k are 0.85 randn -- scores scale * q.k with a standard deviation of 0.72, so that over the 1.3
    million scores of the largest case a row's spread stays below ln(2^12) = 8.3 and no probability falls below P_FLOOR of its
    row maximum, while a row's largest probability is still several times its mean; v randn."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * Lq + Lk + 7 * nh)
    H = nh * D
    q = (0.85 * torch.randn(B, Lq, H, generator=g)).to(torch.float16)
    k = (0.85 * torch.randn(B, Lk, H, generator=g)).to(torch.float16)
    v = torch.randn(B, Lk, H, generator=g).to(torch.float16)
    return q, k, v


def _heads(t):
    b, L, H = t.shape
    return t.reshape(b, L, H // D, D).permute(0, 2, 1, 3)


def _rows(t):
    b, nh, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, L, nh * D)


def reference64(q, k, v):
    """(o64, b_o, smallest probability / row maximum) of the fp16-rounded inputs, in fp64."""
    ref = reference(q, k, v, torch.zeros_like(q), SCALE)
    S = SCALE * (_heads(q.double()) @ _heads(k.double()).transpose(-1, -2))
    floor = float(torch.exp(S.amin(-1) - S.amax(-1)).min())
    return ref["o"], ref["b_o"], floor


def half_ulp16(x):
    """Half an fp16 ulp of |x| (fp64 tensor): 2^(e - 11) with e = floor(log2 |x|) >= -14, i.e. 2^-25 below 2^-14."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 11)


def bound(o64, b_o):
    return C16 * U11 * b_o + half_ulp16(o64)


def units(got, o64, b_o):
    """Worst |got - o64| in units of 2^-11 b_o with the output-rounding term taken off first: what C16 would have to be."""
    err = ((got.double() - o64).abs() - half_ulp16(o64)).clamp_min(0.0)
    return float(torch.where(err == 0, torch.zeros_like(err), err / (U11 * b_o).clamp_min(1e-300)).max())


def r16(t):
    """fp64 -> nearest-even fp16 -> fp64 (overflow to inf as IEEE fp16 does)."""
    return t.to(torch.float16).double()


def emulate(q, k, v, drop=None, dup=None, swap_v=None):
    """The kernel's arithmetic with every fp32 step taken as exact (fp64): S = scale q k^T, p = exp(S - max), l = sum of the
    UNROUNDED p, o = fp16((fp16(p) @ v) / l).  One slip at key j: ``drop`` leaves key j out; ``dup`` reads key j in place of
    key j + 1 (a tile that starts one row early); ``swap_v`` pairs the probabilities of keys j and j + 1 with each other's v
    rows (a misplaced fragment)."""
    Q, K, V = (_heads(t.double()) for t in (q, k, v))
    if dup is not None:
        K, V = K.clone(), V.clone()
        K[:, :, dup + 1], V[:, :, dup + 1] = K[:, :, dup], V[:, :, dup]
    if swap_v is not None:
        perm = torch.arange(V.shape[2])
        perm[swap_v], perm[swap_v + 1] = swap_v + 1, swap_v
        V = V[:, :, perm]
    S = SCALE * (Q @ K.transpose(-1, -2))
    if drop is not None:
        S[..., drop] = -math.inf
    p = torch.exp(S - S.amax(-1, keepdim=True))
    return _rows(r16((r16(p) @ V) / p.sum(-1, keepdim=True))).to(torch.float16)


def boundary_keys(Lk):
    """Keys at which a tile of 16 or 64 keys ends or begins, and the last two: every j of them with a key j + 1."""
    return sorted({j for j in (0, 15, 16, 31, 32, 63, 64, 127, 128, Lk - 2, Lk - 1) if 0 <= j and j + 1 < Lk})
