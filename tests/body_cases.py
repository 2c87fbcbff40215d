"""Inputs and fp64 references of tests/test_gpu_body_kernels.py, on the CPU: the GPU test runs the kernels on exactly these
tensors and tests/test_body_refs_host.py pins the references to the plain torch compositions and re-establishes the gates
that rest on an fp32 restatement.  Nothing here touches the library."""
import math

import numpy as np
import torch

U24, U22, U8 = 2.0 ** -24, 2.0 ** -22, 2.0 ** -8
DTYPES = [torch.float32, torch.bfloat16]
DT_ID = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.float64: "f64"}.get

# ----------------------------------------------------------------------------- bias + GELU / ReLU
GELU_K = 4.0                  # the gates' K, in units of 2^-22 max(1, |x + bias|); the host test holds both fp32 forms to K / 2
GELU_SHAPES = [(1, 4), (7, 36), (11, 40), (8, 1024), (17, 1028), (333, 3072), (8191, 8), (8192, 8), (16400, 8), (32771, 8)]
RELU_SHAPES = [(11, 40), (16400, 8)]


def gelu_case(rows, C, dtype, seed=0):
    """(x (rows, C) in ``dtype``, bias (C) fp32, dy (rows, C) in ``dtype``).  By (r + c) % 4 an element's x + bias is
    2 randn, a ramp over [-14, 14] along the rows of its column, the ramp along the columns of its row, or the ramp over the
    whole tensor; row 0 starts with x + bias = 0.0, -0.0, 40, -40 (bias 0.0, -0.0, 0.5, -0.5 there) and the last row ends
    with 40, -40, 0, 0 up to the rounding of x; dy ~ randn with every seventh element an exact zero."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + C)
    bias = torch.randn(C, generator=g)
    bias[:4] = torch.tensor([0.0, -0.0, 0.5, -0.5])
    r = torch.arange(rows, dtype=torch.float64)[:, None].expand(rows, C)
    c = torch.arange(C, dtype=torch.float64)[None].expand(rows, C)
    ramp = lambda t, n: -14.0 + 28.0 * t / max(n - 1, 1)
    kind = ((r + c) % 4).long()
    target = 2.0 * torch.randn(rows, C, generator=g).double()
    target = torch.where(kind == 1, ramp(r, rows) if rows > 1 else ramp(c, C), target)
    target = torch.where(kind == 2, ramp(c, C), target)
    target = torch.where(kind == 3, ramp(r * C + c, rows * C), target)
    target[-1, -4:] = torch.tensor([40.0, -40.0, 0.0, 0.0], dtype=torch.float64)
    x = (target - bias.double()).float()
    x[0, :4] = torch.tensor([0.0, -0.0, 39.5, -39.5])
    dy = torch.randn(rows, C, generator=g)
    dy.view(-1)[::7] = 0.0
    return x.to(dtype), bias, dy.to(dtype)


def gelu_ref(x, bias, dy):
    """fp64 on the values the kernel gets: (a = |x + bias|, y, gelu'(x + bias), dx, dbias); Phi through erfc, which keeps
    its relative accuracy on the negative tail."""
    u = x.double() + bias.double()
    phi = 0.5 * torch.special.erfc(-u / math.sqrt(2.0))
    grad = phi + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    dx = dy.double() * grad
    return u.abs(), u * phi, grad, dx, dx.sum(0)


def gelu_gates(a, y, dx, dy, bf16):
    """(gate of y, gate of dx, gate of dbias), elementwise, K = GELU_K."""
    unit = GELU_K * U22 * a.clamp_min(1.0)
    gy = unit + (U8 * y.abs() if bf16 else 0.0)
    gdx32 = unit * dy.double().abs() + U24 * dx.abs()
    gdx = gdx32 + (U8 * dx.abs() if bf16 else 0.0)
    rows = y.shape[0]
    return gy, gdx, gdx32.sum(0) + (rows + 4) * U24 * dx.abs().sum(0)


def gelu_fast_f32(u):
    """The bf16 kernels' Abramowitz-Stegun 7.1.26 form (gelu_cdf_fast2 in csrc/common.h) restated in numpy fp32 with an exact
    division and numpy's exp2: (gelu(u), gelu'(u)) for an fp32 array u."""
    f = np.float32
    u = np.asarray(u, dtype=f)
    z = np.abs(u) * f(0.70710678118654752440)
    t = f(1.0) / (z * f(0.3275911) + f(1.0))
    E = np.exp2(u * u * f(-0.72134752044448170368)).astype(f)
    poly = t * f(1.061405429) + f(-1.453152027)
    poly = poly * t + f(1.421413741)
    poly = poly * t + f(-0.284496736)
    poly = poly * t + f(0.254829592)
    he = poly * t * E * f(0.5)
    cdf = np.where(u >= 0, f(1.0) - he, he).astype(f)
    return u * cdf, u * f(0.39894228040143267794) * E + cdf


def relu_ref(x, bias, dy):
    """(y, dx) exact in the tensors' dtype -- one fp32 add, a selection, one rounding of y -- and dbias in fp64."""
    u = x.float() + bias.float()
    dx = torch.where(u > 0, dy.float(), torch.zeros(()))
    return torch.relu(u).to(x.dtype), dx.to(x.dtype), dx.double().sum(0)


# ----------------------------------------------------------------------------- row gather / scatter
ROW_WIDTHS = [4, 40, 252, 768, 1024]
TABLE_ROWS = 37                              # rows of the scatter's destination; ids 30 .. 35 never occur


def scatter_ids(kind, seed=0):
    """int64 ids in [0, TABLE_ROWS) of one scatter case.
    "one": a single row.  "r257": id 0 in rows 0 and 256, so its leader's scan passes one 256-row batch; ids 1 .. 4 between.
    "quarters": 1 000 rows, id 2 on 700 of them, row 0 among them, so all four waves of its leader find it in their
    quarters; id 36 once, in the last row.  "firstlast": 64 rows of which only the first and the last carry id 9.
    "r1100": 1 100 rows over seven ids: a leader's quarter exceeds 256 rows and its scan loops."""
    g = torch.Generator().manual_seed(50 + seed)
    if kind == "one":
        return torch.tensor([29])
    if kind == "r257":
        ids = torch.randint(1, 5, (257,), generator=g)
        ids[0] = ids[256] = 0
        return ids
    if kind == "quarters":
        ids = torch.randint(3, 30, (1000,), generator=g)
        hit = torch.randperm(998, generator=g)[:699] + 1
        ids[hit] = 2
        ids[0], ids[-1] = 2, 36
        return ids
    if kind == "firstlast":
        ids = (torch.randperm(29, generator=g).repeat(3)[:64] + 0).clone()
        ids[ids == 9] = 10
        ids[0] = ids[-1] = 9
        return ids
    assert kind == "r1100"
    return torch.randint(10, 17, (1100,), generator=g)


SCATTER_KINDS = ["one", "r257", "quarters", "firstlast", "r1100"]


def scatter_ref(ids, d, base=None):
    """fp64 (want, gate without the bf16 term, touched rows) of out[id] = (base[id] +) sum of d's rows with that id.  Gate per
    element: (k + 2) 2^-24 sum |terms| over the k terms of that id, the row of ``base`` counting as one of them."""
    H = d.shape[1]
    want = torch.zeros(TABLE_ROWS, H, dtype=torch.float64)
    mag = torch.zeros(TABLE_ROWS, H, dtype=torch.float64)
    k = torch.zeros(TABLE_ROWS, dtype=torch.float64)
    want.index_add_(0, ids, d.double())
    mag.index_add_(0, ids, d.double().abs())
    k.index_add_(0, ids, torch.ones(len(ids), dtype=torch.float64))
    touched = k > 0
    if base is not None:
        want = torch.where(touched[:, None], want + base.double(), base.double())
        mag = mag + base.double().abs()
        k = k + 1
    return want, (k[:, None] + 2) * U24 * mag, touched


# ----------------------------------------------------------------------------- segment gather
SEG_WIDTHS = [4, 40, 768, 1024]
SEG_N_SRC = 9
# output segments as lists of source rows: empty, 1, 5 (source 1 twice), 130 (sources 0 .. 6 again and again), 2 (source 7
# twice), empty; source 8 is read by nobody
SEGMENTS_A = [[], [2], [0, 1, 1, 4, 7], [i % 7 for i in range(130)], [7, 7], []]
# a second aggregation of the same shape with fewer entries; sources 4 and 7 are read by nobody
SEGMENTS_B = [[5], [], [0, 2, 2], [6, 6, 6, 6, 1], [], [8, 3]]


def segment_lists(segments, seed=0):
    """(rowptr, idx, w) as plain lists for SegmentCSR; weights ~ randn, as fp32 values."""
    g = torch.Generator().manual_seed(80 + seed)
    rowptr, idx = [0], []
    for s in segments:
        idx += s
        rowptr.append(len(idx))
    w = torch.randn(len(idx), generator=g)
    w[::5] = w[::5].abs() + 0.5
    return rowptr, idx, w.tolist()


def segment_ref(rowptr, idx, w, src, n_src, dy):
    """fp64: (out, gate of out, dsrc, gate of dsrc), gates (n_e + 2) 2^-24 sum_e |w_e v_e| without the bf16 term."""
    n_out, H = len(rowptr) - 1, src.shape[1]
    wd = torch.tensor(w, dtype=torch.float32).double()
    out, mo, no = (torch.zeros(n_out, H, dtype=torch.float64) for _ in range(3))
    ds, ms, ns = (torch.zeros(n_src, H, dtype=torch.float64) for _ in range(3))
    for r in range(n_out):
        for e in range(rowptr[r], rowptr[r + 1]):
            t = wd[e] * src[idx[e]].double()
            out[r] += t; mo[r] += t.abs(); no[r] += 1
            t = wd[e] * dy[r].double()
            ds[idx[e]] += t; ms[idx[e]] += t.abs(); ns[idx[e]] += 1
    return out, (no + 2) * U24 * mo, ds, (ns + 2) * U24 * ms


# ----------------------------------------------------------------------------- BertEmbeddings
EMBED_SHAPES = [(11, 256, 1, 1), (500, 768, 3, 17), (40, 1024, 2, 64)]
EMBED_EPS = 1e-12


def embed_case(V, H, B, L, seed=0):
    """fp32 masters (word (V, H), pos (L + 3, H), typ (2, H), gamma, beta), ids (B, L) with id 0 in several rows and id 7 (3 where
    V is small) repeated, dy (B, L, H) fp32, and the type row the case adds (1 for the 17-token shape)."""
    g = torch.Generator().manual_seed(300 + seed + V)
    word, pos, typ = torch.randn(V, H, generator=g), torch.randn(L + 3, H, generator=g), torch.randn(2, H, generator=g)
    gamma, beta = 0.5 + torch.rand(H, generator=g), 0.3 * torch.randn(H, generator=g)
    ids = torch.randint(0, V, (B, L), generator=g)
    flat = ids.view(-1)
    n = flat.numel()
    if n == 1:
        flat[0] = 0
    else:
        flat[torch.randperm(n, generator=g)[:max(2, n // 6)]] = 0
        rep = torch.randperm(n, generator=g)[:max(2, n // 8)]
        flat[rep] = 7 if V > 7 else 3
        flat[0], flat[-1] = 0, 0                   # the padding id in the first and in the last row
    dy = torch.randn(B, L, H, generator=g)
    return {"word": word, "pos": pos, "typ": typ, "gamma": gamma, "beta": beta, "ids": ids, "dy": dy,
            "type_index": 1 if L == 17 else 0}


def embed_ref(case, dtype, padding_idx):
    """fp64 reference of BertEmbeddings in compute dtype ``dtype`` (tables and dy rounded to it first): y and the five
    gradients.  z = (word_c[ids] + pos_c[row % L]) + typ_c[type_index]; mean and rstd from the unrounded sum; xhat read from z
    as the kernel saves it (the fp32 sum rounded to ``dtype``; fp64: the sum itself); dz the LayerNorm adjoint.  Also
    |dz| routed like dz (the bf16 gates' 2^-8 sums)."""
    ids, ti = case["ids"], case["type_index"]
    B, L = ids.shape
    wc, pc, tc = (case[k].to(dtype) for k in ("word", "pos", "typ"))
    gamma, beta, dy = case["gamma"].double(), case["beta"].double(), case["dy"].to(dtype).double()
    V, H = wc.shape
    if dtype == torch.float64:
        z = (wc[ids] + pc[:L][None]) + tc[ti]
        z_saved = z
    else:
        z32 = (wc[ids].float() + pc[:L][None].float()) + tc[ti].float()     # the kernel's own two fp32 adds, exactly
        z = (wc[ids].double() + pc[:L][None].double()) + tc[ti].double()
        z_saved = z32.to(dtype).double()
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + EMBED_EPS)
    y = (z - mean) * rstd * gamma + beta
    xh = (z_saved - mean) * rstd
    gd = gamma * dy
    dz = rstd * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    flat, keep = ids.reshape(-1), ids.reshape(-1) != (-1 if padding_idx is None else padding_idx)

    def route(t):
        dw = torch.zeros(V, H, dtype=torch.float64).index_add_(0, flat[keep], t.reshape(-1, H)[keep])
        dp = torch.zeros(pc.shape[0], H, dtype=torch.float64)
        dp[:L] = t.sum(0)
        dt = torch.zeros(2, H, dtype=torch.float64)
        dt[ti] = t.sum((0, 1))
        return dw, dp, dt
    dw, dp, dt = route(dz)
    aw, ap, at = route(dz.abs())
    return {"y": y, "word": dw, "pos": dp, "typ": dt, "gamma": (dy * xh).sum((0, 1)), "beta": dy.sum((0, 1)),
            "abs": {"word": aw, "pos": ap, "typ": at}}


def embed_torch(case, dtype, padding_idx, ref_dtype):
    """The plain torch composition in ``ref_dtype`` on the tables rounded to ``dtype``: F.embedding(padding_idx) + pos + type,
    F.layer_norm, autograd."""
    import torch.nn.functional as F
    ids, ti = case["ids"], case["type_index"]
    L = ids.shape[1]
    ps = {k: case[k].to(dtype).to(ref_dtype).requires_grad_(True) for k in ("word", "pos", "typ")}
    ps.update({k: case[k].to(ref_dtype).requires_grad_(True) for k in ("gamma", "beta")})
    z = (F.embedding(ids, ps["word"], padding_idx=padding_idx) + ps["pos"][:L][None]) + ps["typ"][ti]
    y = F.layer_norm(z, (z.shape[-1],), ps["gamma"], ps["beta"], EMBED_EPS)
    y.backward(case["dy"].to(dtype).to(ref_dtype))
    out = {k: p.grad for k, p in ps.items()}
    out["y"] = y.detach()
    return out


# ----------------------------------------------------------------------------- graph bias
GRAPH_SHAPES = [(1, 1, 1, 1), (3, 5, 12, 20), (2, 3, 12, 63), (4, 8, 12, 80)]
GRAPH_DW0, GRAPH_DB0 = 0.75, -1.25


def graph_case(layers, B, nh, G):
    """dbias (layers, B, nh, G, G) ~ randn; dists (B, G, G) >= 0 with another scale and pattern per sample."""
    g = torch.Generator().manual_seed(layers * 1000 + G)
    dbias = torch.randn(layers, B, nh, G, G, generator=g)
    dists = torch.rand(B, G, G, generator=g) * (1.0 + torch.arange(B, dtype=torch.float32))[:, None, None]
    dists[:, torch.arange(G), torch.arange(G)] = 0.0
    return dbias, dists


def graph_blocks(n):
    return min(512, (n + 4095) // 4096)


def graph_ref(dbias, dists):
    """fp64 (dw, db, gate of dw, gate of db); gates (n / nb / 256 + nb + 16) 2^-24 sum |terms|, the start value a term."""
    terms = dbias.double() * dists.double()[None, :, None]
    n = dbias.numel()
    nb = graph_blocks(n)
    fac = (n / nb / 256 + nb + 16) * U24
    return (GRAPH_DW0 + float(terms.sum()), GRAPH_DB0 + float(dbias.double().sum()),
            fac * (abs(GRAPH_DW0) + float(terms.abs().sum())), fac * (abs(GRAPH_DB0) + float(dbias.double().abs().sum())))


# ----------------------------------------------------------------------------- dropout_add and cast_f32
BIG_N = 8388608 + 4 * 37          # both kernels cap their grid at 8 192 blocks of 256 threads x 4 elements: the first 37
CAST_BIG_N = 8388608 + 4          # (or the first one) threads loop once more
DROP_P = 0.1


def dropout_want(x, res, keep, p=DROP_P):
    """fp64 (want, gate without the bf16 term, the gate as first stated) of y = res + keep x / (1 - p), p as the fp32 value
    the kernel gets.  A dropped element's gate is 0: the residual itself, or 0.  A kept one was first given
    2 x 2^-24 (|x| / (1 - p) + |res|); but x / (1 - p) passes four fp32 roundings on its way into y -- 1 - p, the reciprocal
    (together 0.77 x 2^-24 at p = 0.1), the product, the sum -- and the residual one, so plain fp32 arithmetic exceeds that
    (tests/test_body_refs_host.py: 1.34 times on randn).  The gate is 2^-24 (4 |x| / (1 - p) + 2 |res|)."""
    p32 = float(np.float32(p))
    xk = x.double() / (1.0 - p32)
    r = torch.zeros_like(xk) if res is None else res.double()
    want = torch.where(keep, xk + r, r)
    zero = torch.zeros_like(xk)
    return (want, torch.where(keep, U24 * (4.0 * xk.abs() + 2.0 * r.abs()), zero),
            torch.where(keep, 2.0 * U24 * (xk.abs() + r.abs()), zero))


def _bits(values):
    return torch.tensor(values, dtype=torch.int64).to(torch.int32).view(torch.float32)


def cast_values(n, dtype, seed=0):
    """n fp32 values for a cast to ``dtype`` (bf16 or fp16): the special values below at the head and again at the tail,
    random bit patterns (every exponent, NaNs and infinities among them) and randn in between."""
    f = lambda v: float(np.float32(v))
    if dtype == torch.bfloat16:
        sp = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)]              # ties, even and odd below
        sp += [f(1 + 2.0 ** -8 + 2.0 ** -23), f(1 + 2.0 ** -8 - 2.0 ** -23)]                             # one ulp off a tie
        top = [0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF]      # max, below the tie, the tie (-> inf), above, fp32 max
        tiny = [0x00010000, 0x00008000, 0x00008001, 0x00018000, 0x00000001, 0x00800000, 0x007FFFFF]     # bf16 subnormals and below
    else:
        sp = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11)]
        sp += [f(1 + 2.0 ** -11 + 2.0 ** -23), f(1 + 2.0 ** -11 - 2.0 ** -23)]
        sp += [65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e30, -65519.996, -65520.0]           # fp16 max, the tie to inf
        sp += [2.0 ** -24, 2.0 ** -25, f(2.0 ** -25 * (1 + 2.0 ** -23)), 3 * 2.0 ** -25, 2.0 ** -14, f(2.0 ** -14 * (1 - 2.0 ** -12)),
               1e-10, -2.0 ** -25, -3 * 2.0 ** -25, -1e-10, 1023 * 2.0 ** -24 + 2.0 ** -25]            # subnormals, underflow
        top, tiny = [], [0x00000001, 0x007FFFFF]
    sp += [0.0, -0.0, float("inf"), -float("inf"), float("nan")]
    bits = top + tiny + [b | 0x80000000 for b in top + tiny] + [0x7FC00001, 0xFFC00000, 0x7F800001]  # (three more NaNs)
    special = torch.cat([torch.tensor(sp, dtype=torch.float32), _bits(bits)])
    special = torch.cat([special, torch.zeros((-len(special)) % 4)])
    if n <= 4:
        return special[:n].clone()
    g = torch.Generator().manual_seed(600 + seed)
    out = torch.randn(n, generator=g)
    half = n // 2
    out[:half] = torch.randint(-2 ** 31, 2 ** 31, (half,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    k = len(special)
    out[:k] = special
    out[-k:] = special.flip(0)
    return out
