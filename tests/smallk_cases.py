"""Inputs, fp64 references and gates of tests/test_gpu_smallk.py, on the CPU: the small-K projection LayerNorm
(csrc/smallk.hip: y = (LayerNorm(feat W^T + b) + post1) + table[idx], its backward and its finalize) and the sliced
small-table gradient (embedding_grad_sliced_kernel in csrc/gather.hip).  The GPU test runs the kernels on exactly these
tensors; tests/test_smallk_refs_host.py pins the references to the plain torch compositions and holds torch's fp32
composition and a numpy fp32 restatement of the kernels' own order to half of every gate.  Nothing here touches the library.

Gates are first-order rounding bounds written from fp64 quantities only, u = 2^-24, A = |feat| |W|^T + |b| per element:

    e_z    = (K + 2) u A
    e_xhat = rstd (e_z + mean_H e_z) + 4 u |xhat|            (the subtraction, a two-ulp rsqrtf, the product)
    y      : |gamma| e_xhat + u (|xhat gamma| + |ln| + |ln + post1| + |y|), ln = xhat gamma + beta  (+ 2^-8 |y| for a bf16 y;
             first stated with u (|y| + |post1| + |table row|), which plain fp32 arithmetic comes too near: see ref())
    dz     : rstd (4 u (|g| + mean|g| + |xhat| mean|g xhat|) + |mean(g xhat)| e_xhat + |xhat| mean(|g| e_xhat))
             + |dz| mean(e_xhat |xhat|),  g = gamma dy
    dW, db, dgamma : the per-row gate carried through the sum + D u sum |terms|, the sink's start value a term;
    dbeta  : D u sum |terms|;  D = ceil(rows / nb) + nb / 4 + 6, nb = min(256, ceil(rows / 8)), the depth of the kernels'
             fixed summation tree (sum_depth below restates sk_bwd_blocks, as graph_blocks restates its kernel in body_cases.py)
    d table and the sliced partials : (k + 2) u sum |terms| over the k rows of an id (plus the start value); exact for k = 0.
"""
import functools
import math

import numpy as np
import torch

U24, U8 = 2.0 ** -24, 2.0 ** -8
DTYPES = [torch.float32, torch.bfloat16]
DT_ID = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64"}.get
EPS = 1e-12
TABLE_ROWS = 4                      # ids 0 .. 2 occur, id 3 never does
SINKS = ("W", "b", "gamma", "beta", "table")

# (H, K): K = 1; the k4 * 4 < K groups of phase B (4, 5, 8, 9); K = 16; the largest K the backward's LDS admits at 768 and 1024
WIDTH_K = [(256, 1), (256, 4), (256, 5), (256, 16), (512, 8), (512, 9), (512, 16), (768, 7), (768, 10), (768, 13), (1024, 7)]
WIDTH_K_ROWS = 9
# the backward's 8-row tile (1, 7, 8, 9), every nblocks of the finalize's three loops (1, 2, 3, 4, 5, 8, 9, 12, 13 blocks),
# exactly 256 tiles, and 257 tiles: block 0 gets a second tile that holds one row
BWD_ROWS = [1, 7, 8, 9] + [8 * n - 3 for n in (3, 4, 5, 8, 9, 12, 13)] + [2048, 2049]
BWD_H, BWD_K = 256, 3
CAP_ROWS, CAP_H, CAP_K = 4101, 768, 7            # past the forward's 1 024 blocks x 4 rows; block 0 of the backward owns three tiles
OFFSET_SHAPES = [(1024, 7), (768, 10)]
OFFSET_ROWS = 41
SPARSE_ROWS = 2049
SPARSE_DY_ROWS = (0, 7, 8, 2047, 2048)


def bwd_blocks(rows):
    return min(256, max(1, (rows + 7) // 8))


def sum_depth(rows):
    nb = bwd_blocks(rows)
    return math.ceil(rows / nb) + nb / 4 + 6


def max_k(H):
    """The largest K <= 16 with (K + 8) H 4 + 512 <= 65536: the backward's LDS need ([K][H] + [8][H] + [8][16] floats)."""
    return min(16, (65536 - 512) // (4 * H) - 8)


@functools.lru_cache(maxsize=4)
def case(rows, K, H, dtype, kind="plain", seed=0):
    """One case as a dict of CPU tensors.  fp32 masters feat (rows, K), W (H, K) ~ 0.3 randn, b, gamma in [0.5, 1.5], beta;
    post1, dy (rows, H) and table (TABLE_ROWS, H) hold values of ``dtype`` (table as the fp32 master of exactly those
    values); idx int64.  By row: 0 and the last carry table id 0, id 3 is never used; rows 1, 4, 7, .. have all-zero
    features and one shared post1 row; row 2 (the last row of a shorter case) is one-hot; every seventh element of dy is an
    exact zero.  ``start``: the non-zero fp32 value each sink holds before the backward.
    kind "offset": feat[:, 0] = 1000 on the other rows and W[:, 0] = 1 + 0.01 randn, |mean z| ~ 1e3 its spread;
    kind "sparse": dy is non-zero only in SPARSE_DY_ROWS; kind "nulls": b = 0, post1 = 0 and a zero table, what the
    kernels compute when those pointers are null."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * rows + 7 * K + H + {"plain": 0, "offset": 1, "sparse": 2, "nulls": 3}[kind])
    rn = lambda *s: torch.randn(*s, generator=g)
    feat, W, b = rn(rows, K), 0.3 * rn(H, K), 0.3 * rn(H)
    gamma, beta = 0.5 + torch.rand(H, generator=g), 0.3 * rn(H)
    post1, dy, table = rn(rows, H).to(dtype), rn(rows, H).to(dtype), rn(TABLE_ROWS, H).to(dtype)
    idx = torch.randint(0, TABLE_ROWS - 1, (rows,), generator=g)
    idx[0] = idx[-1] = 0
    r = torch.arange(rows)
    zero_rows, hot = r % 3 == 1, min(2, rows - 1)
    if kind == "offset":
        feat[:, 0] = 1000.0
        W[:, 0] = 1.0 + 0.01 * rn(H)
    feat[zero_rows] = 0.0
    feat[hot] = 0.0
    feat[hot, min(K - 1, 2)] = 1.0
    if bool(zero_rows.any()):
        post1[zero_rows] = post1[1].clone()
    dy.view(-1)[::7] = 0.0
    if kind == "sparse":
        keep = torch.zeros(rows, dtype=torch.bool)
        keep[list(SPARSE_DY_ROWS)] = True
        dy[~keep] = 0.0
    if kind == "nulls":
        b, post1, table = torch.zeros_like(b), torch.zeros_like(post1), torch.zeros_like(table)
    start = {"W": rn(H, K), "b": rn(H), "gamma": rn(H), "beta": rn(H), "table": rn(TABLE_ROWS, H)}
    return {"rows": rows, "K": K, "H": H, "dtype": dtype, "kind": kind, "feat": feat, "W": W, "b": b, "gamma": gamma,
            "beta": beta, "post1": post1, "dy": dy, "table": table.float(), "idx": idx, "zero_rows": zero_rows, "hot": hot,
            "start": start, "tag": f"{DT_ID(dtype)} {kind} {rows}x{K}->{H}"}


def all_cases():
    """(rows, K, H, dtype, kind) of every case of the GPU test, in its order."""
    out = [(WIDTH_K_ROWS, K, H, dt, "plain") for H, K in WIDTH_K for dt in DTYPES]
    out += [(rows, BWD_K, BWD_H, torch.float32, "plain") for rows in BWD_ROWS]
    out += [(CAP_ROWS, CAP_K, CAP_H, dt, "plain") for dt in DTYPES]
    out += [(OFFSET_ROWS, K, H, dt, "offset") for H, K in OFFSET_SHAPES for dt in DTYPES]
    out += [(SPARSE_ROWS, BWD_K, BWD_H, torch.float32, "sparse")]
    out += [(WIDTH_K_ROWS, 7, 768, dt, "nulls") for dt in DTYPES]
    return out


def scatter_ref(ids, d, n, base=None):
    """fp64 (want, gate) of out[t] = (base[t] +) sum of d's rows with id t, t < n; gate (k + 2) u sum |terms| over the k rows
    of the id, the row of ``base`` one more term; a row nobody names keeps ``base`` (or 0) exactly: its gate is 0."""
    H = d.shape[1]
    want, mag = torch.zeros(n, H, dtype=torch.float64), torch.zeros(n, H, dtype=torch.float64)
    k = torch.zeros(n, dtype=torch.float64)
    want.index_add_(0, ids, d.double())
    mag.index_add_(0, ids, d.double().abs())
    k.index_add_(0, ids, torch.ones(len(ids), dtype=torch.float64))
    hit = k > 0
    if base is not None:
        want, mag, k = want + base.double(), mag + base.double().abs(), k + 1
    return want, torch.where(hit[:, None], (k[:, None] + 2) * U24 * mag, torch.zeros_like(mag))


@functools.lru_cache(maxsize=2)
def ref(rows, K, H, dtype, kind="plain", seed=0):
    """fp64 on the values the kernel gets: {"y", "ln", "z", "xhat", "mean", "rstd", "dz", "dW", "db", "dgamma", "dbeta",
    "dtable"} and "gate": the same keys' elementwise bounds (module docstring).  The parameter gradients include the
    sinks' start values."""
    c = case(rows, K, H, dtype, kind, seed)
    f, W, b, gam, bet = (c[k].double() for k in ("feat", "W", "b", "gamma", "beta"))
    post1, dy, table, idx, st = c["post1"].double(), c["dy"].double(), c["table"].double(), c["idx"], c["start"]
    z = f @ W.t() + b
    A = f.abs() @ W.abs().t() + b.abs()
    mean = z.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(1, keepdim=True) + EPS)
    xhat = (z - mean) * rstd
    ln = xhat * gam + bet
    y = (ln + post1) + table[idx]
    g = gam * dy
    m1, m2 = g.mean(1, keepdim=True), (g * xhat).mean(1, keepdim=True)
    dz = rstd * (g - m1 - xhat * m2)
    mH = lambda t: t.mean(1, keepdim=True)
    e_z = (K + 2) * U24 * A
    e_xhat = rstd * (e_z + mH(e_z)) + 4 * U24 * xhat.abs()
    # y as first stated: |gamma| e_xhat + u (|y| + |post1| + |table row|).  That counts three roundings, but four touch y
    # after xhat: the product xhat gamma, the sum with beta, with post1, with the table row; where beta cancels
    # xhat gamma, or post1 the LayerNorm part, the first two are not covered by |y| + |post1| + |table row| and plain fp32
    # arithmetic reaches 0.53 of the stated form (tests/test_smallk_refs_host.py, 2 048 x 3 -> 256).  The gate names each
    # rounding by the magnitude it rounds.
    g_y_stated = gam.abs() * e_xhat + U24 * (y.abs() + post1.abs() + table[idx].abs())
    g_y32 = gam.abs() * e_xhat + U24 * ((xhat * gam).abs() + ln.abs() + (ln + post1).abs() + y.abs())
    g_y = g_y32 + U8 * y.abs() if dtype == torch.bfloat16 else g_y32
    g_dz = (rstd * (4 * U24 * (g.abs() + mH(g.abs()) + xhat.abs() * mH((g * xhat).abs())) + m2.abs() * e_xhat
                    + xhat.abs() * mH(g.abs() * e_xhat)) + dz.abs() * mH(e_xhat * xhat.abs()))
    Du = sum_depth(rows) * U24
    s = {k: v.double() for k, v in st.items()}
    out = {"y": y, "ln": ln, "z": z, "xhat": xhat, "mean": mean, "rstd": rstd, "dz": dz,
           "dW": s["W"] + dz.t() @ f, "db": s["b"] + dz.sum(0), "dgamma": s["gamma"] + (dy * xhat).sum(0),
           "dbeta": s["beta"] + dy.sum(0)}
    out["dtable"], g_tab = scatter_ref(idx, dy, TABLE_ROWS, s["table"])
    out["gate"] = {"y": g_y, "y32": g_y32, "y_stated": g_y_stated, "dz": g_dz, "e_xhat": e_xhat,
                   "dW": g_dz.t() @ f.abs() + Du * (s["W"].abs() + dz.abs().t() @ f.abs()),
                   "db": g_dz.sum(0) + Du * (s["b"].abs() + dz.abs().sum(0)),
                   "dgamma": (dy.abs() * e_xhat).sum(0) + Du * (s["gamma"].abs() + (dy * xhat).abs().sum(0)),
                   "dbeta": Du * (s["beta"].abs() + dy.abs().sum(0)),
                   "dtable": g_tab}
    return out


def torch_composition(c, ref_dtype):
    """The plain torch composition in ``ref_dtype`` on the case's values: F.linear, F.layer_norm, the two sums, autograd;
    the parameter gradients with the sinks' start values added (in ``ref_dtype``).  Also dz."""
    import torch.nn.functional as F
    ps = {k: c[k].to(ref_dtype).requires_grad_(True) for k in ("W", "b", "gamma", "beta", "table", "post1")}
    z = F.linear(c["feat"].to(ref_dtype), ps["W"], ps["b"])
    z.retain_grad()
    y = (F.layer_norm(z, (c["H"],), ps["gamma"], ps["beta"], EPS) + ps["post1"]) + F.embedding(c["idx"], ps["table"])
    y.backward(c["dy"].to(ref_dtype))
    st = c["start"]
    return {"y": y.detach(), "dz": z.grad, "dpost1": ps["post1"].grad, "dW": st["W"].to(ref_dtype) + ps["W"].grad,
            "db": st["b"].to(ref_dtype) + ps["b"].grad, "dgamma": st["gamma"].to(ref_dtype) + ps["gamma"].grad,
            "dbeta": st["beta"].to(ref_dtype) + ps["beta"].grad, "dtable": st["table"].to(ref_dtype) + ps["table"].grad}


# ----------------------------------------------------------------------------- the kernels' own order, in numpy fp32
def _fma(a, b, c):
    """fp32 a * b + c with one rounding: the product of two fp32 values is exact in fp64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _wave_sum(t):
    """Per-lane sums of a row's float4s, (x + y) + (z + w) each, then the xor butterfly over the 64 lanes; t (rows, H)."""
    rows, H = t.shape
    t4 = t.reshape(rows, H // 256, 64, 4)
    s = np.zeros((rows, 64), dtype=np.float32)
    for i in range(H // 256):
        s = s + ((t4[:, i, :, 0] + t4[:, i, :, 1]) + (t4[:, i, :, 2] + t4[:, i, :, 3]))
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, :1]


def _fold4(w):
    return (w[0] + w[1]) + (w[2] + w[3])


@functools.lru_cache(maxsize=2)
def kernel_f32(rows, K, H, dtype, kind="plain", seed=0, one_pass=False, sums=True):
    """smallk_ln_fwd_kernel, smallk_ln_bwd_kernel and smallk_finalize_kernel restated in numpy fp32, operation by operation:
    the bias-seeded fma chain over k, the two-pass statistics of ln_fwd_kernel (``one_pass``: mean(z^2) - mean^2 instead,
    what the kernel must not do), the backward of ln_bwd_chunk_*, phase B's fma per (row, k), a workgroup's tiles in
    ascending order, the four waves' column sums folded pairwise, the finalize's two interleaved chains per wave.  The
    compiler's own fma contractions are not restated.  Returns torch fp64 tensors under the keys of ref(); "y" is the fp32
    value, "y_out" that value rounded to ``dtype``."""
    c = case(rows, K, H, dtype, kind, seed)
    f32 = np.float32
    n = lambda k: c[k].float().numpy()
    feat, W, b, gam, bet, post1, dy, table = (n(k) for k in ("feat", "W", "b", "gamma", "beta", "post1", "dy", "table"))
    idx = c["idx"].numpy()
    invH = f32(1.0 / H)
    v = np.broadcast_to(b, (rows, H)).astype(f32)
    for k in range(K):
        v = _fma(feat[:, k:k + 1], W[None, :, k], v)
    mean = _wave_sum(v) * invH
    if one_pass:
        var = _wave_sum(v * v) * invH - mean * mean
    else:
        d = v - mean
        var = _wave_sum(d * d) * invH
    rstd = (f32(1.0) / np.sqrt(var + f32(EPS))).astype(f32)
    xh = (v - mean) * rstd
    y = ((xh * gam + bet) + post1) + table[idx]
    y_out = torch.from_numpy(y).to(dtype).float().numpy()            # as stored
    gd = dy * gam
    s1, s2 = _wave_sum(gd) * invH, _wave_sum(gd * xh) * invH
    dz = rstd * (gd - s1 - xh * s2)
    out = {"y": y, "y_out": y_out, "dz": dz}
    if sums:
        nb = bwd_blocks(rows)
        ag, ab, ax = (np.zeros((nb, 4, H), dtype=f32) for _ in range(3))
        acc = np.zeros((nb, H, K), dtype=f32)
        for r in range(rows):
            blk, wave = (r // 8) % nb, (r % 8) // 2
            ag[blk, wave] += dy[r] * xh[r]
            ab[blk, wave] += dy[r]
            ax[blk, wave] += dz[r]
            acc[blk] = _fma(dz[r][:, None], feat[r][None, :], acc[blk])

        def finalize(part, start):                       # part (nb, ...) -> start + the fixed-order sum over the workgroups
            waves = []
            for w in range(4):
                s0, s1_ = np.zeros_like(part[0]), np.zeros_like(part[0])
                blk = w
                while blk + 4 < nb:
                    s0, s1_ = s0 + part[blk], s1_ + part[blk + 4]
                    blk += 8
                while blk < nb:
                    s0 = s0 + part[blk]
                    blk += 4
                waves.append(s0 + s1_)
            return start.float().numpy() + _fold4(waves)
        st = c["start"]
        out.update({"dW": finalize(acc, st["W"]), "dgamma": finalize(_fold4(ag.transpose(1, 0, 2)), st["gamma"]),
                    "dbeta": finalize(_fold4(ab.transpose(1, 0, 2)), st["beta"]), "db": finalize(_fold4(ax.transpose(1, 0, 2)), st["b"])})
    return {k: torch.from_numpy(np.ascontiguousarray(t)).double() for k, t in out.items()}


# ----------------------------------------------------------------------------- embedding_grad_sliced
# (H, rows_per_slice, rows, table_rows) of the direct calls: fewer than 256 threads (H = 4: one wave of which one lane works;
# H = 40); the column loop past 1 024 columns; a slice of 3 rows (the r + j < r1 tail) with a shorter last slice; a slice
# of one row; 64-row slices whose last one is short.  Table row table_rows - 1 is named by nobody where table_rows > 1.
SLICED_DIRECT = [(4, 1, 5, 2), (40, 3, 77, 5), (768, 64, 130, 5), (1028, 3, 5, 2), (1028, 64, 77, 1), (768, 3, 1, 1)]
# (table_rows, rows, H) through ops.embedding_grad_small: 43 slices x 100 ids exceed 4 096 workgroups, so the wrapper doubles
# its slice to 128 rows once; and three ids over two slices at 768
SLICED_WRAPPER = [(100, 2700, 256), (3, 77, 768)]


@functools.lru_cache(maxsize=None)
def sliced_case(H, rows, table_rows, dtype, seed=0):
    """(ids, d (rows, H) of ``dtype``, start (table_rows, H) fp32): id 0 in the first and last row, the last id unused."""
    g = torch.Generator().manual_seed(1000 * seed + 13 * rows + H + table_rows)
    ids = torch.randint(0, max(1, table_rows - 1), (rows,), generator=g)
    ids[0] = ids[-1] = 0
    d = torch.randn(rows, H, generator=g).to(dtype)
    d.view(-1)[::7] = 0.0
    return ids, d, torch.randn(table_rows, H, generator=g)


def sliced_ref(ids, d, table_rows, per):
    """fp64 (partials (slices, table_rows, H), their gates): scatter_ref of each slice of ``per`` rows."""
    parts = [scatter_ref(ids[r0:r0 + per], d[r0:r0 + per], table_rows) for r0 in range(0, len(ids), per)]
    return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])


def wrapper_slice_rows(rows, table_rows):
    """ops.embedding_grad_small's slice: 64 rows, doubled while slices x table_rows exceeds 4 096 workgroups."""
    per = 64
    while (rows + per - 1) // per * table_rows > 4096:
        per *= 2
    return per
