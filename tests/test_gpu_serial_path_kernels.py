"""The kernels on the serial path of the training step that keep several loads in flight per thread -- the split-K fold
(bevbert_multi_accum / bevbert_accum_partials), the second stage of the column reductions (bevbert_multi_finalize /
bevbert_colsum_finalize), lift / splat (bevbert_bev_bin_points -> bevbert_bev_splat_mean) and the LayerNorm backward
at few rows -- at the smallest shapes where an unrolled loop, a remainder or a wider workgroup can go wrong.

The folds, the finalize kernels and the splat only add (no multiply, so no FMA): their results are compared for EQUALITY
with numpy float32 sums made in the documented order.  The LayerNorm backward is compared with the fp64 reference under the
bounds of tests/test_gpu_rowops_full_size.py.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_rowops_full_size import (_gen, _keep, _leaf64, _ln_ref64, bf16_rounding_ratio, rel_err, report)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32_CODE, BF16_CODE = 0, 1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


def _call(name, *args):
    from vln_bevbert_amd import lib
    lib.call(name, *args, lib.stream())
    torch.cuda.synchronize()


def _table(records, dtype):
    """Device copy of a task table built from a numpy structured dtype (40-byte records)."""
    assert dtype.itemsize == 40
    host = np.array(records, dtype=dtype)
    return torch.from_numpy(host.view(np.uint8).copy()).to(DEV)


# ----------------------------------------------------------------------------- split-K folds
ACCUM_TASK = np.dtype([("partials", "<u8"), ("sink", "<u8"), ("n4_total", "<u8"), ("off4", "<u4"), ("n4", "<u4"),
                       ("S", "<i4"), ("dtype", "<i4")])
GUARD = 8           # floats left alone before and after every sink range


def _fold_ref(sink, parts):
    """((sink + p0) + p1) + ... in float32"""
    acc = sink.astype(np.float32).copy()
    for p in parts:
        acc = (acc + p.astype(np.float32)).astype(np.float32)
    return acc


@pytest.mark.parametrize("dt", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [1, 2, 3, 5, 8, 32])
def test_multi_accum_exact(ops, S, dt):
    """One launch over hand-built tasks: single-task weights of 1 ... 4 096 float4 groups that start inside their slice
    (off4 != 0), and one weight of 2 * 4 096 + 5 groups cut into three tasks; fp32 / bf16 partials, a non-zero sink.
    Every sink range equals the sequential float32 sum, and the guard floats around it keep their values."""
    rnd = _gen(1000 + S)
    weights = [(n4, 7, n4 + 7 + 3, [(0, n4)]) for n4 in (1, 3, 255, 256, 257, 1023, 4096)]
    weights.append((2 * 4096 + 5, 0, 2 * 4096 + 5, [(0, 4096), (4096, 4096), (8192, 5)]))
    total = sum(n4 * 4 + 2 * GUARD for n4, *_ in weights)
    sink = rnd(total)
    before = sink.cpu().numpy().copy()
    want = before.copy()
    records, keep_alive, spans, pos = [], [], [], 0
    for n4, off4, n4_total, tasks in weights:
        part = rnd(S, n4_total * 4).to(dt).contiguous()
        keep_alive.append(part)
        lo = pos + GUARD
        ph = part.float().cpu().numpy()
        want[lo:lo + n4 * 4] = _fold_ref(before[lo:lo + n4 * 4], [ph[s, off4 * 4:(off4 + n4) * 4] for s in range(S)])
        for t_off, t_n in tasks:        # t_off counts from the weight's first group
            records.append((part.data_ptr(), sink.data_ptr() + (lo + t_off * 4) * 4, n4_total, off4 + t_off, t_n, S,
                            BF16_CODE if dt == BF16 else F32_CODE))
        spans.append((n4, lo, lo + n4 * 4))
        pos = lo + n4 * 4 + GUARD
    table = _table(records, ACCUM_TASK)
    _call("bevbert_multi_accum", table.data_ptr(), len(records))
    got = sink.cpu().numpy()
    bad = got != want
    where = {n4: (int(bad[a:b].sum()), (np.flatnonzero(bad[a:b])[:4] // 4).tolist()) for n4, a, b in spans if bad[a:b].any()}
    assert not bad.any(), f"{int(bad.sum())} of {total} floats differ; (count, first float4 groups) per n4: {where}"


@pytest.mark.parametrize("n4,S,dt", [(1, 3, BF16), (255, 5, torch.float32), (1023, 4, BF16), (5000, 9, torch.float32),
                                     (2 * 8192 * 256 + 300, 2, BF16)])
def test_accum_partials_exact(ops, n4, S, dt):
    """The single-weight entry (the same loop over a grid-stride range): below one element per thread, and past the
    8 192-block cap where a thread takes several elements and a remainder."""
    rnd = _gen(n4 % 9973 + S)
    sink = rnd(n4 * 4 + 2 * GUARD)
    part = rnd(S, n4 * 4).to(dt).contiguous()
    want = sink.cpu().numpy().copy()
    ph = part.float().cpu().numpy()
    want[GUARD:GUARD + n4 * 4] = _fold_ref(want[GUARD:GUARD + n4 * 4], [ph[s] for s in range(S)])
    _call("bevbert_accum_partials", part.data_ptr(), sink.data_ptr() + GUARD * 4, S, n4 * 4,
          BF16_CODE if dt == BF16 else F32_CODE)
    assert np.array_equal(sink.cpu().numpy(), want)


# ----------------------------------------------------------------------------- second stage of the column reductions
FINALIZE_TASK = np.dtype([("partials", "<u8"), ("out", "<u8"), ("nblocks", "<i4"), ("row_stride", "<i4"),
                          ("col0", "<i4"), ("ncols", "<i4"), ("accumulate", "<i4"), ("pad", "<i4")])


def _finalize_ref(p, out, accumulate):
    """p [nblocks][ncols]: 16 running float32 sums over b = ty, ty + 16, ..., folded k = 0 ... 15, then the accumulate rule"""
    s = np.zeros((16, p.shape[1]), np.float32)
    for b in range(p.shape[0]):
        s[b % 16] = s[b % 16] + p[b]
    t = s[0].copy()
    for k in range(1, 16):
        t = t + s[k]
    return (out + t).astype(np.float32) if accumulate else t


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nblocks", [1, 15, 16, 17, 33, 127, 512, 1000])
def test_multi_finalize_and_colsum_finalize_exact(ops, nblocks, accumulate):
    rnd = _gen(nblocks * 2 + accumulate)
    # multi_finalize: three tasks of 1 / 63 / 64 columns at col0 != 0 inside rows wider than the columns used
    row_stride, records, outs, wants, parts = 200, [], [], [], []
    for ncols, col0 in ((1, 5), (63, 64), (64, 130)):
        part = rnd(nblocks, row_stride)
        out = rnd(ncols + 2 * GUARD)
        want = out.cpu().numpy().copy()
        want[GUARD:GUARD + ncols] = _finalize_ref(part.cpu().numpy()[:, col0:col0 + ncols], want[GUARD:GUARD + ncols],
                                                  accumulate)
        records.append((part.data_ptr(), out.data_ptr() + GUARD * 4, nblocks, row_stride, col0, ncols, accumulate, 0))
        parts.append(part); outs.append(out); wants.append(want)
    table = _table(records, FINALIZE_TASK)
    _call("bevbert_multi_finalize", table.data_ptr(), len(records))
    for out, want in zip(outs, wants):
        assert np.array_equal(out.cpu().numpy(), want)
    # colsum_finalize: partials [nblocks][3][C], the middle output absent
    for C in (1, 63, 64, 130):
        part = rnd(nblocks, 3, C)
        o0, o2 = rnd(C), rnd(C)
        ph = part.cpu().numpy()
        w0 = _finalize_ref(ph[:, 0], o0.cpu().numpy(), accumulate)
        w2 = _finalize_ref(ph[:, 2], o2.cpu().numpy(), accumulate)
        _call("bevbert_colsum_finalize", part.data_ptr(), nblocks, 3, C, o0.data_ptr(), None, o2.data_ptr(), accumulate)
        assert np.array_equal(o0.cpu().numpy(), w0) and np.array_equal(o2.cpu().numpy(), w2), C


# ----------------------------------------------------------------------------- lift (mode 1) -> splat
RES = 0.5


def _points_in_cells(cells, dim):
    """Ego-frame points at the centres of the given cells (exact in fp32 for res 0.5): (P, 3)"""
    half = (dim - 1) / 2.0
    cells = np.asarray(cells)
    pts = np.zeros((len(cells), 3), np.float32)
    pts[:, 0] = ((cells % dim) - half) * RES
    pts[:, 2] = ((cells // dim) - half) * RES
    return pts


def _check_binning(cell, order, start, K):
    for i in range(cell.shape[0]):
        kept = np.flatnonzero(cell[i] >= 0)
        assert np.array_equal(start[i], np.concatenate([[0], np.cumsum(np.bincount(cell[i][kept], minlength=K))]))
        assert start[i, K] == len(kept)
        assert np.array_equal(order[i, :len(kept)], kept[np.argsort(cell[i][kept], kind="stable")])


@pytest.mark.parametrize("dim", [21, 32])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000, 2352, 24576])
def test_bin_points_counting_sort(ops, P, dim):
    """Four samples: every point in one cell, every point dropped, the points dealt over all cells in turn (each in its
    own cell while P <= dim^2), and random cells with ~40 % dropped.  The cell ids are the constructed ones, cell_start the
    cumulative count of the kernel's cell ids and order the stable argsort of the kept points."""
    K = dim * dim
    g = np.random.default_rng(P * 37 + dim)
    cells = np.stack([np.full(P, K // 2 + 3), g.integers(0, K, P), np.arange(P) % K, g.integers(0, K, P)])
    drop = np.zeros((4, P), bool)
    drop[1] = True
    drop[3] = g.random(P) < 0.4
    pts = np.stack([_points_in_cells(c, dim) for c in cells])
    cell, order, start = ops.bev_bin_points(torch.from_numpy(pts).to(DEV), torch.from_numpy(drop).to(DEV), dim, RES)
    torch.cuda.synchronize()
    cell, order, start = cell.cpu().numpy(), order.cpu().numpy(), start.cpu().numpy()
    assert np.array_equal(cell, np.where(drop, -1, cells))
    _check_binning(cell, order, start, K)


SPLAT_COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 40)


@pytest.fixture(scope="module")
def splat_case(ops):
    """Two samples of 21 x 21 cells: cells 3 * j holding SPLAT_COUNTS[j] points in shuffled point order plus dropped
    points, and 1 000 random points with ~40 % dropped; binned once by the kernel."""
    g = np.random.default_rng(5)
    a = np.concatenate([np.full(n, 3 * j) for j, n in enumerate(SPLAT_COUNTS)] + [np.full(42, -1)])
    P = 1000
    a = np.concatenate([a, np.full(P - len(a), -1)])
    g.shuffle(a)
    b = np.where(g.random(P) < 0.4, -1, g.integers(0, 441, P))
    cells = np.stack([a, b])
    drop = cells < 0
    pts = np.stack([_points_in_cells(np.maximum(c, 0), 21) for c in cells])
    cell, order, start = ops.bev_bin_points(torch.from_numpy(pts).to(DEV), torch.from_numpy(drop).to(DEV), 21, RES)
    torch.cuda.synchronize()
    assert np.array_equal(cell.cpu().numpy(), cells)
    _check_binning(cell.cpu().numpy(), order.cpu().numpy(), start.cpu().numpy(), 441)
    counts = np.diff(start.cpu().numpy()[0])
    assert sorted(counts[counts > 0]) == sorted(n for n in SPLAT_COUNTS if n)
    return cells, order, start


@pytest.mark.parametrize("C", [768, 64])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_splat_mean_exact(ops, splat_case, dt, C):
    """Every cell's mean equals the float32 sum of its rows in point order divided by max(n, 1), bit for bit."""
    cells, order, start = splat_case
    B, P = cells.shape
    feat = _gen(C)(B, P, C).to(dt)
    out, _, _ = ops.bev_splat_mean(feat, order, start, 441, out_dtype=torch.float32)
    torch.cuda.synchronize()
    fh = feat.float().cpu().numpy()
    want = np.zeros((B, 441, C), np.float32)
    for b in range(B):
        n = np.zeros(441, np.float32)
        for p in range(P):              # ascending point id = the order of the kernel's lists
            if cells[b, p] >= 0:
                want[b, cells[b, p]] = want[b, cells[b, p]] + fh[b, p]
                n[cells[b, p]] += 1
        want[b] = want[b] / np.maximum(n, 1)[:, None]
    assert np.array_equal(out.cpu().numpy(), want)


# ----------------------------------------------------------------------------- LayerNorm backward, few rows
LN_ROWS = (2, 5, 9, 11, 41, 130)        # 10 rows per block: waves with zero, one, two and three rows


def _res32_step(ops, x, bias, residual, gamma, beta, a, b, outs, p, seed):
    from vln_bevbert_amd.ops_rowops import _BiasDropResLN32
    for t in (x, bias, residual, gamma, beta):
        t.grad = None
    ops.RT.new_step(seed)
    off = ops.RT.offset
    y16, y32 = _BiasDropResLN32.apply(x, bias, residual, gamma, beta, 1e-12, p)
    loss = 0
    if outs in ("both", "y16"):
        loss = loss + (y16.float() * a).sum()
    if outs in ("both", "y32"):
        loss = loss + (y32 * b).sum()
    loss.backward()
    torch.cuda.synchronize()
    return off, [t.grad.clone() for t in (x, residual, gamma, beta, bias)]


@pytest.mark.parametrize("res", ["f32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("outs", ["y16", "y32", "both"])
@pytest.mark.parametrize("H", [256, 768])
def test_res32_layernorm_bwd_few_rows(ops, H, outs, p, res):
    """bevbert_layernorm_res32_bwd where a wave has zero to three rows: dy16 only, dy32 only and both, with and without
    dropout, dz in fp32 and bf16; against the fp64 LayerNorm, and the same bits from a second launch."""
    for rows in LN_ROWS:
        rnd = _gen(rows * 131 + H)
        x = rnd(rows, H).to(BF16).requires_grad_(True)
        residual = (2 * rnd(rows, H)).to(BF16 if res == "bf16" else torch.float32).requires_grad_(True)
        gamma = (1 + 0.1 * rnd(H)).requires_grad_(True)
        beta = (0.1 * rnd(H)).requires_grad_(True)
        bias = (0.1 * rnd(H)).requires_grad_(True)
        a = rnd(rows, H).to(BF16).float()
        b = rnd(rows, H)
        off, got = _res32_step(ops, x, bias, residual, gamma, beta, a, b, outs, p, 99 + rows)
        _, again = _res32_step(ops, x, bias, residual, gamma, beta, a, b, outs, p, 99 + rows)
        assert all(torch.equal(u, v) for u, v in zip(got, again)), "a second launch gave other bits"
        keep = _keep(ops, rows * H, p, off, (rows, H))
        xd, rd, gd, bd, bid = (_leaf64(t) for t in (x, residual, gamma, beta, bias))
        dy = (a.double() if outs in ("both", "y16") else 0) + (b.double() if outs in ("both", "y32") else 0)
        _ln_ref64(xd, bid, rd, gd, bd, keep, p).backward(dy)
        dx, dz, dgamma, dbeta, dbias = got
        errs = {}
        if res == "f32":
            errs["dz"] = rel_err(dz, rd.grad)
            assert errs["dz"] <= 2e-5, (rows, errs)
        else:
            errs["dz_bf16"] = bf16_rounding_ratio(dz, rd.grad)
            assert errs["dz_bf16"] <= 1.0, (rows, errs)
        errs["dx16"] = bf16_rounding_ratio(dx, xd.grad)
        errs["dgamma"], errs["dbeta"], errs["dbias"] = rel_err(dgamma, gd.grad), rel_err(dbeta, bd.grad), rel_err(dbias, bid.grad)
        report(f"res32 LN bwd rows={rows} H={H} outs={outs} p={p} res={res}", **errs)
        assert errs["dx16"] <= 1.0, (rows, errs)
        assert max(errs["dgamma"], errs["dbeta"], errs["dbias"]) <= 1e-4, (rows, errs)


@pytest.mark.parametrize("H", [256, 768])
@pytest.mark.parametrize("rows", [1, 5])
def test_res32_layernorm_fwd_gives_the_bits_of_the_plain_layernorm(ops, rows, H):
    """ln_res32_fwd_kernel and ln_fwd_kernel share one row body: without dropout, y32 is bit for bit the plain fp32
    LayerNorm of (x + bias) + residual summed in that order, and y16 its bf16 rounding."""
    from vln_bevbert_amd.ops_rowops import _BiasDropResLN32
    rnd = _gen(rows * 17 + H)
    x = rnd(rows, H).to(BF16)
    residual, gamma, beta, bias = 2 * rnd(rows, H), 1 + 0.1 * rnd(H), 0.1 * rnd(H), 0.1 * rnd(H)
    y16, y32 = _BiasDropResLN32.apply(x, bias, residual, gamma, beta, 1e-12, 0.0)
    plain = ops.layernorm((x.float() + bias) + residual, gamma, beta, 1e-12)
    assert torch.equal(y32, plain) and torch.equal(y16, plain.to(BF16))


def _plain_step(ops, x, bias, residual, gamma, beta, dy, dz_add, p, seed):
    from vln_bevbert_amd.ops_rowops import _BiasDropResLN
    for t in (x, bias, residual, gamma, beta):
        t.grad = None
    ops.RT.new_step(seed)
    off = ops.RT.offset
    if dz_add is None:
        y = _BiasDropResLN.apply(x, bias, residual, gamma, beta, 1e-12, p, False, None, None)
        y.backward(dy)
    else:
        y, z = _BiasDropResLN.apply(x, bias, residual, gamma, beta, 1e-12, p, False, None, None, True)
        torch.autograd.backward([y, z], [dy, dz_add])
    torch.cuda.synchronize()
    return off, [t.grad.clone() for t in (x, residual, gamma, beta, bias)]


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "dz_add"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [256, 768])
def test_plain_layernorm_bwd_few_rows(ops, H, p, with_add, dt=torch.float32):
    """bevbert_layernorm_bwd_add on fp32 activations, with and without the addend that reaches z through its other
    consumer: activation gradients within 2e-5 of the fp64 ones relative to their largest element, parameter gradients
    within 1e-4 (the bounds of the fp32-residual kernel's fp32 outputs); the same bits from a second launch."""
    res32 = ops.RT.res32
    ops.RT.res32 = False
    try:
        for rows in LN_ROWS:
            rnd = _gen(rows * 17 + H)
            x = rnd(rows, H).to(dt).requires_grad_(True)
            residual = (2 * rnd(rows, H)).to(dt).requires_grad_(True)
            gamma = (1 + 0.1 * rnd(H)).requires_grad_(True)
            beta = (0.1 * rnd(H)).requires_grad_(True)
            bias = (0.1 * rnd(H)).requires_grad_(True)
            dy = rnd(rows, H).to(dt)
            dz_add = rnd(rows, H).to(dt) if with_add else None
            off, got = _plain_step(ops, x, bias, residual, gamma, beta, dy, dz_add, p, 7 + rows)
            _, again = _plain_step(ops, x, bias, residual, gamma, beta, dy, dz_add, p, 7 + rows)
            assert all(torch.equal(u, v) for u, v in zip(got, again)), "a second launch gave other bits"
            keep = _keep(ops, rows * H, p, off, (rows, H))
            xd, rd, gd, bd, bid = (_leaf64(t) for t in (x, residual, gamma, beta, bias))
            t = xd + bid
            if keep is not None:
                t = torch.where(keep, t / (1 - p), torch.zeros_like(t))
            z = t + rd
            y = torch.nn.functional.layer_norm(z, (H,), gd, bd, 1e-12)
            if with_add:
                torch.autograd.backward([y, z], [dy.double(), dz_add.double()])
            else:
                y.backward(dy.double())
            dx, dz, dgamma, dbeta, dbias = got
            errs = {"dz": rel_err(dz, rd.grad), "dx": rel_err(dx, xd.grad)}
            ok = errs["dz"] <= 2e-5 and errs["dx"] <= 2e-5
            errs["dgamma"], errs["dbeta"], errs["dbias"] = rel_err(dgamma, gd.grad), rel_err(dbeta, bd.grad), rel_err(dbias, bid.grad)
            report(f"plain LN bwd rows={rows} H={H} {dt} p={p} add={with_add}", **errs)
            assert ok and max(errs["dgamma"], errs["dbeta"], errs["dbias"]) <= 1e-4, (rows, errs)
    finally:
        ops.RT.res32 = res32


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "dz_add"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [256, 768])
def test_plain_layernorm_bwd_bf16_few_rows(ops, H, p, with_add):
    """A SELF-CONSISTENCY check of the same kernel on bf16 activations, called through the C ABI: the reference is the
    kernel's own documented formula (above ln_bwd_kernel) evaluated in fp64 on the operands as stored, not an independent
    fp64 LayerNorm -- an error in the formula itself would pass here; the fp32 test above and the fp32-stream tests compare
    with autograd.  Why: the bf16 forward saves z ROUNDED to bf16 next to the mean / rstd of the unrounded sum, so the
    backward is not the derivative of an fp64 LayerNorm of the forward's inputs to within a bf16 rounding.  Bounds: dz and
    dx (one rounding of an fp32 value whose own error is four orders smaller) within one bf16 rounding, the fp32 column
    sums within 1e-4."""
    from vln_bevbert_amd import lib
    seed = 11
    for rows in LN_ROWS:
        rnd = _gen(rows * 29 + H)
        z = (2 * rnd(rows, H)).to(BF16)
        dy = rnd(rows, H).to(BF16)
        add = rnd(rows, H).to(BF16) if with_add else None
        gamma = 1 + 0.1 * rnd(H)
        mean = z.float().mean(1).contiguous()
        rstd = (z.float().var(1, unbiased=False) + 1e-12).rsqrt().contiguous()
        ws = torch.empty(int(lib.load().bevbert_colsum_workspace_floats(3 * H)), device=DEV)
        off = 4096 * rows

        def run():
            dz, dx = torch.empty_like(z), torch.empty_like(z)
            dg, db, dbi = (torch.empty(H, device=DEV) for _ in range(3))
            _call("bevbert_layernorm_bwd_add", dy.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                  gamma.data_ptr(), dz.data_ptr(), dx.data_ptr(), None if add is None else add.data_ptr(), dg.data_ptr(),
                  db.data_ptr(), dbi.data_ptr(), ws.data_ptr(), rows, H, BF16_CODE, p, seed, off, 0)
            return dz, dx, dg, db, dbi

        got, again = run(), run()
        assert all(torch.equal(u, v) for u, v in zip(got, again)), "a second launch gave other bits"
        xh = (z.double() - mean.double()[:, None]) * rstd.double()[:, None]
        gd = gamma.double() * dy.double()
        dz_ref = rstd.double()[:, None] * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
        if with_add:
            dz_ref = dz_ref + add.double()
        dx_ref = dz_ref
        if p > 0:
            keep = ops.dropout_keep_mask(rows * H, p, seed, off, DEV).view(rows, H)
            dx_ref = torch.where(keep, dz_ref / (1 - p), torch.zeros_like(dz_ref))
        dz, dx, dg, db, dbi = got
        errs = {"dz": bf16_rounding_ratio(dz, dz_ref), "dx": bf16_rounding_ratio(dx, dx_ref),
                "dgamma": rel_err(dg, (dy.double() * xh).sum(0)), "dbeta": rel_err(db, dy.double().sum(0)),
                "dbias": rel_err(dbi, dx_ref.sum(0))}
        report(f"plain LN bwd bf16 rows={rows} H={H} p={p} add={with_add}", **errs)
        assert errs["dz"] <= 1.0 and errs["dx"] <= 1.0, (rows, errs)
        assert max(errs["dgamma"], errs["dbeta"], errs["dbias"]) <= 1e-4, (rows, errs)
