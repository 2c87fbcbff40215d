"""The row kernels every encoder layer runs, on the MI355X against plain fp64 references at their shape and value edges:
bevbert_bias_gelu/relu_fwd/bwd with the column sums behind them, bevbert_rows_gather / bevbert_rows_scatter and ops.take_rows,
bevbert_segment_wsum with SegmentCSR, bevbert_embed_sum_layernorm_fwd with _EmbedLN.backward (plain tensors and the arena
route), bevbert_graph_bias_fwd/bwd, bevbert_dropout_add and bevbert_cast_f32 (csrc/colwise.hip, gather.hip, layernorm.hip, pointwise.hip, optimizer.hip;
ops_rowops.py).

Inputs and references live in tests/body_cases.py, written in fp64 on the values the kernel gets (bf16 inputs are rounded
to bf16 first, then widened); tests/test_body_refs_host.py pins them to the plain torch compositions on the CPU.  Branches
are reached by shape, never by an environment knob.

Gates -- none is taken from the code under test:

* gathers, ReLU's y and dx, rows no id names, the padding row, dropped elements, casts, repeats: exact;
* GELU, with a = |x + bias|: y within K 2^-22 max(1, a); dx within K 2^-22 max(1, a) |dy| + 2^-24 |want|; dbias within the
  sum over the rows of the dx gate plus (rows + 4) 2^-24 sum |dx|; K = 4, twice what torch's fp32 GELU and an fp32
  restatement of the Abramowitz-Stegun form need on these inputs (host test).  No relative gate on the negative tail;
* sums of k terms (scatter, segment gather): (k + 2) 2^-24 sum |terms|.  A second scatter adds to a stored row: that row
  is one more term (the last addition errs by 2^-24 of the whole sum, however small the new rows are; host test);
* BertEmbeddings: max(1e-4 max(1, |want|max) for y, 1e-4 |want|max for the gradients, 4 x e32), e32 the error of torch's fp32
  F.layer_norm composition on the CPU; bf16 gradients of the tables add the summed 2^-8 |dz| (dz is stored in bf16 before
  it is routed), and plain bf16 tables, whose gradient autograd returns in bf16, one more 2^-8 |want|;
* graph bias: (n / nb / 256 + nb + 16) 2^-24 sum |terms| for the two sums, 2^-23 (|d w| + |b|) for the forward;
* dropout_add, kept elements: 2^-24 (4 |x| / (1 - p) + 2 |res|).  First stated as 2 x 2^-24 (|x| / (1 - p) + |res|), which
  plain fp32 arithmetic exceeds 1.34 times: four roundings touch the x term (body_cases.dropout_want, host test);
* any result stored in bf16: 2^-8 |want| on top.

Every test prints its worst error per quantity under ``-s`` (lines that begin with "body-kernel-errors:");
profiles/body_kernel_errors.txt is that output from the MI355X.
"""
import functools

import pytest
import torch

from tests import body_cases as bc
from tests.body_cases import DT_ID, DTYPES, U8, U24
from tests.kernel_gates import Worst as _Worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
Worst = functools.partial(_Worst, prefix="body-kernel-errors:")
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


def _bf(t, on):
    return U8 * t.abs() if on else 0.0


# ----------------------------------------------------------------------------- 1. bias + GELU / ReLU
@pytest.mark.parametrize("rows,C", bc.GELU_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_bias_gelu_every_launch_shape_and_the_negative_tail(ops, dtype, rows, C):
    """ops.bias_gelu forward and backward at every shape at which bias_act_fwd / bias_act_bwd launch differently: the 4-wide
    bf16 forward (C % 8 != 0), one and two column slices, fewer rows than a block owns, the 10 / 16 rows-per-block switch,
    both grid caps with their unrolled batches and tail rows.  x + bias ramps over [-14, 14] along rows and columns and
    holds 0.0, -0.0 and +-40."""
    x, bias, dy = bc.gelu_case(rows, C, dtype)
    a, y, _, dx, dbias = bc.gelu_ref(x, bias, dy)
    gy, gdx, gdb = bc.gelu_gates(a, y, dx, dy, dtype == BF)
    xd, bd = x.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    got = ops.bias_gelu(xd, bd)
    got.backward(dy.to(DEV))
    worst = Worst(f"bias_gelu {DT_ID(dtype)} {rows}x{C}")
    unit = bc.U22 * a.clamp_min(1.0)
    worst.bound("y", got, y, gy)
    worst.bound("dx", xd.grad, dx, gdx)
    worst.bound("dbias", bd.grad, dbias, gdb)
    # observed units of 2^-22 max(1, a) (gate: K = 4); a bf16 y or dx hides them behind its own rounding, so for bf16 they
    # are read off dbias, which sums the unrounded fp32 values
    err = lambda g, w: (g.detach().double().cpu() - w).abs()
    if dtype == torch.float32:
        worst.note("y units", float((err(got, y) / unit).max()), bc.GELU_K)
        den = (unit * dy.double().abs() + U24 * dx.abs()).clamp_min(1e-300)
        worst.note("dx units", float(torch.where(dy.double() == 0, torch.zeros_like(den), err(xd.grad, dx) / den).max()), bc.GELU_K)
    worst.note("dbias units", bc.GELU_K * float((err(bd.grad, dbias) / gdb.clamp_min(1e-300)).max()), bc.GELU_K)
    worst.report()


@pytest.mark.parametrize("rows,C", bc.RELU_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_bias_relu_is_exact_and_its_column_sums_hold_the_bound(ops, dtype, rows, C):
    x, bias, dy = bc.gelu_case(rows, C, dtype)
    y, dx, dbias = bc.relu_ref(x, bias, dy)
    xd, bd = x.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    got = ops.bias_relu(xd, bd)
    got.backward(dy.to(DEV))
    assert torch.equal(got.detach().cpu(), y) and torch.equal(xd.grad.cpu(), dx)
    worst = Worst(f"bias_relu {DT_ID(dtype)} {rows}x{C}")
    worst.bound("dbias", bd.grad, dbias, (rows + 4) * U24 * dx.double().abs().sum(0))
    worst.report()


@pytest.mark.parametrize("rows,C", [(11, 40), (333, 3072)])
def test_bias_gelu_bf16_unaligned_views_take_the_4_wide_kernel_with_equal_bits(ops, rows, C):
    """x and y 8 bytes into a larger buffer with C % 8 == 0: bias_gelu_fwd_kernel<bf16, 0> instead of the 8-wide kernel; both
    go through gelu4_of<bf16_raw>, so the bits equal the aligned call's."""
    from vln_bevbert_amd.lib import BF16, call, ptr, stream
    x, bias, _ = bc.gelu_case(rows, C, BF)
    n = rows * C
    bufx, bufy = torch.zeros(n + 8, dtype=BF, device=DEV), torch.full((n + 8,), 3.0, dtype=BF, device=DEV)
    xv, yv = bufx[4:4 + n].view(rows, C), bufy[4:4 + n].view(rows, C)
    xv.copy_(x)
    xa, ya, bd = x.to(DEV), torch.empty(rows, C, dtype=BF, device=DEV), bias.to(DEV)
    assert xv.data_ptr() % 16 == 8 and yv.data_ptr() % 16 == 8 and xa.data_ptr() % 16 == 0 and ya.data_ptr() % 16 == 0
    call("bevbert_bias_gelu_fwd", ptr(xv), ptr(bd), ptr(yv), rows, C, BF16, stream())
    call("bevbert_bias_gelu_fwd", ptr(xa), ptr(bd), ptr(ya), rows, C, BF16, stream())
    assert torch.equal(yv, ya)
    assert bool((bufy[:4] == 3.0).all()) and bool((bufy[4 + n:] == 3.0).all())


# ----------------------------------------------------------------------------- 2. row gather and scatter
@pytest.mark.parametrize("H", bc.ROW_WIDTHS + [2048])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_rows_gather_copies_rows_bit_for_bit(ops, dtype, H):
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    g = torch.Generator().manual_seed(H)
    src = torch.randn(bc.TABLE_ROWS, H, generator=g).to(dtype).to(DEV)
    for kind in ("one", "firstlast", "r257"):
        ids = bc.scatter_ids(kind).to(DEV)
        out = torch.full((len(ids) + 2, H), 3.0, dtype=dtype, device=DEV)
        call("bevbert_rows_gather", ptr(src), ptr(ids), ptr(out), len(ids), H, dtype_code(src), stream())
        assert torch.equal(out[:len(ids)], src[ids]) and bool((out[len(ids):] == 3.0).all()), kind


@pytest.mark.parametrize("H", bc.ROW_WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_rows_scatter_sums_duplicates_and_accumulates_once_rounded(ops, dtype, H):
    """bevbert_rows_scatter directly: into a sentinel-filled table (accumulate 0 stores the touched rows, the others keep
    their bits), then a second scatter with accumulate 1 onto the result -- for bf16 a read of the stored bf16 row, an fp32
    sum and one rounding.  Widths that fill part of a lane's four column groups, the last one (H in (768, 1024]) included."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    bf = dtype == BF
    worst = Worst(f"rows_scatter {DT_ID(dtype)} H={H}")
    for n, kind in enumerate(bc.SCATTER_KINDS):
        g = torch.Generator().manual_seed(H + n)
        ids = bc.scatter_ids(kind)
        ids2 = bc.scatter_ids(bc.SCATTER_KINDS[(n + 1) % len(bc.SCATTER_KINDS)], seed=1)
        d, d2 = torch.randn(len(ids), H, generator=g).to(dtype), torch.randn(len(ids2), H, generator=g).to(dtype)
        want, gate, touched = bc.scatter_ref(ids, d)
        idd, dd, idd2, dd2 = ids.to(DEV), d.to(DEV), ids2.to(DEV), d2.to(DEV)
        runs = []
        for _ in range(2):
            out = torch.full((bc.TABLE_ROWS, H), 3.0, dtype=dtype, device=DEV)
            call("bevbert_rows_scatter", ptr(idd), ptr(dd), ptr(out), len(ids), H, dtype_code(out), 0, stream())
            first = out.clone()
            call("bevbert_rows_scatter", ptr(idd2), ptr(dd2), ptr(out), len(ids2), H, dtype_code(out), 1, stream())
            runs.append((first.cpu(), out.cpu()))
        (first, second), again = runs
        assert torch.equal(first, again[0]) and torch.equal(second, again[1]), kind
        assert bool((first[~touched] == 3.0).all()), kind
        worst.bound("store", first[touched], want[touched], (gate + _bf(want, bf))[touched], where=kind)
        want2, gate2, touched2 = bc.scatter_ref(ids2, d2, first)
        assert torch.equal(second[~touched2], first[~touched2]), kind
        worst.bound("accumulate", second[touched2], want2[touched2], (gate2 + _bf(want2, bf))[touched2], where=kind)
    worst.report()


@pytest.mark.parametrize("H", bc.ROW_WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_take_rows_two_selections_share_one_gradient(ops, dtype, H):
    bf = dtype == BF
    g = torch.Generator().manual_seed(H + 3)
    x = torch.randn(bc.TABLE_ROWS, H, generator=g).to(dtype).to(DEV).requires_grad_(True)
    idx, idx2 = bc.scatter_ids("quarters"), bc.scatter_ids("r257", seed=1)
    idx2[5:9] = 2                                   # overlaps the first selection's 700-row id
    da, db = torch.randn(len(idx), H, generator=g).to(dtype), torch.randn(len(idx2), H, generator=g).to(dtype)

    def run(second):
        x.grad = None
        a, b = ops.take_rows(x, idx.to(DEV), idx2.to(DEV))
        assert torch.equal(a, x.detach()[idx.to(DEV)]) and torch.equal(b, x.detach()[idx2.to(DEV)])
        torch.autograd.backward([a, b] if second else [a], [da.to(DEV), db.to(DEV)] if second else [da.to(DEV)])
        return x.grad.cpu()
    first, both = run(False), run(True)
    worst = Worst(f"take_rows {DT_ID(dtype)} H={H}")
    want, gate, touched = bc.scatter_ref(idx, da)
    assert bool((first[~touched] == 0).all())
    worst.bound("first", first, want, gate + _bf(want, bf))
    want2, gate2, touched2 = bc.scatter_ref(idx2, db, first)
    assert torch.equal(both[~touched2], first[~touched2])
    worst.bound("both", both, want2, torch.where(touched2[:, None], gate2 + _bf(want2, bf), torch.zeros_like(gate2)))
    assert torch.equal(run(True), both)
    worst.report()


def test_rows_scatter_refuses_widths_beyond_its_lds_fold():
    from vln_bevbert_amd import lib
    l = lib.load()
    for code in (lib.F32, lib.BF16):
        rc = l.bevbert_rows_scatter(None, None, None, 1, 1028, code, 0, None)
        assert rc == -1 and b"rows_scatter: H=1028 must be a multiple of 4 and <= 1024" in l.bevbert_last_error()


# ----------------------------------------------------------------------------- 3. segment gather
def _segment_run(ops, csr, src, dy):
    s = src.to(DEV).requires_grad_(True)
    out = ops.segment_wsum(s, csr)
    out.backward(dy.to(DEV))
    return out.detach().cpu(), s.grad.cpu()


@pytest.mark.parametrize("H", bc.SEG_WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_segment_wsum_hand_built_segments_update_and_capacity(ops, dtype, H):
    """SegmentCSR from small integer lists: empty segments (first and last), 1, 5 and 130 entries, repeated sources, a source
    nobody reads, capacity = entries + 7; then update() to an aggregation with fewer entries, which must give the bits of a
    freshly built CSR.  H = 4 and 40 leave most of the 192 threads idle, 1024 takes a second pass of their loop."""
    bf = dtype == BF
    g = torch.Generator().manual_seed(H)
    src = torch.randn(bc.SEG_N_SRC, H, generator=g).to(dtype)
    dy = torch.randn(len(bc.SEGMENTS_A), H, generator=g).to(dtype)
    worst = Worst(f"segment_wsum {DT_ID(dtype)} H={H}")
    rowptr, idx, w = bc.segment_lists(bc.SEGMENTS_A)
    csr = ops.SegmentCSR(rowptr, idx, w, bc.SEG_N_SRC, DEV, capacity=len(idx) + 7)
    for name, segments in (("A", bc.SEGMENTS_A), ("B after update", bc.SEGMENTS_B)):
        rowptr, idx, w = bc.segment_lists(segments)
        if segments is bc.SEGMENTS_B:
            csr.update(rowptr, idx, w)
        out, dsrc = _segment_run(ops, csr, src, dy)
        want, gate, dwant, dgate = bc.segment_ref(rowptr, idx, w, src, bc.SEG_N_SRC, dy)
        worst.bound("out", out, want, gate + _bf(want, bf), where=name)
        worst.bound("dsrc", dsrc, dwant, dgate + _bf(dwant, bf), where=name)
        empty = [r for r, s in enumerate(segments) if not s]
        unread = sorted(set(range(bc.SEG_N_SRC)) - {i for s in segments for i in s})
        assert empty and unread and bool((out[empty] == 0).all()) and bool((dsrc[unread] == 0).all()), name
        fresh = _segment_run(ops, ops.SegmentCSR(rowptr, idx, w, bc.SEG_N_SRC, DEV), src, dy)
        assert torch.equal(fresh[0], out) and torch.equal(fresh[1], dsrc), name
    worst.report()


# ----------------------------------------------------------------------------- 4. BertEmbeddings
class _Emb(torch.nn.Module):
    def __init__(self, case, padding_idx):
        super().__init__()
        V, H = case["word"].shape
        self.word = torch.nn.Embedding(V, H, padding_idx=padding_idx)
        self.pos = torch.nn.Embedding(case["pos"].shape[0], H)
        self.typ = torch.nn.Embedding(2, H)
        self.ln = torch.nn.LayerNorm(H, eps=bc.EMBED_EPS)
        with torch.no_grad():
            for p, k in ((self.word.weight, "word"), (self.pos.weight, "pos"), (self.typ.weight, "typ"),
                         (self.ln.weight, "gamma"), (self.ln.bias, "beta")):
                p.copy_(case[k])


SINK0 = 0.5                   # what every gradient sink of the arena route holds before the backward: the kernels add


def _embed_plain(ops, case, dtype, padding_idx):
    ps = {k: case[k].to(dtype).to(DEV).requires_grad_(True) for k in ("word", "pos", "typ")}
    ps.update({k: case[k].to(DEV).requires_grad_(True) for k in ("gamma", "beta")})
    y = ops.embed_sum_layernorm(case["ids"].to(DEV), ps["word"], ps["pos"], ps["typ"], ps["gamma"], ps["beta"], bc.EMBED_EPS,
                                case["type_index"], padding_idx)
    y.backward(case["dy"].to(dtype).to(DEV))
    torch.cuda.synchronize()
    out = {k: p.grad.cpu() for k, p in ps.items()}
    out["y"] = y.detach().cpu()
    return out


def _embed_arena(ops, case, dtype, padding_idx):
    from vln_bevbert_amd.arena import ParamArena
    m = _Emb(case, padding_idx)
    arena = ParamArena(m, DEV, dtype)
    arena.grads.fill_(SINK0)
    ops.RT.scratch.reset()
    y = ops.embed_sum_layernorm(case["ids"].to(DEV), m.word.weight, m.pos.weight, m.typ.weight, m.ln.weight, m.ln.bias,
                                bc.EMBED_EPS, case["type_index"], padding_idx)
    y.backward(case["dy"].to(dtype).to(DEV))
    arena.sync()
    torch.cuda.synchronize()
    out = {"y": y.detach().cpu()}
    for k, n in (("word", "word.weight"), ("pos", "pos.weight"), ("typ", "typ.weight"), ("gamma", "ln.weight"), ("beta", "ln.bias")):
        o, cnt = arena.slices[n]
        out[k] = arena.grads[o:o + cnt].view(case[k].shape).cpu().clone()
    if dtype != torch.float32:                    # the compute copies the kernel read are the masters rounded once
        assert torch.equal(m.word.weight.compute.cpu(), case["word"].to(dtype))
    return out


@pytest.mark.parametrize("V,H,B,L", bc.EMBED_SHAPES)
@pytest.mark.parametrize("padding_idx", [None, 0], ids=["nopad", "pad0"])
@pytest.mark.parametrize("route", ["plain", "arena"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_bert_embeddings_forward_and_every_gradient_by_both_routes(ops, dtype, route, padding_idx, V, H, B, L):
    """ops.embed_sum_layernorm through plain tensors and through parameters in a ParamArena, where the type row's gradient
    is the LayerNorm backward's third column sum and the word and position gradients are deferred to the weight-gradient
    stream; the arena's sinks hold 0.5 beforehand (the kernels add).  One row (B = L = 1), 17 and 64 positions, type row 1
    for the 17-token shape; padding_idx 0 with id 0 in the first and the last row."""
    bf = dtype == BF
    case = bc.embed_case(V, H, B, L)
    run = _embed_plain if route == "plain" else _embed_arena
    got, again = run(ops, case, dtype, padding_idx), run(ops, case, dtype, padding_idx)
    ref, r32 = bc.embed_ref(case, dtype, padding_idx), bc.embed_torch(case, dtype, padding_idx, torch.float32)
    base = SINK0 if route == "arena" else 0.0
    worst = Worst(f"embed {DT_ID(dtype)} {route} pad={padding_idx} V={V} H={H} {B}x{L}")
    worst.check("y", got["y"], ref["y"], r32["y"], 1e-4, bf16_out=bf)
    for k in ("word", "pos", "typ", "gamma", "beta"):
        assert torch.equal(got[k], again[k]), k
        want = ref[k] + base
        top = float(want.abs().max())
        e32 = float((r32[k].double() + base - want).abs().max())
        allow = torch.full_like(want, max(1e-4 * top, 4.0 * e32))
        if bf and k in ref["abs"]:
            allow = allow + U8 * ref["abs"][k] + (U8 * want.abs() if route == "plain" else 0.0)
        worst.bound(k, got[k], want, allow, e32=r32[k].double() + base - want)
    assert torch.equal(got["y"], again["y"])
    if padding_idx == 0:
        assert bool((got["word"][0] == base).all())
    assert bool((got["typ"][1 - case["type_index"]] == base).all())
    assert bool((got["pos"][L:] == base).all())
    worst.report()


# ----------------------------------------------------------------------------- 5. graph bias
@pytest.mark.parametrize("layers,B,nh,G", bc.GRAPH_SHAPES)
def test_graph_bias_forward_and_the_two_sums_over_layers_samples_and_heads(ops, layers, B, nh, G):
    """bevbert_graph_bias_bwd directly: contiguous runs of the (layers, B, nh, G, G) gradients that straddle heads, samples
    and layers (n a multiple of neither 256 nor 4 096), and nb at its cap of 512; dw and db start at non-zero values."""
    from vln_bevbert_amd.lib import call, ptr, stream
    dbias, dists = bc.graph_case(layers, B, nh, G)
    dw, db, gw, gb = bc.graph_ref(dbias, dists)
    dbd, dd = dbias.to(DEV), dists.to(DEV)
    ws = torch.empty(1024, device=DEV)
    runs = []
    for _ in range(2):
        out = torch.tensor([bc.GRAPH_DW0, bc.GRAPH_DB0, 7.0], device=DEV)
        call("bevbert_graph_bias_bwd", ptr(dbd), ptr(dd), layers, B, nh, G, ptr(out[0:]), ptr(out[1:]), ptr(ws), stream())
        runs.append(out.cpu())
    assert torch.equal(runs[0], runs[1]) and float(runs[0][2]) == 7.0
    worst = Worst(f"graph_bias layers={layers} B={B} nh={nh} G={G}")
    worst.bound("dw", runs[0][0], torch.tensor(dw, dtype=torch.float64), gw)
    worst.bound("db", runs[0][1], torch.tensor(db, dtype=torch.float64), gb)
    w, b = torch.tensor([1.7], device=DEV), torch.tensor([-0.3], device=DEV)
    out = torch.full((dists.numel() + 2,), 3.0, device=DEV)
    call("bevbert_graph_bias_fwd", ptr(dd), ptr(w), ptr(b), ptr(out), dists.numel(), stream())
    dwp = dists.double().view(-1) * float(w)
    worst.bound("fwd", out[:-2], dwp + float(b), 2.0 ** -23 * (dwp.abs() + abs(float(b))))
    assert bool((out[-2:] == 3.0).all())
    worst.report()


# ----------------------------------------------------------------------------- 6. dropout_add and cast_f32
@pytest.mark.parametrize("n", [4, bc.BIG_N])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("tin,tout", [(torch.float32, torch.float32), (torch.float32, BF), (BF, BF)],
                         ids=["f32-f32", "f32-bf16", "bf16-bf16"])
def test_dropout_add_beyond_the_grid_cap_against_the_exported_mask(ops, tin, tout, with_res, n):
    """8 388 608 + 148 elements: the grid is capped at 8 192 blocks, the first 37 threads loop once more.  Against the
    keep mask of ops.dropout_keep_mask for the same (seed, offset), element by element, on the device in fp64."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    seed, offset = 1234, 4096
    g = torch.Generator(device=DEV).manual_seed(n % 1000)
    x = torch.randn(n, generator=g, device=DEV).to(tin)
    res = torch.randn(n, generator=g, device=DEV).to(tout) if with_res else None
    y = torch.full((n + 4,), 3.0, dtype=tout, device=DEV)
    call("bevbert_dropout_add", ptr(x), ptr(res), ptr(y), n, dtype_code(x), dtype_code(y), bc.DROP_P, seed, offset, stream())
    keep = ops.dropout_keep_mask(n, bc.DROP_P, seed, offset, DEV)
    assert bool((y[n:] == 3.0).all())
    if n > 4:
        assert 0.895 < float(keep.float().mean()) < 0.905
    want, gate, _ = bc.dropout_want(x, res, keep)
    drop = ~keep
    assert torch.equal(y[:n][drop], res[drop] if with_res else torch.zeros_like(y[:n][drop]))
    worst = Worst(f"dropout_add {DT_ID(tin)}->{DT_ID(tout)} res={with_res} n={n}")
    worst.bound("y", y[:n], want, gate + _bf(want, tout == BF))
    worst.report()


@pytest.mark.parametrize("n", [4, bc.CAST_BIG_N])
@pytest.mark.parametrize("dtype", [BF, torch.float16], ids=DT_ID)
def test_cast_f32_equals_the_cpu_conversion_bit_for_bit(ops, dtype, n):
    """Ties of both parities, values below the destination's maximum that round to inf, subnormals, underflow, +-0, +-inf,
    NaN and random bit patterns; beyond the grid cap the first thread loops once more."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    src = bc.cast_values(n, dtype)
    srcd, dst = src.to(DEV), torch.full((n + 4,), 3.0, dtype=dtype, device=DEV)
    call("bevbert_cast_f32", ptr(srcd), ptr(dst), n, dtype_code(dtype), stream())
    got, want = dst[:n].cpu(), src.to(dtype)
    assert bool((dst[n:] == 3.0).all())
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    same = got.view(torch.int16)[ok] == want.view(torch.int16)[ok]
    bad = (~same).nonzero().view(-1)[:5]
    assert bool(same.all()), (int((~same).sum()), src[ok][bad].tolist(), got[ok][bad].tolist(), want[ok][bad].tolist())
    print(f"body-kernel-errors: cast_f32 -> {DT_ID(dtype)} n={n}: {int(ok.sum())} bit patterns equal, {int(want.isnan().sum())} NaN positions equal")
