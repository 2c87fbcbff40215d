"""The small-K projection LayerNorm and the sliced small-table gradient on the MI355X, against plain fp64 references at their
launch-shape and value edges: smallk_ln_fwd_kernel, smallk_ln_bwd_kernel and smallk_finalize_kernel (csrc/smallk.hip)
through ops.smallk_linear_layernorm_plus with a module, a ParamArena and sinks that hold non-zero start values, and through
the C ABI for the null-pointer branches the wrapper cannot reach; embedding_grad_sliced_kernel (csrc/gather.hip) through
the C ABI and through ops.embedding_grad_small.

Inputs, references and gates live in tests/smallk_cases.py, written in fp64 on the values the kernel gets (bf16 inputs are
rounded to bf16 first, then widened); its docstring states every gate.  tests/test_smallk_refs_host.py pins the references to
torch's fp64 autograd composition and holds torch's fp32 composition and a numpy fp32 restatement of the kernels' own order
to half of every gate.  No gate is taken from the code under test; branches are reached by shape, never by an environment
knob.

Every test prints its worst error per quantity under ``-s`` (lines that begin with "smallk-kernel-errors:": the element
nearest its bound, the fp32 restatement's error at that element, the bound); profiles/smallk_kernel_errors.txt is that
output from the MI355X.
"""
import functools

import pytest
import torch

from tests import smallk_cases as sc
from tests.kernel_gates import Worst as _Worst
from tests.smallk_cases import DT_ID, DTYPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
Worst = functools.partial(_Worst, prefix="smallk-kernel-errors:")
NAMES = {"W": "lin.weight", "b": "lin.bias", "gamma": "ln.weight", "beta": "ln.bias", "table": "emb.weight"}
GRADS = {"W": "dW", "b": "db", "gamma": "dgamma", "beta": "dbeta", "table": "dtable"}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


def _module(c):
    K, H = c["K"], c["H"]

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin, self.ln = torch.nn.Linear(K, H), torch.nn.LayerNorm(H, eps=sc.EPS)
            self.emb = torch.nn.Embedding(sc.TABLE_ROWS, H)
    m = M()
    with torch.no_grad():
        for key, name in NAMES.items():
            dict(m.named_parameters())[name].copy_(c[key])
    return m


def _check_case(ops, params, worst):
    """One case through ops.smallk_linear_layernorm_plus: y and every gradient inside their gates elementwise, d post1 = dy
    bit for bit, the table row nobody names and the arena's padding untouched, rows of zero features bit-equal to each other,
    and the same bits from a second forward and backward out of the same start values."""
    from vln_bevbert_amd.arena import ParamArena
    c, r, k32 = sc.case(*params), sc.ref(*params), sc.kernel_f32(*params)
    rows, H, dtype = c["rows"], c["H"], c["dtype"]
    m = _module(c)
    arena = ParamArena(m, DEV, dtype)
    g = torch.Generator().manual_seed(rows + H)
    start = 0.5 + torch.rand(arena.grads.numel(), generator=g)            # the padding holds non-zero values too
    inside = torch.zeros(arena.grads.numel(), dtype=torch.bool)
    for key, name in NAMES.items():
        o, k = arena.slices[name]
        start[o:o + k] = c["start"][key].reshape(-1)
        inside[o:o + k] = True
    start_dev = start.to(DEV)
    feat, idx, dy = c["feat"].to(DEV), c["idx"].to(DEV), c["dy"].to(dtype).to(DEV)
    post1 = c["post1"].to(dtype).to(DEV).requires_grad_(True)
    assert ops.smallk_linear_layernorm_plus_supported(feat, m.lin, m.ln, post1, m.emb)
    assert torch.equal(ops._compute(m.emb.weight).float().cpu(), c["table"])       # the kernel reads the case's table values

    def run():
        arena.grads.copy_(start_dev)
        post1.grad = None
        ops.RT.scratch.reset()
        y = ops.smallk_linear_layernorm_plus(feat, m.lin, m.ln, sc.EPS, post1, m.emb, idx)
        y.backward(dy)
        arena.sync()
        torch.cuda.synchronize()
        return y.detach().clone(), arena.grads.clone(), post1.grad.clone()
    y, grads, dpost1 = run()
    where = c["tag"]
    worst.bound("y", y, r["y"], r["gate"]["y"], where, e32=k32["y_out"] - r["y"])
    gc = grads.cpu()
    for key, name in NAMES.items():
        o, k = arena.slices[name]
        q = GRADS[key]
        got = gc[o:o + k].view(c["start"][key].shape)
        worst.bound(q, got, r[q], r["gate"][q], where, e32=k32[q] - r[q] if q in k32 else None)
        if key == "table":
            assert torch.equal(got[-1], c["start"]["table"][-1]), "the table row nobody names changed"
    assert torch.equal(dpost1, dy), "d post1 is not dy bit for bit"
    assert torch.equal(gc[~inside], start[~inside]), "the arena's padding changed"
    yc, zr = y.cpu(), c["zero_rows"]
    for t in range(sc.TABLE_ROWS):
        same = (zr & (c["idx"] == t)).nonzero().view(-1)
        if len(same) > 1:
            assert torch.equal(yc[same], yc[same[:1]].expand(len(same), H)), ("rows of zero features differ", t)
    y2, grads2, dpost2 = run()
    assert torch.equal(y2, y) and torch.equal(grads2, grads) and torch.equal(dpost2, dpost1), "a second run gave other bits"


@pytest.mark.parametrize("H,K", sc.WIDTH_K)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_smallk_every_width_and_every_k_group(ops, dtype, H, K):
    """Nine rows at each width with K = 1, the K that open and close phase B's groups of four (4, 5, 8, 9, 16), and the
    largest K the backward's LDS admits at 768 and 1 024."""
    worst = Worst(f"smallk {DT_ID(dtype)} {K}->{H}")
    _check_case(ops, (sc.WIDTH_K_ROWS, K, H, dtype, "plain"), worst)
    worst.report()


def test_smallk_backward_tiles_blocks_and_every_finalize_loop(ops):
    """Row counts around the backward's 8-row tile, every workgroup count of the finalize's three loops (1 .. 5, 8, 9, 12, 13
    partial planes), exactly 256 tiles, and 257: workgroup 0 gets a second tile that holds one row."""
    worst = Worst(f"smallk f32 {sc.BWD_K}->{sc.BWD_H} rows {sc.BWD_ROWS[0]}..{sc.BWD_ROWS[-1]}")
    for rows in sc.BWD_ROWS:
        _check_case(ops, (rows, sc.BWD_K, sc.BWD_H, torch.float32, "plain"), worst)
    worst.report()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_smallk_past_the_forward_grid_cap(ops, dtype):
    """4 101 rows: the forward's 1 024 workgroups loop, wave 0 of workgroup 0 owns rows 0 and 4 096, the last group of four
    rows is short, and workgroup 0 of the backward owns three tiles."""
    worst = Worst(f"smallk {DT_ID(dtype)} {sc.CAP_K}->{sc.CAP_H} rows {sc.CAP_ROWS}")
    _check_case(ops, (sc.CAP_ROWS, sc.CAP_K, sc.CAP_H, dtype, "plain"), worst)
    worst.report()


@pytest.mark.parametrize("H,K", sc.OFFSET_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_smallk_projection_with_a_mean_far_above_its_spread(ops, dtype, H, K):
    """|mean z| ~ 1e3 times the spread of z: the gate grows with |z| through e_z, a two-pass variance stays inside and a
    one-pass mean(z^2) - mean^2 does not (host test)."""
    worst = Worst(f"smallk {DT_ID(dtype)} offset {K}->{H}")
    _check_case(ops, (sc.OFFSET_ROWS, K, H, dtype, "offset"), worst)
    worst.report()


def test_smallk_each_row_reaches_the_sums_once(ops):
    """2 049 rows of which five carry a gradient (the first and last of tiles 0, 1, 255 and the one row of tile 256): the
    other rows' dz is exactly zero, the sums have five terms, and a missing or doubled row lies outside their gates."""
    worst = Worst(f"smallk f32 sparse dy {sc.BWD_K}->{sc.BWD_H} rows {sc.SPARSE_ROWS}")
    _check_case(ops, (sc.SPARSE_ROWS, sc.BWD_K, sc.BWD_H, torch.float32, "sparse"), worst)
    worst.report()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_smallk_null_bias_post1_and_table_through_the_c_abi(ops, dtype):
    """bevbert_smallk_linear_layernorm_fwd with bias, post1, table and idx null, and ..._bwd with bias null, which the Python
    wrapper never passes: the references of the case with b = 0, post1 = 0 and a zero table, the same gates."""
    from vln_bevbert_amd import lib
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    params = (sc.WIDTH_K_ROWS, 7, 768, dtype, "nulls")
    c, r, k32 = sc.case(*params), sc.ref(*params), sc.kernel_f32(*params)
    rows, K, H = c["rows"], c["K"], c["H"]
    feat, W, gamma, beta = (c[k].to(DEV) for k in ("feat", "W", "gamma", "beta"))
    dy = c["dy"].to(dtype).to(DEV)
    ws = torch.empty(int(lib.load().bevbert_smallk_workspace_floats(rows, K, H)), device=DEV)

    def run():
        y = torch.empty(rows, H, dtype=dtype, device=DEV)
        mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        call("bevbert_smallk_linear_layernorm_fwd", ptr(feat), ptr(W), None, ptr(gamma), ptr(beta), None, None, None, ptr(y),
             ptr(mean), ptr(rstd), rows, K, H, sc.EPS, dtype_code(y), stream())
        sinks = {k: c["start"][k].to(DEV) for k in ("W", "b", "gamma", "beta")}
        call("bevbert_smallk_linear_layernorm_bwd", ptr(dy), ptr(feat), ptr(W), None, ptr(mean), ptr(rstd), ptr(gamma),
             ptr(sinks["W"]), ptr(sinks["b"]), ptr(sinks["gamma"]), ptr(sinks["beta"]), ptr(ws), rows, K, H, dtype_code(dy),
             stream())
        torch.cuda.synchronize()
        return y, sinks
    y, sinks = run()
    worst = Worst(f"smallk {DT_ID(dtype)} null pointers 7->768")
    worst.bound("y", y, r["y"], r["gate"]["y"], c["tag"], e32=k32["y_out"] - r["y"])
    for key in ("W", "b", "gamma", "beta"):
        q = GRADS[key]
        worst.bound(q, sinks[key], r[q], r["gate"][q], c["tag"], e32=k32[q] - r[q])
    y2, sinks2 = run()
    assert torch.equal(y2, y) and all(torch.equal(sinks2[k], sinks[k]) for k in sinks)
    worst.report()


# ----------------------------------------------------------------------------- embedding_grad_sliced
@pytest.mark.parametrize("H,per,rows,T", sc.SLICED_DIRECT)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_embedding_grad_sliced_partials_through_the_c_abi(ops, dtype, H, per, rows, T):
    """bevbert_embedding_grad_sliced directly: partials[slice][id] against the fp64 sum of that slice's rows of that id; a
    (slice, id) nobody names is exactly zero; nothing is written past the last slice."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    ids, d, _ = sc.sliced_case(H, rows, T, dtype)
    want, gate = sc.sliced_ref(ids, d, T, per)
    slices = want.shape[0]
    assert slices == -(-rows // per)
    ids_d, d_d = ids.to(DEV), d.to(DEV)
    outs = []
    for _ in range(2):
        part = torch.full((slices + 1, T, H), 3.0, device=DEV)
        call("bevbert_embedding_grad_sliced", ptr(ids_d), ptr(d_d), ptr(part), rows, H, T, per, dtype_code(d_d), stream())
        torch.cuda.synchronize()
        outs.append(part)
    worst = Worst(f"embedding_grad_sliced {DT_ID(dtype)} {rows}x{H} per {per} ids {T}")
    worst.bound("partials", outs[0][:slices], want, gate)
    assert bool((outs[0][slices] == 3.0).all()) and torch.equal(outs[0], outs[1])
    worst.report()


@pytest.mark.parametrize("T,rows,H", sc.SLICED_WRAPPER)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_embedding_grad_small_folds_its_slices_onto_the_start_value(ops, dtype, T, rows, H):
    """ops.embedding_grad_small: at (100, 2 700) the wrapper doubles its slice once; the fold adds to the sink's start value,
    a row nobody names keeps it bit for bit, and a second run gives the same bits."""
    ids, d, start = sc.sliced_case(H, rows, T, dtype)
    want, gate = sc.scatter_ref(ids, d, T, start)
    outs = []
    for _ in range(2):
        ops.RT.scratch.reset()
        sink = start.to(DEV)
        ops.embedding_grad_small(ids.to(DEV), d.to(DEV), sink, T)
        ops.WgradStream.flush_all()
        torch.cuda.synchronize()
        outs.append(sink)
    worst = Worst(f"embedding_grad_small {DT_ID(dtype)} {rows}x{H} ids {T}")
    worst.bound("d table", outs[0], want, gate)
    assert torch.equal(outs[0][-1].cpu(), start[-1]) and torch.equal(outs[0], outs[1])
    worst.report()
