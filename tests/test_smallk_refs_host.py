"""The fp64 references, the inputs and the gates of tests/test_gpu_smallk.py, checked without a GPU (tests/smallk_cases.py
holds them): every reference against torch's fp64 autograd composition to 1e-12 of the result's scale; torch's fp32
composition and the numpy fp32 restatement of the kernels' own order within half of every gate on every case; the edges each
case is there for; that a one-pass variance falls outside the y gate of the ``offset`` cases; and that the support
predicate's LDS bound is the backward entry's own."""
import ctypes

import pytest
import torch

from tests import smallk_cases as sc
from tests.smallk_cases import DT_ID, DTYPES

TIGHT = 1e-12
HALF = 0.5
QUANTITIES = ("y", "dz", "dW", "db", "dgamma", "dbeta")
CASE_ID = lambda p: f"{DT_ID(p[3])}-{p[4]}-{p[0]}x{p[1]}-{p[2]}"


def _close(a, b):
    a, b = a.double(), b.double()
    return float((a - b).detach().abs().max()) <= TIGHT * max(1.0, float(b.detach().abs().max()))


def _fraction(got, want, gate):
    err = (got.double() - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / gate.clamp_min(1e-300)).max())


@pytest.mark.parametrize("params", sc.all_cases(), ids=CASE_ID)
def test_references_equal_torch_fp64_and_fp32_arithmetic_stays_within_half_of_every_gate(params):
    rows, K, H, dtype, kind = params
    c, r = sc.case(*params), sc.ref(*params)
    t64 = sc.torch_composition(c, torch.float64)
    for k in QUANTITIES + ("dtable",):
        assert _close(r[k], t64[k]), k
    assert torch.equal(t64["dpost1"], c["dy"].double())
    t32, k32 = sc.torch_composition(c, torch.float32), sc.kernel_f32(*params)
    frac = {}
    for k in QUANTITIES:                                  # y: the fp32 value against the gate without its bf16 term
        gate = r["gate"]["y32" if k == "y" else k]
        frac[k] = (_fraction(t32[k], r[k], gate), _fraction(k32[k], r[k], gate))
    frac["y as first stated"] = (_fraction(t32["y"], r["y"], r["gate"]["y_stated"]), _fraction(k32["y"], r["y"], r["gate"]["y_stated"]))
    frac["dtable"] = (_fraction(t32["dtable"], r["dtable"], r["gate"]["dtable"]), float("nan"))
    print(f"smallk-kernel-errors: host {c['tag']:<28} largest error / gate (torch fp32, kernel order fp32): " +
          "  ".join(f"{k} {a:.3f} {b:.3f}" for k, (a, b) in frac.items()))
    assert all(a <= HALF and not b > HALF for k, (a, b) in frac.items() if k != "y as first stated"), frac
    assert _fraction(k32["y_out"], r["y"], r["gate"]["y"]) <= 1.0          # one more rounding: 2^-8 |y| at the most


@pytest.mark.parametrize("params", sc.all_cases(), ids=CASE_ID)
def test_cases_hold_the_edges_they_are_there_for(params):
    rows, K, H, dtype, kind = params
    c, r = sc.case(*params), sc.ref(*params)
    idx, feat, dy = c["idx"], c["feat"], c["dy"]
    assert idx[0] == 0 and idx[-1] == 0 and int(idx.max()) < sc.TABLE_ROWS - 1 and int(idx.min()) >= 0
    assert torch.equal(r["dtable"][-1], c["start"]["table"][-1].double()) and bool((r["gate"]["dtable"][-1] == 0).all())
    assert all(bool((v != 0).all()) for v in c["start"].values())
    for k in ("post1", "dy", "table"):                    # values of the compute dtype, "the values the kernel gets"
        assert torch.equal(c[k].to(dtype).to(c[k].dtype), c[k])
    zr = c["zero_rows"]
    assert torch.equal(zr, torch.arange(rows) % 3 == 1) and bool((feat[zr] == 0).all())
    if rows > 1:
        # z = b exactly on those rows: one LayerNorm part, bit for bit, and nothing for dW
        assert bool((r["z"][zr] == c["b"].double()).all()) and bool((r["ln"][zr] == r["ln"][1]).all())
        assert torch.equal(c["post1"][zr], c["post1"][1:2].expand(int(zr.sum()), H))
        keep = ~zr
        assert _close(r["dW"], c["start"]["W"].double() + r["dz"][keep].t() @ feat[keep].double())
    hot = feat[c["hot"]]
    assert int((hot != 0).sum()) == 1 and float(hot.sum()) == 1.0
    assert bool((dy.reshape(-1)[::7] == 0).all()) and bool((dy != 0).any())
    if kind == "offset":
        ratio = r["mean"].abs() * r["rstd"]
        plain = ~zr
        plain[c["hot"]] = False
        assert float(ratio[plain].min()) > 50 and bool((feat[plain, 0] == 1000).all())
    if kind == "sparse":
        live = torch.zeros(rows, dtype=torch.bool)
        live[list(sc.SPARSE_DY_ROWS)] = True
        assert bool((dy[~live] == 0).all()) and bool((r["dz"][~live] == 0).all()) and bool((r["gate"]["dz"][~live] == 0).all())
        assert bool((dy[live] != 0).any(1).all())
        # five terms and the start value: one row missing or doubled lies outside the gates
        for k, term in (("dbeta", dy.double()), ("db", r["dz"])):
            for row in sc.SPARSE_DY_ROWS:
                off = (term[row].abs() > r["gate"][k])[term[row] != 0]
                assert float(off.double().mean()) > 0.95, (k, row)
    if kind == "nulls":
        assert not bool(c["b"].any()) and not bool(c["post1"].any()) and not bool(c["table"].any())


def test_shapes_reach_the_branches_they_name():
    assert sc.max_k(768) == 13 and sc.max_k(1024) == 7 and sc.max_k(256) == 16 and sc.max_k(512) == 16
    assert {(H, K) for H, K in sc.WIDTH_K if K == sc.max_k(H)} == {(256, 16), (512, 16), (768, 13), (1024, 7)}
    assert {-(-K // 4) for _, K in sc.WIDTH_K} == {1, 2, 3, 4} and {4, 5, 8, 9} <= {K for _, K in sc.WIDTH_K}
    nbs = [sc.bwd_blocks(r) for r in sc.BWD_ROWS]
    assert nbs == [1, 1, 1, 2, 3, 4, 5, 8, 9, 12, 13, 256, 256]
    # the finalize, per wave w of a launch over nb workgroups: (pairs summed while b + 4 < nb, singles after them)
    loops = lambda nb, w: (len(range(w, nb - 4, 8)), len(range(w + 8 * len(range(w, nb - 4, 8)), nb, 4)))
    assert {loops(nb, w) for nb in nbs for w in range(4)} >= {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (32, 0)}
    assert sc.BWD_ROWS[-2] == 256 * 8 and sc.BWD_ROWS[-1] == 256 * 8 + 1
    assert sc.CAP_ROWS > 1024 * 4 and sc.CAP_ROWS % 4 and -(-sc.CAP_ROWS // 8) > 2 * 256
    assert sc.sum_depth(4101) == 17 + 64 + 6 and sc.sum_depth(1) == 1 + 0.25 + 6


@pytest.mark.parametrize("H,K", sc.OFFSET_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_a_one_pass_variance_falls_outside_the_y_gate_of_the_offset_cases(dtype, H, K):
    """mean(z^2) - mean^2 in fp32 loses |mean z|^2 / var ~ 1e4 .. 1e6 ulps of the variance; the two-pass form of the same
    restatement stays inside (the test above).  Otherwise the ``offset`` cases would not test what they claim."""
    params = (sc.OFFSET_ROWS, K, H, dtype, "offset")
    r = sc.ref(*params)
    one = sc.kernel_f32(*params, one_pass=True, sums=False)
    bad = (one["y"] - r["y"]).abs() > r["gate"]["y"]
    frac = _fraction(one["y"], r["y"], r["gate"]["y"])
    print(f"smallk-kernel-errors: host {DT_ID(dtype)} offset {K}->{H} one-pass variance: y error / gate {frac:.1f}, {int(bad.sum())} elements outside")
    assert frac > 2.0 and int(bad.any(1).sum()) >= sc.OFFSET_ROWS // 3


# ----------------------------------------------------------------------------- embedding_grad_sliced
def test_sliced_cases_reach_their_branches_and_their_references_fold_to_index_add():
    threads = lambda H: (H // 4 + 63) // 64 * 64 if H // 4 < 256 else 256
    assert {threads(H) for H, *_ in sc.SLICED_DIRECT} == {64, 192, 256}
    assert any(H > 1024 and H % 4 == 0 for H, *_ in sc.SLICED_DIRECT)                       # the column loop runs twice
    assert any(per % 4 and rows % per and rows > per for _, per, rows, _ in sc.SLICED_DIRECT)   # r + j < r1; a short last slice
    assert {per for _, per, _, _ in sc.SLICED_DIRECT} == {1, 3, 64} and {t for *_, t in sc.SLICED_DIRECT} == {1, 2, 5}
    for H, per, rows, T in sc.SLICED_DIRECT:
        ids, d, _ = sc.sliced_case(H, rows, T, torch.float32)
        want, gate = sc.sliced_ref(ids, d, T, per)
        assert _close(want.sum(0), torch.zeros(T, H, dtype=torch.float64).index_add_(0, ids, d.double()))
        assert ids[0] == 0 and ids[-1] == 0 and bool((d.reshape(-1)[::7] == 0).all())
        if T > 1:
            assert not bool(want[:, T - 1].any()) and not bool(gate[:, T - 1].any())
    (T, rows, H), _ = sc.SLICED_WRAPPER
    assert sc.wrapper_slice_rows(rows, T) == 128 and sc.wrapper_slice_rows(77, 3) == 64 and -(-rows // 64) * T > 4096


# ----------------------------------------------------------------------------- the predicate's LDS bound
def test_support_predicate_and_backward_entry_agree_on_the_lds_bound():
    """ops.smallk_linear_layernorm_plus_supported restates the backward's LDS need; the forward entry needs less and accepts
    pairs the backward refuses (768, 14).  Null pointers where the entry does not look, rows = 1, a dtype without a kernel:
    past the LDS check the entry answers "dtype 2 unsupported", and nothing is launched either way."""
    from vln_bevbert_amd import lib, ops
    from vln_bevbert_amd.arena import ParamArena
    l = lib.load()
    buf = (ctypes.c_uint8 * 64)()
    N, p = None, ctypes.addressof(buf)
    bwd = lambda H, K: (l.bevbert_smallk_linear_layernorm_bwd(N, N, N, N, p, p, N, N, N, N, N, p, 1, K, H, 2, N),
                        l.bevbert_last_error().decode())

    class _OnDevice:                                   # the predicate asks its feature tensor one thing
        is_cuda = True

    def admitted(H, K):
        class M(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.lin, self.ln = torch.nn.Linear(K, H), torch.nn.LayerNorm(H)
        m = M()
        ParamArena(m, "cpu", torch.float32)
        return bool(ops.smallk_linear_layernorm_plus_supported(_OnDevice(), m.lin, m.ln, torch.zeros(1, H)))
    for H in (256, 512, 768, 1024):
        K = max(k for k in range(1, 17) if admitted(H, k))
        assert K == sc.max_k(H), (H, K)
        rc, msg = bwd(H, K)
        assert rc == -3 and "smallk_linear_layernorm_bwd: dtype 2 unsupported" in msg, (H, K, rc, msg)
        if K < 16:
            rc, msg = bwd(H, K + 1)
            assert rc == -1 and f"smallk_linear_layernorm_bwd: K={K + 1} x H={H} needs more than 64 KB of LDS" in msg, (H, K, rc, msg)
            assert not admitted(H, K + 1)
            rc = l.bevbert_smallk_linear_layernorm_fwd(*[N] * 11, 1, K + 1, H, 1e-12, 2, N)
            assert rc == -3 and "dtype 2 unsupported" in l.bevbert_last_error().decode()
