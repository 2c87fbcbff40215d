"""CPU side of tests/test_gpu_attention_edges.py: the closed-form fp64 gradients of tests/attn_cases.py against autograd, what
a bf16 and an fp32 restatement need of the gates (C16, C32), the proof that the gates see one wrong key at a tile edge, and
the case table against the dispatch plan.  Run with -s for the figures."""
import pytest
import torch

from tests import attn_cases as ac
from tests.test_host_logic import attn_plan
from vln_bevbert_amd import lib

KERNELS = ("attn_short_fwd", "attn_small_fwd", "attn_fwd4", "attn_fwd2", "attn_mfma_fwd", "attn_f32_fwd", "attn_simple_fwd",
           "attn_short_bwd", "attn_small_bwd2", "attn_small_bwd", "attn_bwd3", "attn_bwd2", "attn_mfma_bwd1", "attn_mfma_bwd",
           "attn_f32_bwd", "attn_simple_bwd")


def _host_keep(c, seed):
    if c.p == 0:
        return None
    g = torch.Generator().manual_seed(977 * seed + c.Lq + c.Lk)
    return torch.rand(c.B, c.nh, c.Lq, c.Lk, generator=g) >= c.p


def _cpu_subset():
    """The rows of CASES a CPU gets through in seconds: each axis up to 130, and 130 x 449; one row per distinct
    (Lq, Lk, mask, bias, p)."""
    seen, out = set(), []
    for c in ac.CASES:
        key = (c.Lq, c.Lk, c.mask, c.bias, c.p)
        if key in seen or not ((c.Lq <= 130 and c.Lk <= 130) or (c.Lq, c.Lk) == (130, 449)):
            continue
        seen.add(key)
        out.append(c)
    return out


@pytest.mark.parametrize("Lq,Lk,mask,bias,p", [(5, 7, None, False, 0.0), (9, 17, "holes", True, 0.25), (17, 33, "holes_inf", True, 0.1)])
def test_closed_form_gradients_equal_autograd(Lq, Lk, mask, bias, p):
    B, nh = 2, 2
    q, k, v, do, km, b = ac.make_inputs(B, nh, Lq, Lk, torch.float64, mask, bias, seed=3)
    keep = torch.rand(B, nh, Lq, Lk, generator=torch.Generator().manual_seed(5)) >= p if p else None
    ref = ac.reference(q, k, v, do, ac.SCALE, km, b, keep, p)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    # per-head bias so that autograd's gradient is the per-head dbias
    ba = b.double()[:, None].expand(B, nh, Lq, Lk).clone().requires_grad_(True) if bias else None
    S = ac.SCALE * (ac._heads(qa) @ ac._heads(ka).transpose(-1, -2))
    if km is not None:
        S = S + km.double()[:, None, None, :]
    if ba is not None:
        S = S + ba
    P = torch.softmax(S, -1)
    if keep is not None:
        P = torch.where(keep, P / (1 - p), torch.zeros_like(P))
    o = ac._rows(P @ ac._heads(va))
    o.backward(do)
    rel = lambda a, w: float((a - w).abs().max() / w.abs().max().clamp_min(1e-300))
    assert rel(ref["o"], o.detach()) < 1e-12
    assert rel(ref["lse"], torch.logsumexp(S.detach(), -1)) < 1e-12
    for name, grad in (("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)) + ((("dbias", ba.grad),) if bias else ()):
        assert rel(ref[name], grad) < 1e-12, (name, rel(ref[name], grad))
    # every bound tensor dominates the magnitude of what it bounds
    for name in ("o", "dq", "dk", "dv", "dbias"):
        assert bool((ref["b_" + name] * (1 + 1e-12) >= ref[name].abs()).all()), name


def test_restatements_stay_inside_the_gates_and_define_c32():
    """emulate_bf16 needs at most C16 / 4 units of every gate; torch's fp32 composition needs C32 / 4 at the most (that is what
    C32 is) and its lse stays inside 2^-18 b_lse with the same margin of four."""
    worst16, worst32 = {}, {}
    for n, c in enumerate(_cpu_subset()):
        q, k, v, do, km, b = ac.make_inputs(c.B, c.nh, c.Lq, c.Lk, torch.bfloat16, c.mask, c.bias, seed=n)
        keep = _host_keep(c, n)
        ref = ac.reference(q, k, v, do, ac.SCALE, km, b, keep, c.p)
        for kind, fn, worst in (("bf16", ac.emulate_bf16, worst16), ("f32", ac.compose_f32, worst32)):
            got = fn(q, k, v, do, ac.SCALE, km, b, keep, c.p)
            assert all(bool(torch.isfinite(t).all()) for t in got.values())
            for name, u in ac.units(got, ref, kind).items():
                if u > worst.get(name, (0.0, ""))[0]:
                    worst[name] = (u, f"{c.Lq}x{c.Lk} {c.mask} bias={c.bias} p={c.p}")
    for tag, worst in (("emulate_bf16 (units of 2^-8 b_x)", worst16), ("torch fp32 (units of 2^-24 b_x)", worst32)):
        for name, (u, where) in worst.items():
            print(f"attn-ref-host: {tag:<34} {name:<6} {u:.3f}  at {where}")
    for name in ("o", "dq", "dk", "dv", "dbias"):
        assert worst16[name][0] <= ac.C16 / 4, (name, worst16[name])
        assert worst32[name][0] <= ac.C32 / 4, (name, worst32[name])
    assert worst16["lse"][0] <= 0.25 and worst32["lse"][0] <= 0.25, (worst16["lse"], worst32["lse"])
    # C32 is four times what the fp32 composition needs, not a blanket factor: it may not sit more than 2 x above that
    assert ac.C32 <= 8 * max(worst32[name][0] for name in ("o", "dq", "dk", "dv", "dbias"))


def test_one_wrong_key_at_a_tile_edge_leaves_the_gates():
    """For every boundary key j of the CPU subset's masked dropout shapes, each of the four mutations moves at least one
    element of o and of at least two gradients beyond twice its gate -- the gate a correct kernel is held to, so the GPU test
    cannot pass a kernel that drops, mis-masks, mis-drops or misplaces one key.  So that no mutation is a no-op, sample 0 is
    pinned to keep key j and mask key j + 1, and sample 1 to leave both unmasked with the keep bit of j set and that of j + 1
    clear in every row (under the device's own mask the two bits differ in 18 % of the rows, and a wrong bit shows in those).
    Shapes with fewer than 16 queries are left out: a single key has to carry a weight of the order of the gate in some
    row, and a handful of rows may not give it one."""
    shapes = sorted({(c.Lq, c.Lk) for c in _cpu_subset() if c.Lq >= 16 and c.Lk >= 2})
    assert (130, 449) in shapes and len(shapes) >= 12
    p, least, failures = 0.1, {}, []
    for n, (Lq, Lk) in enumerate(shapes):
        c = ac._c(Lq, Lk, "holes", p, "mfma_fwd", "mfma_bwd")
        q, k, v, do, km0, _ = ac.make_inputs(c.B, c.nh, Lq, Lk, torch.bfloat16, "holes", False, seed=n)
        keep0 = _host_keep(c, n)
        for j in ac.boundary_indices(Lk):
            km = km0.clone()
            km[:, j], km[0, j + 1], km[1, j + 1] = 0.0, -10000.0, 0.0
            keep = keep0.clone()
            keep[1, :, :, j], keep[1, :, :, j + 1] = True, False
            ref = ac.reference(q, k, v, do, ac.SCALE, km, None, keep, p)
            gate = ac.gates(ref, "bf16")
            for kind in ac.MUTATIONS:
                mut = ac.mutate(kind, j, q, k, v, do, ac.SCALE, km, None, keep, p)
                over = {name: float(((mut[name] - ref[name]).abs() / gate[name].clamp_min(1e-300)).max())
                        for name in ("o", "dq", "dk", "dv")}
                grads = sorted(over[name] for name in ("dq", "dk", "dv"))
                if not (over["o"] > 2 and grads[1] > 2):
                    failures.append((kind, Lq, Lk, j, {k_: round(v_, 2) for k_, v_ in over.items()}))
                least[kind] = min(least.get(kind, float("inf")), over["o"], grads[1])
    assert not failures, failures
    for kind, x in least.items():
        print(f"attn-ref-host: mutation {kind:<7} least (o, second gradient) over its gate: {x:.1f} x")


def _rows_of(name):
    return [c for c in ac.CASES if name in (c.fwd, c.bwd)]


def test_case_table_is_what_the_plan_says_and_covers_every_kernel_and_length(monkeypatch):
    l = lib.load()
    assert set(ac.ATTN_KNOBS) >= {k for c in ac.CASES for k in c.knobs}
    for c in ac.CASES:
        assert attn_plan(l, ac.plan_row(c), 256, monkeypatch) == (c.fwd, c.bwd), ac.case_id(c)
    assert len({ac.case_id(c) for c in ac.CASES}) == len(ac.CASES)
    assert {c.fwd for c in ac.CASES} | {c.bwd for c in ac.CASES} == set(KERNELS) == set(ac.REQUIRED)
    for name, need in ac.REQUIRED.items():
        rows = _rows_of(name)
        for axis in ("Lq", "Lk"):
            assert set(need.get(axis, ())) <= {getattr(c, axis) for c in rows}, (name, axis)
        assert set(need.get("bias_Lk", ())) <= {c.Lk for c in rows if c.bias}, name
        assert set(need.get("pairs", ())) <= {(c.Lq, c.Lk) for c in rows}, name
        assert set(need.get("wgs", ())) <= {c.knobs.get("BEVBERT_FWD4_WGS") for c in rows}, name
        assert set(need.get("impl3", ())) <= {(c.Lq, c.Lk) for c in rows if c.impl == 3}, name
        if need.get("both_dtypes"):
            for dtype in ("f32", "bf16"):
                for axis in ("Lq", "Lk"):
                    assert set(need[axis]) <= {getattr(c, axis) for c in rows if c.dtype == dtype}, (name, dtype, axis)
        assert {c.mask for c in rows} == set(ac.MASKS), name
        assert {c.p for c in rows} == {0.0, 0.1}, name
        # the keep mask is indexed with Lk rounded up to even
        assert any(c.p > 0 and c.Lk % 2 for c in rows), name
    assert all(c.B == 2 and c.nh == 2 for c in ac.CASES)
