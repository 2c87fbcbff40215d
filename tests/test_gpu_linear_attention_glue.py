"""The autograd glue between the kernels and the model, one op at a time against an fp64 composition of the same op from
the same rounded inputs: ``linear`` / ``linear_res`` (the residual tap folded into the input-gradient GEMM), the packed
Q|K|V and K|V projections, attention on packed and strided operands through every backward kernel of the default dispatch,
and ``hoisted_kv`` by every route a gradient can take to its per-layer views.

Tolerances are the single-op ones of tests/test_gpu_kernels.py: GEMM-backed values rel_err < 1e-4 (fp32) / 1e-2 (bf16) as in
test_lt_gemm_linear_fwd_dgrad_wgrad; attention 1e-4 / 1e-2 of max(1, |ref|max) forward and rel_err < 1e-3 / 2.5e-2 backward
as in test_attention_fwd_bwd.  Chains are checked stage by stage (the captured dK|dV buffer against the attention
reference, then dx / dW / db against fp64 GEMMs OF THAT BUFFER), so no bound is compounded.
"""
import pytest
import torch

from tests.attn_cases import ATTN_KNOBS
from tests.test_gpu_kernels import _attn_ref, _make_attn_inputs, ops, rel_err  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, NH = 768, 12
BF16, F32 = torch.bfloat16, torch.float32


def _gemm_tol(dtype):
    return 1e-4 if dtype == F32 else 1e-2


def _randn(g, *shape, scale=1.0, dtype=F32):
    return (torch.randn(*shape, generator=g) * scale).to(DEV, dtype)


def _close(name, got, ref, tol):
    err = rel_err(got, ref)
    print(f"{name}: rel_err {err:.3e} (bound {tol:.1e})")
    assert bool(torch.isfinite(got.float()).all()) and err < tol, (name, err, tol)


# ----------------------------------------------------------------------------- 1. linear / linear_res
def _make_linear(ops, N, K, dtype, in_arena, seed):
    """nn.Linear(K, N) in a ParamArena (fp32 masters, ``dtype`` compute copy) or as plain ``dtype`` parameters, and the
    fp64 images of the values the GEMMs read."""
    from vln_bevbert_amd.arena import ParamArena
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(K, N)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(N, generator=g))
    arena = ParamArena(lin, DEV, dtype) if in_arena else None
    if not in_arena:
        lin.to(DEV, dtype)
    wd, bd = ops._compute(lin.weight).detach().double(), ops._compute(lin.bias).detach().double()
    return lin, arena, wd, bd


def _param_grads_of(lin, arena):
    if arena is None:
        return lin.weight.grad, lin.bias.grad
    arena.sync()
    torch.cuda.synchronize()
    return lin.weight.main_grad.clone(), lin.bias.main_grad.clone()


ROWS = (2, 23)                                       # 46 rows: no multiple of any GEMM tile
# (out, in): square, FFN, a 1-wide head, N % 4 != 0 (bevbert_colsum_any).  With K = 768 every N * K is a multiple of 4: 766 -> 3
# (N * K = 2298) takes the ``sink.add_`` branch of _wgrad_into.  Its split-K arm (part.sum(0)) needs >= 1280 rows and stays
# uncovered here.
LINEAR_SHAPES = [(768, 768), (3072, 768), (1, 768), (6, 768), (3, 766)]


@pytest.mark.parametrize("in_arena", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("N,K", LINEAR_SHAPES)
def test_linear_fwd_and_every_gradient(ops, N, K, dtype, in_arena):
    """ops.linear: y, dx, dW, db against fp64 -- into the arena (split-K / colsum / colsum_any routes) or returned to
    autograd for plain parameters."""
    lin, arena, wd, bd = _make_linear(ops, N, K, dtype, in_arena, N + K)
    g = torch.Generator().manual_seed(1)
    x = _randn(g, *ROWS, K, dtype=dtype).requires_grad_(True)
    dy = _randn(g, *ROWS, N, dtype=dtype)
    y = ops.linear(x, lin.weight, lin.bias)
    tol = _gemm_tol(dtype)
    assert y.dtype == dtype and y.shape == ROWS + (N,)
    _close("y", y.detach(), x.detach().double() @ wd.t() + bd, tol)
    y.backward(dy)
    gw, gb = _param_grads_of(lin, arena)
    x2, dy2 = x.detach().double().reshape(-1, K), dy.double().reshape(-1, N)
    _close("dx", x.grad, dy.double() @ wd, tol)
    _close("dW", gw, dy2.t() @ x2, tol)
    _close("db", gb, dy2.sum(0), tol)
    if in_arena:
        assert arena._touched == {"weight", "bias"}


@pytest.mark.parametrize("in_arena", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("pattern", ["both", "tap", "y"])
@pytest.mark.parametrize("N,K", [(768, 768), (3072, 768)])
def test_linear_res_folds_the_tap_gradient_into_the_input_gradient_gemm(ops, N, K, pattern, dtype, in_arena):
    """ops.linear_res: (y, tap).  Both consumed: dx = dy W + d_res (the beta = 1 addend of bevbert_gemm_run_add); only the
    tap: dx is d_res bit for bit and the parameters receive nothing; only y: dx = dy W.  d_res is 8x the size of dy W, so a
    dropped or doubled addend is two orders of magnitude outside the bound."""
    lin, arena, wd, bd = _make_linear(ops, N, K, dtype, in_arena, N + K + 1)
    g = torch.Generator().manual_seed(2)
    x = _randn(g, *ROWS, K, dtype=dtype).requires_grad_(True)
    dy = _randn(g, *ROWS, N, dtype=dtype)
    dres = _randn(g, *ROWS, K, scale=8.0, dtype=dtype)
    y, tap = ops.linear_res(x, lin.weight, lin.bias)
    tol = _gemm_tol(dtype)
    assert tap.data_ptr() == x.data_ptr() and tap.shape == x.shape
    _close("y", y.detach(), x.detach().double() @ wd.t() + bd, tol)
    if pattern == "both":
        torch.autograd.backward([y, tap], [dy, dres])
    elif pattern == "tap":
        tap.backward(dres)
    else:
        y.backward(dy)
    gw, gb = _param_grads_of(lin, arena)
    if pattern == "tap":
        assert torch.equal(x.grad, dres)
        if in_arena:
            assert not arena._touched and not bool(arena.grads.any())
        else:
            assert gw is None and gb is None
        return
    prod = dy.double() @ wd
    _close("dx", x.grad, prod + dres.double() if pattern == "both" else prod, tol)
    x2, dy2 = x.detach().double().reshape(-1, K), dy.double().reshape(-1, N)
    _close("dW", gw, dy2.t() @ x2, tol)
    _close("db", gb, dy2.sum(0), tol)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_linear_dgrad_addend_of_any_layout_and_dtype(ops, dtype):
    """_linear_dgrad(dy, w, add=...): the addend is read as dy's dtype and dense, whatever it came as."""
    N, K, M = 3072, 768, ROWS[0] * ROWS[1]
    g = torch.Generator().manual_seed(3)
    w = _randn(g, N, K, scale=0.05, dtype=dtype)
    dy = _randn(g, M, N, dtype=dtype)
    prod = dy.double() @ w.double()
    other = BF16 if dtype == F32 else F32
    wide = _randn(g, M, K + 64, scale=8.0, dtype=dtype)
    adds = {"column slice": wide[:, 32:32 + K], "transposed": _randn(g, K, M, scale=8.0, dtype=dtype).t(),
            "other dtype": _randn(g, M, K, scale=8.0, dtype=other),
            "3-d, other dtype, strided": _randn(g, ROWS[0], ROWS[1], K + 8, scale=8.0, dtype=other)[..., 8:]}
    for name, add in adds.items():
        assert name == "other dtype" or not add.is_contiguous()
        keep = add.clone()
        dx = ops._linear_dgrad(dy, w, add=add)
        assert dx.dtype == dtype and dx.shape == (M, K)
        _close(name, dx, prod + add.to(dtype).double().reshape(M, K), _gemm_tol(dtype))
        assert torch.equal(add, keep)                       # the addend is an input, not the destination


# ----------------------------------------------------------------------------- 2. linear_packed / linear_packed_res
class _Proj(torch.nn.Module):
    def __init__(self, names):
        super().__init__()
        for n in names:
            setattr(self, n, torch.nn.Linear(H, H))


def _make_packed(ops, names, dtype, seed):
    """The members' parameters laid out back to back in an arena and packed as BertSelfAttention._after_arena does."""
    from vln_bevbert_amd.arena import ParamArena
    torch.manual_seed(seed)
    m = _Proj(names)
    with torch.no_grad():
        for n in names:
            getattr(m, n).bias.normal_()
    wn, bn = [f"{n}.weight" for n in names], [f"{n}.bias" for n in names]
    arena = ParamArena(m, DEV, dtype, groups=[wn, bn])
    wc, wg = arena.packed(wn, (len(names) * H, H))
    bc, bg = arena.packed(bn, (len(names) * H,))
    pw = ops._PackedParam([getattr(m, n).weight for n in names], wc, wg)
    pb = ops._PackedParam([getattr(m, n).bias for n in names], bc, bg)
    return m, arena, pw, pb, wn + bn


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("names,res", [(("query", "key", "value"), False), (("query", "key", "value"), True),
                                       (("key", "value"), False), (("key", "value"), True)])
def test_linear_packed_members_against_their_own_linears(ops, names, res, dtype):
    """ops.linear_packed / linear_packed_res: one GEMM for Q|K|V (K|V); forward against the separate fp64 linears; after
    arena.sync() each member's main_grad holds prefill + its own dW / db (accumulate semantics, from a non-zero prefill),
    every member is marked touched, dx carries the tap gradient, and a second run leaves the same bits."""
    m, arena, pw, pb, pnames = _make_packed(ops, names, dtype, 5 + len(names))
    g = torch.Generator().manual_seed(6)
    n = len(names)
    x0 = _randn(g, *ROWS, H, dtype=dtype)
    dy = _randn(g, *ROWS, n * H, dtype=dtype)
    dres = _randn(g, *ROWS, H, scale=8.0, dtype=dtype)
    prefill = _randn(g, arena.grads.numel())
    tol = _gemm_tol(dtype)

    def run():
        arena.grads.copy_(prefill)
        x = x0.clone().requires_grad_(True)
        if res:
            y, tap = ops.linear_packed_res(x, pw, pb)
            assert tap.data_ptr() == x.data_ptr()
            torch.autograd.backward([y, tap], [dy, dres])
        else:
            y = ops.linear_packed(x, pw, pb)
            y.backward(dy)
        arena.sync()
        torch.cuda.synchronize()
        return y.detach(), x.grad, arena.grads.clone()

    y, dx, grads = run()
    assert set(pnames) <= arena._touched, sorted(set(pnames) - arena._touched)
    xd, x2 = x0.double(), x0.double().reshape(-1, H)
    dx_ref = dres.double() if res else torch.zeros_like(xd)
    for i, name in enumerate(names):
        lin = getattr(m, name)
        wd, bd = ops._compute(lin.weight).detach().double(), ops._compute(lin.bias).detach().double()
        _close(f"y[{name}]", y[..., i * H:(i + 1) * H], xd @ wd.t() + bd, tol)
        dyi = dy[..., i * H:(i + 1) * H].double()
        dx_ref = dx_ref + dyi @ wd
        for kind, p, ref in (("weight", lin.weight, dyi.reshape(-1, H).t() @ x2), ("bias", lin.bias, dyi.reshape(-1, H).sum(0))):
            o, k = arena.slices[f"{name}.{kind}"]
            assert p.main_grad.data_ptr() == arena.grads[o:o + k].data_ptr()
            _close(f"d {name}.{kind}", grads[o:o + k].view(p.shape), prefill[o:o + k].view(p.shape).double() + ref, tol)
    _close("dx", dx, dx_ref, tol)
    y2, dx2, grads2 = run()
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(grads, grads2)
    if res:                     # only the tap consumed: dx is the tap's gradient bit for bit, the arena is left alone
        arena.grads.copy_(prefill)
        x = x0.clone().requires_grad_(True)
        ops.linear_packed_res(x, pw, pb)[1].backward(dres)
        arena.sync()
        torch.cuda.synchronize()
        assert torch.equal(x.grad, dres) and torch.equal(arena.grads, prefill)


# ----------------------------------------------------------------------------- 3. packed / strided attention operands
# One row per backward kernel of the default dispatch (attn_plan_bwd, capi.hip), the smallest shapes bevbert_attn_plan sends
# there at B = 2: (cross Lq, cross Lk, self L, graph bias, dtype, impl, dropout p, knobs, forward kernel, backward kernel).
# The kernel names are those of the cross-shaped forms; the self-shaped form asserts the backward kernel and whatever
# forward the plan names for L x L.  attn_small_bwd2 is not in the table: every shape it supports (Lq, Lk <= 96, no bias) goes
# to attn_short_bwd under the default knobs.
ATTN_GLUE_CASES = {
    "short":       (23, 17, 17, False, BF16, 0, 0.1, {}, "attn_short_fwd", "attn_short_bwd"),
    "bias_bwd1":   (23, 23, 23, True, BF16, 0, 0.1, {}, "attn_mfma_fwd", "attn_mfma_bwd1"),      # gmap self-attention
    "short_bwd1":  (100, 40, 100, False, BF16, 0, 0.1, {}, "attn_short_fwd", "attn_mfma_bwd1"),    # BEV <- text
    "bwd3":        (70, 261, 261, False, BF16, 0, 0.1, {}, "attn_fwd2", "attn_bwd3"),
    "bwd2":        (70, 261, 261, False, BF16, 0, 0.1, {"BEVBERT_ATTN_BWD3": "0"}, "attn_fwd2", "attn_bwd2"),
    "split_long":  (70, 460, 460, False, BF16, 0, 0.1, {}, "attn_fwd2", "attn_mfma_bwd"),          # keys beyond 448
    "split_impl3": (23, 17, 17, False, BF16, 3, 0.1, {}, "attn_short_fwd", "attn_mfma_bwd"),
    "f32":         (23, 17, 17, False, F32, 0, 0.0, {}, "attn_f32_fwd", "attn_f32_bwd"),
    "f32_bias":    (23, 23, 23, True, F32, 0, 0.0, {}, "attn_f32_fwd", "attn_f32_bwd"),
    "simple":      (23, 17, 17, False, BF16, 1, 0.1, {}, "attn_simple_fwd", "attn_simple_bwd"),
}
ATTN_SEED = 777
SENTINEL = 7.0


def _set_knobs(monkeypatch, env):
    for name in ATTN_KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _planned(ops, B, Lq, Lk, dtype, impl, wb, p):
    """(forward, backward) kernel of the call _Attention makes for this shape, under the knobs the environment holds now."""
    from vln_bevbert_amd import lib
    has_bits = int(p > 0 and dtype == BF16 and impl != 1)            # ops_attention.py: when a keep-bit workspace is passed
    code = lib.BF16 if dtype == BF16 else lib.F32
    return tuple(lib.load().bevbert_attn_plan(B, NH, Lq, Lk, code, impl, 1, int(wb), p, has_bits, 0, int(wb), 0, backward).decode()
                 for backward in (0, 1))


def _traced(ops, fn):
    """Run ``fn`` with the call trace armed (the backward runs on autograd's thread: the trace reads the path there)."""
    ops.RT.trace, ops.RT.paths = {}, {}
    try:
        out = fn()
        torch.cuda.synchronize()
        paths = tuple(sorted(k.split(" -> ")[1] for k in ops.RT.paths))
    finally:
        ops.RT.trace, ops.RT.paths = None, {}
    return out, paths


@pytest.fixture(scope="module")
def glue_refs():
    """Per-case references of this module (filled by _attn_glue_reference), released with the module."""
    cache = {}
    yield cache
    cache.clear()


def _attn_glue_reference(cache, ops, case, is_self):
    """Inputs of one case, the same call on contiguous operands through ops.attention (under the case's own knobs, set
    here) and the fp64 reference under the exported dropout mask; computed once, shared by the forms, never modified."""
    if (case, is_self) not in cache:
        with pytest.MonkeyPatch.context() as mp:
            _set_knobs(mp, ATTN_GLUE_CASES[case][7])
            cache[case, is_self] = _make_attn_glue_reference(ops, case, is_self)
    return cache[case, is_self]


def _make_attn_glue_reference(ops, case, is_self):
    Lq, Lk, Ls, wb, dtype, impl, p, _, _, _ = ATTN_GLUE_CASES[case]
    if is_self:
        Lq = Lk = Ls
    B = 2
    q, k, v, _, bias, nh = _make_attn_inputs(B, Lq, Lk, None, wb, dtype, seed=Lq + 2 * Lk)
    km = torch.zeros(B, Lk, device=DEV)
    km[1, Lk - Lk // 3:] = -10000.0                       # ragged batch
    do = torch.randn(B, Lq, H, generator=torch.Generator().manual_seed(Lq)).to(DEV, dtype)
    qi, ki, vi = (t.clone().requires_grad_(True) for t in (q, k, v))
    bi = bias.clone().requires_grad_(True) if wb else None
    ops.RT.new_step(ATTN_SEED)
    (o, _), paths = _traced(ops, lambda: (lambda o: (o, o.backward(do)))(
        ops.attention(qi, ki, vi, km, bi, nh, p, training=True, impl=impl)))
    got = {"o": o.detach(), "dq": qi.grad, "dk": ki.grad, "dv": vi.grad}
    keep = None
    if p > 0:
        Lk2 = (Lk + 1) // 2 * 2            # the kernels index dropout elements with the key count rounded up to even
        keep = ops.dropout_keep_mask(B * nh * Lq * Lk2, p, ops.RT.seed, 0, DEV).view(B, nh, Lq, Lk2)[..., :Lk]
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    br = bias.double().requires_grad_(True) if wb else None
    orf = _attn_ref(qr, kr, vr, km.double(), br, nh, keep, p)
    orf.backward(do.double())
    ref = {"o": orf.detach(), "dq": qr.grad, "dk": kr.grad, "dv": vr.grad}
    if wb:
        got["dbias"], ref["dbias"] = bi.grad, br.grad
    return dict(q=q, k=k, v=v, km=km, bias=bias, do=do, got=got, ref=ref, paths=paths, shape=(B, Lq, Lk))


@pytest.mark.parametrize("form", ["self", "cross", "hoisted", "strided"])
@pytest.mark.parametrize("case", list(ATTN_GLUE_CASES))
def test_attention_on_packed_and_strided_operands(ops, glue_refs, case, form, monkeypatch):
    """_Attention on the operand layouts of the model -- 'self': packed (B, L, 3H); 'cross': packed (B, Lk, 2H); 'hoisted':
    the middle (B, Lk, 2H) column slice of a three-layer (B, Lk, 3 * 2H) tensor, gradient into the slot of a _KVGradHolder;
    'strided': the same slice without a slot (the gradient buffer _grad_like allocates) -- through the kernel the table names.
    Output and dq / dk / dv (dbias) are BIT-equal to ops.attention on contiguous copies: the same kernel runs the same
    arithmetic in the same order, only the addresses differ.  Both are within the attention bounds of the fp64 reference.
    Sentinels around the slice: the forward leaves the parent alone, the backward the neighbouring layers' columns."""
    _, _, _, wb, dtype, impl, p, env, want_fwd, want_bwd = ATTN_GLUE_CASES[case]
    _set_knobs(monkeypatch, env)
    c = _attn_glue_reference(glue_refs, ops, case, form == "self")
    B, Lq, Lk = c["shape"]
    plan = _planned(ops, B, Lq, Lk, dtype, impl, wb, p)
    assert plan[1] == want_bwd and (form == "self" or plan[0] == want_fwd), (plan, want_fwd, want_bwd)
    assert c["paths"] == tuple(sorted(plan)), (c["paths"], plan)              # the contiguous comparator ran them too
    bi = c["bias"].clone().requires_grad_(True) if wb else None
    holder = parent = None
    if form == "self":
        a = torch.cat([c["q"], c["k"], c["v"]], -1).requires_grad_(True)
        args = ("self", a, None, None)
    else:
        a = c["q"].clone().requires_grad_(True)
        kv = torch.cat([c["k"], c["v"]], -1)
        if form == "cross":
            b_ = kv.requires_grad_(True)
        else:
            parent = torch.full((B, Lk, 3 * 2 * H), SENTINEL, device=DEV, dtype=dtype)
            parent[..., 2 * H:4 * H] = kv
            before = parent.clone()
            if form == "hoisted":
                b_ = parent[..., 2 * H:4 * H].detach().requires_grad_(True)
                holder = ops._KVGradHolder(3, 2 * H)
                holder.buf = torch.full_like(parent, SENTINEL)
                b_._kv_grad_slot = (holder, 1)
            else:
                parent.requires_grad_(True)
                b_ = parent[..., 2 * H:4 * H]
            assert b_.stride() == (Lk * 6 * H, 6 * H, 1)
        args = ("cross", a, b_, None)
    ops.RT.new_step(ATTN_SEED)
    (o, _), paths = _traced(ops, lambda: (lambda o: (o, o.backward(c["do"])))(
        ops._Attention.apply(*args, c["km"], bi, NH, p, impl)))
    assert paths == tuple(sorted(plan)), (paths, plan)
    if form == "self":
        dq, dk, dv = a.grad.split(H, -1)
    elif form == "strided":
        dq, (dk, dv) = a.grad, parent.grad[..., 2 * H:4 * H].split(H, -1)
        assert not bool(parent.grad[..., :2 * H].any()) and not bool(parent.grad[..., 4 * H:].any())
    else:
        dq, (dk, dv) = a.grad, b_.grad.split(H, -1)
    if parent is not None:
        assert torch.equal(parent.detach(), before), "the forward wrote to its operands"
    if holder is not None:
        assert torch.equal(holder.buf[..., 2 * H:4 * H], b_.grad), "the gradient is not in the holder's slot"
        assert bool((holder.buf[..., :2 * H] == SENTINEL).all()) and bool((holder.buf[..., 4 * H:] == SENTINEL).all()), \
            "the backward wrote to a neighbouring layer's columns"
    got = {"o": o.detach(), "dq": dq, "dk": dk, "dv": dv}
    if wb:
        got["dbias"] = bi.grad
    ft, gt = (1e-4, 1e-3) if dtype == F32 else (1e-2, 2.5e-2)
    for name, x in got.items():
        ref = c["ref"][name]
        if name == "o":
            err, bound = float((x.double() - ref).abs().max()), ft * max(1.0, float(ref.abs().max()))
        else:
            err, bound = rel_err(x, ref), gt
        print(f"{case}/{form} {paths} {name}: {err:.3e} (bound {bound:.3e})")
        assert torch.equal(x, c["got"][name]), f"{name} differs from the same call on contiguous operands"
        assert bool(torch.isfinite(x.float()).all()) and err < bound, (name, err, bound)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("mode", ["sep", "cross"])
def test_attention_on_operands_expanded_over_the_batch(ops, mode, dtype):
    """One (1, L, .) tensor expanded to the batch (stride 0) shares its rows between the batches: the kernels would write
    every batch's gradient to one place, so _Attention works on a dense copy.  Output and dq of the other operand are
    bit-equal to the call on dense operands, and the expanded tensor's gradient is the sum of the two batches' (one
    addition: no order to differ in)."""
    B, Lq, Lk = 2, 23, 17
    q, k, v, _, _, _ = _make_attn_inputs(B, Lq, Lk, None, False, dtype, seed=31)
    km = torch.zeros(B, Lk, device=DEV)
    km[1, 12:] = -10000.0
    do = _randn(torch.Generator().manual_seed(32), B, Lq, H, dtype=dtype)
    q1 = q[:1].clone().requires_grad_(True)                        # sep: q, k and v expanded; cross: the packed K|V
    k1, v1, kv1 = (t.clone().requires_grad_(True) for t in (k[:1], v[:1], torch.cat([k[:1], v[:1]], -1)))
    if mode == "sep":
        leaves = (q1, k1, v1)
        args = tuple(t.expand(B, -1, -1) for t in leaves)
    else:
        leaves = (q.clone().requires_grad_(True), kv1)
        args = (leaves[0], kv1.expand(B, -1, -1), None)
    assert all(t is None or t.stride(0) in (0, t.shape[1] * t.shape[2]) for t in args) and args[1].stride(0) == 0
    o = ops._Attention.apply(mode, *args, km, None, NH, 0.0, 0)
    o.backward(do)
    dense = [t.detach().expand(B, -1, -1).contiguous().requires_grad_(True) for t in leaves]
    od = ops._Attention.apply(mode, *dense, *((None,) if mode == "cross" else ()), km, None, NH, 0.0, 0)
    od.backward(do)
    torch.cuda.synchronize()
    assert torch.equal(o, od)
    for leaf, d in zip(leaves, dense):
        want = d.grad if leaf.shape[0] == B else d.grad.sum(0, keepdim=True)
        assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, want)
    assert bool(dense[1].grad[0].ne(dense[1].grad[1]).any())        # the batches' gradients differ: a shared row would lose one


# ----------------------------------------------------------------------------- 4. hoisted_kv by every route
class _KVLayers(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.layers = torch.nn.ModuleList([_Proj(("key", "value")) for _ in range(n)])


HOIST_ROUTES = [("attn", "attn", "attn"), ("attn", "none", "attn"), ("torch", "attn", "none"), ("twice", "attn", "attn"),
                ("noslot", "twice", "torch")]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("routes", HOIST_ROUTES)
def test_hoisted_kv_gradient_by_every_route(ops, routes, dtype):
    """ops.hoisted_kv, three layers: whatever way a gradient reaches the per-layer K|V views -- a slot-aware attention_cross
    ('attn'), not at all ('none': the slice must be exactly zero), a plain torch expression ('torch': the copy-in branch), TWO
    attentions on one view ('twice': the slot is claimed once, the sum must be right), a view of the view that carries no slot
    ('noslot': a strided operand whose gradient buffer _Attention allocates) -- the (B, Lk, layers * 2H) buffer holds each
    layer's dK|dV (against the fp64 attention reference on the K|V the forward produced), and dx and every key / value dW /
    db are the fp64 GEMMs of THAT buffer.  Two runs leave the same bits."""
    from vln_bevbert_amd.arena import ParamArena
    n, B, Lq, Lk = 3, 2, 23, 17
    torch.manual_seed(9)
    m = _KVLayers(n)
    with torch.no_grad():
        for p_ in m.parameters():
            if p_.dim() == 1:
                p_.normal_()
    wn = [f"layers.{i}.{k}.weight" for i in range(n) for k in ("key", "value")]
    bn = [f"layers.{i}.{k}.bias" for i in range(n) for k in ("key", "value")]
    arena = ParamArena(m, DEV, dtype, groups=[wn, bn])
    wc, wg = arena.packed(wn, (n * 2 * H, H))
    bc, bg = arena.packed(bn, (n * 2 * H,))
    by_name = dict(m.named_parameters())
    pw = ops._PackedParam([by_name[x] for x in wn], wc, wg)
    pb = ops._PackedParam([by_name[x] for x in bn], bc, bg)
    g = torch.Generator().manual_seed(10)
    x0 = _randn(g, B, Lk, H, dtype=dtype)
    qs = [[_randn(g, B, Lq, H, dtype=dtype) for _ in range(2)] for _ in range(n)]
    dos = [[_randn(g, B, Lq, H, scale=s, dtype=dtype) for s in (1.0, 3.0)] for _ in range(n)]
    es = [_randn(g, B, Lk, 2 * H, dtype=dtype) for _ in range(n)]
    km = torch.zeros(B, Lk, device=DEV)
    km[1, 12:] = -10000.0

    def consume(i, route, kv, attn):
        """The loss terms of layer i (gradients are dos / es exactly: the products are taken in fp32 / fp64)."""
        wide = torch.float64 if kv.dtype == torch.float64 else F32
        terms = []
        if route in ("attn", "twice", "noslot"):
            for j in range(2 if route == "twice" else 1):
                terms.append((attn(qs[i][j], kv.view_as(kv) if route == "noslot" else kv).to(wide) * dos[i][j].to(wide)).sum())
        elif route == "torch":
            terms.append((kv.to(wide) * es[i].to(wide)).sum())
        return terms

    def run():
        arena.grads.zero_()
        x = x0.clone().requires_grad_(True)
        kvs = ops.hoisted_kv(x, pw, pb, n)
        holder = kvs[0]._kv_grad_slot[0]
        assert all(kv._kv_grad_slot == (holder, i) and kv.shape == (B, Lk, 2 * H) and kv.stride() == (Lk * n * 2 * H, n * 2 * H, 1)
                   for i, kv in enumerate(kvs))
        # the buffer comes from torch.empty: start it from a sentinel so that a slice nobody wrote cannot be zero by luck
        holder.buf = torch.full((B, Lk, n * 2 * H), SENTINEL, device=DEV, dtype=dtype)
        terms = [t for i, r in enumerate(routes) for t in consume(i, r, kvs[i], lambda q, kv: ops.attention_cross(q, kv, km, NH))]
        sum(terms).backward()
        arena.sync()
        torch.cuda.synchronize()
        return [kv.detach().clone() for kv in kvs], holder.buf.clone(), x.grad.clone(), arena.grads.clone()

    kvs, buf, dx, grads = run()
    at, tol = (1e-3 if dtype == F32 else 2.5e-2), _gemm_tol(dtype)
    # stage 1: the buffer, layer by layer
    for i, route in enumerate(routes):
        sl = buf[..., i * 2 * H:(i + 1) * 2 * H]
        if route == "none":
            assert not bool(sl.any()), f"layer {i}: an unconsumed layer's slice is not zero"
        elif route == "torch":
            assert torch.equal(sl, es[i]), f"layer {i}: copy-in"
        else:
            kvr = kvs[i].double().requires_grad_(True)
            sum(consume(i, route, kvr, lambda q, kv: _attn_ref(q.double(), kv[..., :H], kv[..., H:], km.double(), None, NH))).backward()
            _close(f"layer {i} ({route}) dK", sl[..., :H], kvr.grad[..., :H], at)
            _close(f"layer {i} ({route}) dV", sl[..., H:], kvr.grad[..., H:], at)
    # stage 2: the GEMMs of the buffer
    bd, x2 = buf.double().reshape(-1, n * 2 * H), x0.double().reshape(-1, H)
    _close("dx", dx, (bd @ wc.detach().double()).view(B, Lk, H), tol)
    assert set(wn + bn) <= arena._touched
    for j, (w_name, b_name) in enumerate(zip(wn, bn)):
        cols = bd[:, j * H:(j + 1) * H]
        ow, kw = arena.slices[w_name]
        ob, kb = arena.slices[b_name]
        if not bool(cols.any()):
            assert not bool(grads[ow:ow + kw].any()) and not bool(grads[ob:ob + kb].any()), w_name
            continue
        _close(f"d {w_name}", grads[ow:ow + kw].view(H, H), cols.t() @ x2, tol)
        bound = tol
        if dtype == F32 and ".key." in b_name and routes[j // 2] in ("attn", "twice", "noslot"):
            # d key.bias of an attention-fed layer is the sum over the keys of dK, which is ZERO in exact arithmetic (the rows
            # of dS sum to zero: a key bias moves no softmax).  The fp32 buffer's columns add up to rounding residue, 1e-6 of
            # their entries, and no fp32 summation meets 1e-4 of THAT: torch's own fp32 column sum of the same captured buffer
            # is 6.6e-2 .. 9.7e-2 of it from the fp64 sum (rel_err, measured on the MI355X over the routes; the kernel's is
            # 5.9e-2 .. 9.0e-2).  Allowed: twice what that composition shows on this buffer.  bf16, the copy-in route and every
            # value bias keep the plain bound (the residue of a bf16-rounded buffer is 1e-3 of its entries).
            measured = rel_err(buf.reshape(-1, n * 2 * H)[:, j * H:(j + 1) * H].sum(0), cols.sum(0))
            bound = max(tol, 2 * measured)
            print(f"d {b_name}: fp32 torch column sum of the buffer against fp64: rel_err {measured:.3e}")
        _close(f"d {b_name}", grads[ob:ob + kb], cols.sum(0), bound)
    _, buf2, dx2, grads2 = run()
    assert torch.equal(buf, buf2) and torch.equal(dx, dx2) and torch.equal(grads, grads2)
