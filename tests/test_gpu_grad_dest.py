"""Where every parameter gradient lands, on the device: each op of tests/grad_dest_cases.py with arena parameters (the second
reduction stages deferred to the step's one bevbert_multi_finalize, and run in place) and with plain parameters, all
trainable and with each parameter frozen in turn.

Trainable arena parameters receive a non-zero prefill plus the fp64 reference; everything else in the arena -- frozen
parameters, the other rows of a RowOfTable's table, the parameters of the other ops, the padding -- keeps the prefill bit
for bit.  No tolerance is new:
  * activation biases, BertEmbeddings, small-K projection, graph bias, table lookups: the elementwise gates tests/body_cases.py
    and tests/smallk_cases.py state for these inputs (their generators are used at this file's shapes), the sink's start value
    one more fp32 rounding where the stated gate does not already count it;
  * LayerNorm gamma / beta / bias: 1e-4 of the reference's largest element, as in tests/test_gpu_rowops_full_size.py and
    tests/test_gpu_serial_path_kernels.py, against a reference that reads xhat from z as the kernel saved it (rounded to the
    compute dtype: body_cases.embed_ref does the same);
  * GEMM-backed weight and bias gradients: rel_err < 1e-4 (fp32) / 1e-2 (bf16), as in tests/test_gpu_linear_attention_glue.py.
A plain parameter's gradient is returned in the parameter's dtype: 2^-8 |want| more for bf16."""
import pytest
import torch

from tests import body_cases as bc
from tests import grad_dest_cases as gc
from tests import smallk_cases as sk
from tests.kernel_gates import U8, U24
from tests.test_gpu_kernels import ops  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# entry -> argument indices of its column-sum destinations (null when the second stage is deferred)
DESTS = {"bevbert_layernorm_bwd_add": (8, 9, 10), "bevbert_layernorm_bwd": (7, 8, 9), "bevbert_bias_gelu_bwd": (4,),
         "bevbert_bias_relu_bwd": (4,)}
QUEUES = {"layernorm", "bdrl", "bdrl_row", "prenorm", "gelu", "relu", "linear", "linear_packed", "hoisted_kv", "embed_ln",
          "smallk", "lookup"}            # ops that hand ReduceQueue a record when their parameters live in the arena
# smallk has one form (smallk_linear_layernorm_plus_supported asks for the deferral); lookup's other route is a one-hot GEMM
SAME_BITS_DIRECT = set(gc.OPS) - {"smallk", "lookup"}


# ----------------------------------------------------------------------------- fp64 references
def _ln_ref(i, gamma, beta, bias, dtype, prenorm):
    """dgamma, dbeta, dbias of LayerNorm(x + bias + res) (prenorm: z carries a gradient of its own), xhat read from the z
    the kernel saved."""
    x, res, dy = i["x"].cpu(), i["res"].cpu(), i["dy"].cpu().double()
    z = x.double() + bias.double() + res.double()
    z_saved = ((x.float() + bias.float()) + res.float()).to(dtype).double()
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + gc.EPS)
    xh = (z_saved - mean) * rstd
    g = gamma.double() * dy
    dz = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if prenorm:
        dz = dz + i["dz"].cpu().double()
    return (dy * xh).sum(0), dy.sum(0), dz.sum(0)


def _rel(delta, tol, rows=None):
    """Gate ``tol`` of the reference's largest element (on ``rows`` of a table; the other rows may not move)."""
    allow = torch.full_like(delta, tol * float(delta.abs().max()))
    if rows is not None:
        keep = torch.zeros(delta.shape[0], dtype=torch.bool)
        keep[rows] = True
        allow[~keep] = 0.0
    return allow


def reference(op, m, i, dtype, start, lookup_gemm=False):
    """{parameter name: (fp64 gradient without the start value, elementwise gate)}; ``start``: name -> the sink's prefill (CPU).
    ``lookup_gemm``: the table lookup's gradient came from its one-hot GEMM (no deferral, or a plain table): the GEMM gate."""
    val = lambda n: dict(m.named_parameters())[n].detach().float().cpu()
    gt = 1e-4 if dtype == torch.float32 else 1e-2
    out = {}
    if op in ("layernorm", "bdrl", "bdrl_row", "prenorm"):
        bias = torch.zeros(gc.H) if op == "layernorm" else val("typ5.weight")[gc.ROW] if op == "bdrl_row" else val("ln_in")
        ii = dict(i, res=torch.zeros_like(i["x"])) if op == "layernorm" else i
        dg, db, dbi = _ln_ref(ii, val("ln.weight"), val("ln.bias"), bias, dtype, op == "prenorm")
        out = {"ln.weight": (dg, _rel(dg, 1e-4)), "ln.bias": (db, _rel(db, 1e-4))}
        if op == "bdrl_row":
            t = torch.zeros(gc.TROWS, gc.H, dtype=torch.float64)
            t[gc.ROW] = dbi
            out["typ5.weight"] = (t, _rel(t, 1e-4, [gc.ROW]))
        elif op != "layernorm":
            out["ln_in"] = (dbi, _rel(dbi, 1e-4))
    elif op in ("gelu", "relu"):
        n, x, dy = ("gelu_b", i["xg"].cpu(), i["dg"].cpu()) if op == "gelu" else ("relu_b", i["xr"].cpu(), i["dr"].cpu())
        if op == "gelu":
            a, y, _, dx, dbias = bc.gelu_ref(x, val(n), dy)
            gate = bc.gelu_gates(a, y, dx, dy, dtype == BF)[2]
        else:
            _, dx, dbias = bc.relu_ref(x, val(n), dy)
            gate = (gc.ROWS + 4) * U24 * dx.double().abs().sum(0)
        out[n] = (dbias, gate + U24 * (start[n].double() + dbias).abs())           # + the sum's one addition to the sink
    elif op in ("linear", "linear3", "linear_packed", "hoisted_kv"):
        x, dy, wn, bn = {"linear": (i["xl"], i["dl"], ["lin.weight"], ["lin.bias"]),
                         "linear3": (i["xl"], i["dl3"], ["lin3.weight"], ["lin3.bias"]),
                         "linear_packed": (i["x"], i["dqkv"], gc.QKV_W, gc.QKV_B),
                         "hoisted_kv": (i["ctx"], torch.cat(i["dkv"], -1) if op == "hoisted_kv" else None, gc.KV_W, gc.KV_B)}[op]
        x2, dy2 = x.cpu().double().reshape(gc.ROWS, -1), dy.cpu().double().reshape(gc.ROWS, -1)
        dW, db = dy2.t() @ x2, dy2.sum(0)
        for names, full in ((wn, dW), (bn, db)):                # a packed run: one gate over the whole GEMM output
            for n, part in zip(names, full.chunk(len(names), 0)):
                out[n] = (part, torch.full_like(part, gt * float(full.abs().max())))
    elif op == "embed_ln":
        case = bc.embed_case(*gc.EMB)
        ref, r32 = bc.embed_ref(case, dtype, None), bc.embed_torch(case, dtype, None, torch.float32)
        for k, n in (("word", "word.weight"), ("pos", "pos.weight"), ("typ", "typ.weight"), ("gamma", "eln.weight"),
                     ("beta", "eln.bias")):                     # the gate of test_bert_embeddings_forward_and_every_gradient...
            want = ref[k] + start[n].double()
            allow = torch.full_like(want, max(1e-4 * float(want.abs().max()), 4.0 * float((r32[k].double() - ref[k]).abs().max())))
            if dtype == BF and k in ref["abs"]:
                allow = allow + U8 * ref["abs"][k]
            allow[ref["abs"][k] == 0 if k in ref["abs"] else torch.zeros_like(want, dtype=torch.bool)] = 0.0      # rows nobody names
            out[n] = (ref[k], allow)
    elif op == "smallk":
        r = sk.ref(gc.ROWS, gc.K, gc.H, dtype)
        for key, n in (("W", "loc.weight"), ("b", "loc.bias"), ("gamma", "loc_ln.weight"), ("beta", "loc_ln.bias"), ("table", "nav.weight")):
            q = "d" + key
            out[n] = (r[q] - start[n].double(), r["gate"][q])   # (sk.ref includes the start values, and so do its gates)
    elif op == "graph_bias":
        dw, db, gw, gb = bc.graph_ref(*bc.graph_case(gc.LAYERS, gc.B, gc.NH, gc.G))
        out = {"sprel.weight": (torch.full((1, 1), dw - bc.GRAPH_DW0, dtype=torch.float64), torch.full((1, 1), gw)),
               "sprel.bias": (torch.full((1,), db - bc.GRAPH_DB0, dtype=torch.float64), torch.full((1,), gb))}
    elif op == "use_param":
        terms = i["vec"].cpu().double() * i["dvec"].cpu().double()
        out["scalar"] = (terms.sum().view(1), (8 + 2) * U24 * (terms.abs().sum().view(1) + start["scalar"].double().abs()))
    elif op == "lookup":
        want, gate = sk.scatter_ref(i["look"].cpu(), i["dy"].cpu(), gc.TROWS, start["typ5.weight"])
        delta = want - start["typ5.weight"].double()
        out["typ5.weight"] = (delta, gt * float(delta.abs().max()) * (gate > 0) if lookup_gemm else gate)
    return out


# ----------------------------------------------------------------------------- one run
def _prefill(m, arena, dtype):
    p = torch.sin(torch.arange(arena.numel, dtype=torch.float32) * 0.37) + 0.01
    s = sk.case(gc.ROWS, gc.K, gc.H, dtype)["start"]
    for n, t in (("loc.weight", s["W"]), ("loc.bias", s["b"]), ("loc_ln.weight", s["gamma"]), ("loc_ln.bias", s["beta"]),
                 ("nav.weight", s["table"]), ("sprel.weight", torch.tensor(bc.GRAPH_DW0)), ("sprel.bias", torch.tensor(bc.GRAPH_DB0))):
        o, k = arena.slices[n]
        p[o:o + k] = t.reshape(-1)
    return p


def run(ops, monkeypatch, op, dtype, in_arena=True, frozen=(), defer=True):
    from vln_bevbert_amd import ops_core
    from vln_bevbert_amd.arena import ParamArena
    labels, _, runner = gc.OPS[op]
    m = gc.Params(dtype)
    gc.freeze(m, {n for l in frozen for n in labels[l]})
    r = {"m": m, "i": gc.inputs(dtype, DEV), "calls": []}
    monkeypatch.setattr(ops.RT, "res32", False)
    monkeypatch.setattr(ops.WgradStream, "DEFER_FINALIZE", defer)
    if in_arena:
        m.arena = arena = ParamArena(m, DEV, dtype, groups=gc.GROUPS)
        r["prefill"] = _prefill(m, arena, dtype)
        arena.grads.copy_(r["prefill"])
        ops.RT.scratch.reset()
    else:                                                    # GEMM operands and tables in the compute dtype, the rest fp32
        m.to(DEV)
        for mod in m.modules():
            if isinstance(mod, (torch.nn.Linear, torch.nn.Embedding)):
                mod.to(dtype)
    raw = ops_core._raw_call
    monkeypatch.setattr(ops_core, "_raw_call", lambda name, *a: (r["calls"].append((name, a)), raw(name, *a))[1])
    outs, grads = runner(ops, m, r["i"])
    r["ran"] = any(o.requires_grad for o in outs)
    if r["ran"]:
        torch.autograd.backward(outs, grads)
    if in_arena:
        arena.sync()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops_core, "_raw_call", raw)
    if in_arena:
        r["grads"], r["touched"] = arena.grads.cpu(), set(arena._touched)
    r["pgrad"] = {n: p.grad for n, p in m.named_parameters()}
    return r


def _check_arena(op, dtype, r, ref, trainable, tag):
    """Trainable ranges: prefill + reference within the gate; every other element of the arena: the prefill's bits."""
    arena, got, pre = r["m"].arena, r["grads"], r["prefill"]
    assert r["touched"] == trainable, (tag, r["touched"])
    same = torch.ones(arena.numel, dtype=torch.bool)
    for n in sorted(trainable):
        o, k = arena.slices[n]
        same[o:o + k] = False
        delta, allow = ref[n]
        err = (got[o:o + k].double() - pre[o:o + k].double() - delta.reshape(-1)).abs()
        print(f"grad-dest: {tag:<40} {n:<18} worst error / gate {float((err / allow.reshape(-1).clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= allow.reshape(-1)).all()), (tag, n, float(err.max()), float(allow.max()))
        assert bool((got[o:o + k] != pre[o:o + k]).any()), (tag, n, "nothing arrived")
    assert torch.equal(got[same], pre[same]), (tag, "a frozen parameter, another op's parameter or the padding changed")
    for n, p in r["m"].named_parameters():
        assert (p.grad is None) == (n not in trainable), (tag, n)


def _check_route(op, r, defer, any_queued):
    names = [c[0] for c in r["calls"]]
    assert names.count("bevbert_multi_finalize") == (1 if defer and any_queued else 0), names
    for name, args in r["calls"]:
        if name in DESTS and defer:
            assert all(args[k] is None for k in DESTS[name]), (name, "a deferred first stage was handed a destination")
    assert ("bevbert_colsum_partials" in names) == (defer and op in ("linear", "linear_packed", "hoisted_kv") and any_queued)
    assert "bevbert_colsum" not in names or not defer


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=bc.DT_ID)
@pytest.mark.parametrize("op", list(gc.OPS))
def test_arena_parameters_trainable_and_frozen_deferred_and_direct(ops, monkeypatch, op, dtype):
    labels = gc.OPS[op][0]
    everything = {n for names in labels.values() for n in names}
    full = run(ops, monkeypatch, op, dtype)
    start = {n: full["prefill"][o:o + k].view(dict(full["m"].named_parameters())[n].shape)
             for n, (o, k) in full["m"].arena.slices.items()}
    ref = reference(op, full["m"], full["i"], dtype, start)
    assert full["ran"] and set(ref) == everything
    _check_arena(op, dtype, full, ref, everything, f"{op} {bc.DT_ID(dtype)}")
    _check_route(op, full, True, op in QUEUES)
    if op in SAME_BITS_DIRECT:
        direct = run(ops, monkeypatch, op, dtype, defer=False)
        assert torch.equal(direct["grads"], full["grads"]), "deferred and direct reductions differ"
        _check_route(op, direct, False, op in QUEUES)
        for name, args in direct["calls"]:                   # in place: the destinations themselves
            if name in DESTS:
                assert any(args[k] is not None for k in DESTS[name]), name
    elif op == "lookup":                                     # its other route: a one-hot GEMM in the compute dtype
        direct = run(ops, monkeypatch, op, dtype, defer=False)
        _check_arena(op, dtype, direct, reference(op, full["m"], full["i"], dtype, start, lookup_gemm=True), everything,
                     f"{op} {bc.DT_ID(dtype)} direct")
        _check_route(op, direct, False, True)
    for label, names in labels.items():
        r = run(ops, monkeypatch, op, dtype, frozen=(label,))
        assert r["ran"] == (op not in ("use_param", "lookup"))
        left = everything - set(names)
        _check_arena(op, dtype, r, ref, left, f"{op} {bc.DT_ID(dtype)} frozen {label}")
        for n in left:                                       # the others: what they got with everything trainable
            o, k = r["m"].arena.slices[n]
            assert torch.equal(r["grads"][o:o + k], full["grads"][o:o + k]), (label, n)
        queued = {"linear": "lin.bias" in left, "linear_packed": bool(left & set(gc.QKV_B)), "smallk": "nav.weight" in left,
                  "hoisted_kv": bool(left & set(gc.KV_B))}.get(op, bool(left) and op in QUEUES)      # (weights fold elsewhere)
        _check_route(op, r, True, queued)


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=bc.DT_ID)
@pytest.mark.parametrize("op", [op for op, (_, needs_arena, _) in gc.OPS.items() if not needs_arena])
def test_plain_parameters_trainable_and_frozen(ops, monkeypatch, op, dtype):
    labels = gc.OPS[op][0]
    everything = {n for names in labels.values() for n in names}
    ref = None
    for frozen in [()] + [(l,) for l in labels]:
        r = run(ops, monkeypatch, op, dtype, in_arena=False, frozen=frozen)
        if ref is None:
            params = dict(r["m"].named_parameters())
            ref = reference(op, r["m"], r["i"], dtype, {n: torch.zeros(p.shape) for n, p in params.items()}, lookup_gemm=True)
            off = run(ops, monkeypatch, op, dtype, in_arena=False, defer=False)       # the switch is the arena's alone
            assert [c[0] for c in off["calls"]] == [c[0] for c in r["calls"]]
            assert all(torch.equal(g, r["pgrad"][n]) for n, g in off["pgrad"].items() if g is not None)
        gone = {n for l in frozen for n in labels[l]}
        assert "bevbert_multi_finalize" not in [c[0] for c in r["calls"]]
        for n, g in r["pgrad"].items():
            assert (g is None) == (n not in everything - gone), (op, frozen, n)
            if g is not None:
                delta, allow = ref[n]
                allow = allow + (U8 * delta.abs() if g.dtype == BF else 0.0)
                err = (g.detach().cpu().double() - delta).abs()
                assert g.dtype == params[n].dtype and bool((err <= allow).all()), (op, frozen, n, float(err.max()), float(allow.max()))
