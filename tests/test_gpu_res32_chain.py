"""The chained form of the fp32-stream LayerNorm: a LayerNorm that will run a backward keeps z32, mean and rstd anyway, so it
does not write its fp32 output y32; the next LayerNorm of the stream recomputes it in its own kernel
(bevbert_layernorm_res32_chain_fwd) with the producer's expression on the producer's operands.  Everything here is an
EQUALITY of bits with the materialised form (BEVBERT_RES32_Y32=1): kernel against kernel, three LayerNorms through
autograd, and a training step of the tiny model.
"""
import pytest
import torch

from tests.test_gpu_rowops_full_size import _gen

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32_CODE = 0
EPS = 1e-12


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


def _p(t):
    return None if t is None else t.data_ptr()


# ----------------------------------------------------------------------------- kernel against kernel
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [256, 768, 1024])
def test_chain_entry_gives_the_bits_of_the_old_entry_fed_y32(ops, H, p, with_bias):
    """A producer LayerNorm through the old entry leaves y32, z32, mean, rstd.  The consumer through the old entry with
    residual = y32 and through the chain entry with (z32, mean, rstd, gamma, beta) of the producer: y16, z32, mean, rstd
    (and y32, when asked for) equal bit for bit.  Rows 1 .. 37: one wave, a partial last workgroup of four rows, ten
    workgroups; fixed dropout seed and offset."""
    seed, off = 20240917, 4096
    for rows in (1, 3, 4, 5, 37):
        rnd = _gen(rows * 1009 + H)
        f32 = lambda *s: torch.full(s, 7.0, device=DEV)
        x0, r0 = rnd(rows, H).to(BF16), 2 * rnd(rows, H)
        g0, b0, bias0 = 1 + 0.1 * rnd(H), 0.1 * rnd(H), 0.1 * rnd(H)
        y16_0 = torch.empty(rows, H, dtype=BF16, device=DEV)
        y32_0, z32_0, mean0, rstd0 = f32(rows, H), f32(rows, H), f32(rows), f32(rows)
        _call("bevbert_layernorm_res32_fwd", _p(x0), _p(bias0), _p(r0), F32_CODE, _p(g0), _p(b0), _p(y16_0), _p(y32_0), _p(z32_0),
              _p(mean0), _p(rstd0), rows, H, EPS, 0.0, seed, 0)
        x = rnd(rows, H).to(BF16)
        gamma, beta = 1 + 0.1 * rnd(H), 0.1 * rnd(H)
        bias = 0.1 * rnd(H) if with_bias else None

        def outputs(fill):
            return (torch.full((rows, H), fill, dtype=BF16, device=DEV), torch.full((rows, H), fill, device=DEV),
                    torch.full((rows, H), fill, device=DEV), torch.full((rows,), fill, device=DEV),
                    torch.full((rows,), fill, device=DEV))

        want = outputs(1.0)
        _call("bevbert_layernorm_res32_fwd", _p(x), _p(bias), _p(y32_0), F32_CODE, _p(gamma), _p(beta), *(_p(t) for t in want),
              rows, H, EPS, p, seed, off)
        for with_y32 in (True, False):
            got = outputs(2.0)
            ptrs = [_p(t) for t in got]
            if not with_y32:
                ptrs[1] = None
            _call("bevbert_layernorm_res32_chain_fwd", _p(x), _p(bias), _p(z32_0), _p(mean0), _p(rstd0), _p(g0), _p(b0),
                  _p(gamma), _p(beta), *ptrs, rows, H, EPS, p, seed, off)
            for name, a, b in zip(("y16", "y32", "z32", "mean", "rstd"), got, want):
                if name == "y32" and not with_y32:
                    assert bool((a == 2.0).all()), "y32 == NULL, yet something was written"
                    continue
                assert torch.equal(a, b), (name, rows, H, p, with_bias, with_y32, float((a.float() - b.float()).abs().max()))


# ----------------------------------------------------------------------------- three LayerNorms through autograd
def _three_layernorms(ops, start, feed16, seed):
    """LN3(LN2(LN1(.))) on 37 rows of 768 with p = 0.1 through ops.bias_dropout_residual_layernorm.  ``start``: "bf16" -- the
    stream starts from a bf16 residual -- or "f32" -- from a bf16 tensor that carries its fp32 twin.  ``feed16``: the dense
    input of a LayerNorm is made from the previous y16 (so every producer receives dy16 AND dy32) or is a leaf of its own
    (LN1 and LN2 receive dy32 alone).  Only the last y16 reaches the loss: the last fp32 output has no consumer.
    Returns (last y16, the gradients of every leaf)."""
    rows, H, p = 37, 768, 0.1
    rnd = _gen(seed)
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.detach().clone().requires_grad_(True)
        return leaves[name]

    if start == "bf16":
        h = leaf("r0", (2 * rnd(rows, H)).to(BF16))
    else:
        r32 = leaf("r0", 2 * rnd(rows, H))
        h = r32.to(BF16)
        h._res32 = r32
    ops.RT.new_step(seed)
    for i in (1, 2, 3):
        u = leaf(f"u{i}", rnd(rows, H).to(BF16))
        x = (h * leaf(f"w{i}", rnd(rows, H).to(BF16)) + u) if feed16 else u
        h = ops.bias_dropout_residual_layernorm(x.contiguous(), leaf(f"bias{i}", 0.1 * rnd(H)), h, leaf(f"gamma{i}", 1 + 0.1 * rnd(H)),
                                                leaf(f"beta{i}", 0.1 * rnd(H)), EPS, p, training=True)
    a = rnd(rows, H)
    (h.float() * a).sum().backward()
    torch.cuda.synchronize()
    missing = [k for k, t in leaves.items() if t.grad is None and not (k.startswith("w") and not feed16)]
    assert not missing, missing
    return h.detach(), {k: t.grad.clone() for k, t in leaves.items() if t.grad is not None}


@pytest.mark.parametrize("start,feed16", [("bf16", True), ("f32", False), ("f32", True)], ids=["from_bf16", "dy32_only", "from_f32"])
def test_three_chained_layernorms_equal_the_materialised_ones(ops, monkeypatch, start, feed16):
    res32 = ops.RT.res32
    ops.RT.res32 = True
    try:
        calls = {}
        from vln_bevbert_amd import ops_core
        raw = ops_core._raw_call
        for knob in ("1", "0"):
            monkeypatch.setenv("BEVBERT_RES32_Y32", knob)
            names = []
            monkeypatch.setattr(ops_core, "_raw_call", lambda name, *a, names=names: (names.append(name), raw(name, *a))[1])
            out = _three_layernorms(ops, start, feed16, 4242)
            monkeypatch.setattr(ops_core, "_raw_call", raw)
            calls[knob] = (names, out)
        (n1, (y1, g1)), (n0, (y0, g0)) = calls["1"], calls["0"]
        # the knob is what it says: no chain launches with it; without it LN2 and LN3 chain, and LN1, whose residual is a
        # plain bf16 or fp32 tensor, takes the old entry
        assert n1.count("bevbert_layernorm_res32_chain_fwd") == 0 and n1.count("bevbert_layernorm_res32_fwd") == 3
        assert n0.count("bevbert_layernorm_res32_chain_fwd") == 2 and n0.count("bevbert_layernorm_res32_fwd") == 1
        assert torch.equal(y1, y0)
        assert g1.keys() == g0.keys()
        for k in g1:
            assert torch.equal(g1[k], g0[k]), (k, float((g1[k].float() - g0[k].float()).abs().max()))
    finally:
        ops.RT.res32 = res32


def test_lazy_layernorm_allocates_no_y32_and_hands_on_a_handle(ops, monkeypatch):
    """In grad mode the bf16 output carries a handle (z32, mean, rstd, gamma, beta) and no fp32 tensor of its own; under
    no_grad, with the knob, and through _BiasDropResLN32.apply directly it carries / returns the materialised y32."""
    from vln_bevbert_amd.ops_rowops import _BiasDropResLN32, _Res32Handle
    res32 = ops.RT.res32
    ops.RT.res32 = True
    try:
        rnd = _gen(5)
        rows, H = 5, 256
        x, r = rnd(rows, H).to(BF16).requires_grad_(True), (2 * rnd(rows, H)).to(BF16)
        gamma, beta = (1 + 0.1 * rnd(H)).requires_grad_(True), (0.1 * rnd(H)).requires_grad_(True)
        monkeypatch.delenv("BEVBERT_RES32_Y32", raising=False)
        y = ops.bias_dropout_residual_layernorm(x, None, r, gamma, beta, EPS)
        assert isinstance(y._res32, _Res32Handle) and y._res32.z32.grad_fn is not None and y._res32.gamma is gamma
        y16, y32 = _BiasDropResLN32.apply(x, None, r, gamma, beta, EPS, 0.0)
        with torch.no_grad():
            yn = ops.bias_dropout_residual_layernorm(x, None, r, gamma, beta, EPS)
        monkeypatch.setenv("BEVBERT_RES32_Y32", "1")
        yk = ops.bias_dropout_residual_layernorm(x, None, r, gamma, beta, EPS)
        for t in (yn._res32, yk._res32):
            assert torch.is_tensor(t) and torch.equal(t, y32)
        assert torch.equal(y, y16) and torch.equal(yn, y16) and torch.equal(yk, y16)
    finally:
        ops.RT.res32 = res32


# ----------------------------------------------------------------------------- the tiny model
def _tiny_step(task, grad, monkeypatch):
    """One step of the tiny pre-training model (bf16 operands, fp32 residual stream, dropout on): (loss, gradient arena,
    number of chained LayerNorm launches)."""
    from tests.test_gpu_model import build
    from vln_bevbert_amd import ops, ops_core, synthetic
    raw, chained = ops_core._raw_call, []
    monkeypatch.setattr(ops_core, "_raw_call", lambda name, *a: (chained.append(name == "bevbert_layernorm_res32_chain_fwd"), raw(name, *a))[1])
    from vln_bevbert_amd.config import BevBertConfig
    cfg = BevBertConfig.tiny()
    model, arena = build(cfg, "pretrain_state_dict_keys_tiny.txt", BF16, residual=torch.float32)
    model.train()
    batch = synthetic.batch_to(synthetic.make_batch(cfg, task, 3, seed=11, ragged=True), DEV)
    ops.RT.new_step(77)
    if not grad:
        with torch.no_grad():
            loss = model(batch, task).mean()
        torch.cuda.synchronize()
        return loss.detach().clone(), None, sum(chained)
    arena.zero_grad()
    loss = model(batch, task).mean()
    loss.backward()
    arena.sync()
    torch.cuda.synchronize()
    return loss.detach().clone(), arena.grads.detach().clone(), sum(chained)


@pytest.mark.parametrize("grad", [True, False], ids=["train", "no_grad"])
@pytest.mark.parametrize("task", ["mlm", "sap"])
def test_tiny_model_step_equals_the_materialised_one(ops, monkeypatch, task, grad):
    try:
        monkeypatch.setenv("BEVBERT_RES32_Y32", "1")
        loss1, grads1, chained1 = _tiny_step(task, grad, monkeypatch)
        monkeypatch.setenv("BEVBERT_RES32_Y32", "0")
        loss0, grads0, chained0 = _tiny_step(task, grad, monkeypatch)
        assert chained1 == 0 and (chained0 > 0) == grad, (chained1, chained0)      # the model's layers do take the chained form
        assert torch.equal(loss1, loss0), (float(loss1), float(loss0))
        if grad:
            assert float(grads1.abs().max()) > 0
            assert torch.equal(grads1, grads0), float((grads1 - grads0).abs().max())
    finally:
        ops.RT.res32 = False
