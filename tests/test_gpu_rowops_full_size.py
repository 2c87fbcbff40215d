"""Row kernels of the bf16 + fp32-residual training step at the benchmark's sizes (28 224 BEV rows, 5 120 text rows at
B = 64), against fp64 torch references computed on the GPU from the same inputs: the fp32-residual LayerNorm
(ln_res32_*_kernel), the deferred second stages of the column reductions (ReduceQueue / bevbert_multi_finalize) against
the direct ones, and bias + GELU / ReLU.

bf16 inputs are upcast exactly; dropout uses the exported keep mask at the offset the op drew.  "One bf16 rounding" means
|got - ref| <= 2^-8 |ref| + 1e-6 max|ref| element by element.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def bf16_rounding_ratio(got, ref):
    """Worst |got - ref| / (2^-8 |ref| + 1e-6 max|ref|): at most 1 when every element is within one bf16 rounding."""
    ref = ref.double()
    bound = 2.0 ** -8 * ref.abs() + 1e-6 * float(ref.abs().max())
    return float(((got.double() - ref).abs() / bound.clamp_min(1e-30)).max())


def report(name, **vals):
    print(f"\n[worst] {name}: " + " ".join(f"{k}={v:.3e}" for k, v in vals.items()))


def _gen(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return lambda *shape: torch.randn(*shape, device=DEV, generator=g)


def _keep(ops, n, p, offset, shape):
    return ops.dropout_keep_mask(n, p, ops.RT.seed, offset, DEV).view(shape) if p > 0 else None


def _ln_ref64(x, bias, residual, gamma, beta, keep, p, eps=1e-12):
    """fp64 LayerNorm(dropout(x + bias) + residual); every operand a leaf that requires grad (bias may be None)."""
    t = x if bias is None else x + bias
    if keep is not None:
        t = torch.where(keep, t / (1 - p), torch.zeros_like(t))
    if residual is not None:
        t = t + residual
    return torch.nn.functional.layer_norm(t, (t.shape[-1],), gamma, beta, eps)


def _leaf64(t):
    return None if t is None else t.detach().double().requires_grad_(True)


# ----------------------------------------------------------------------------- fp32-residual LayerNorm
RES32_CASES = [
    # rows, H, residual dtype, outputs that receive a gradient, dropout p, bias
    *[(r, 768, "f32", "both", 0.1, "grad") for r in (1, 3, 517, 5120, 8191, 8192, 16397, 28224)],
    *[(5120, h, "f32", "both", 0.1, "grad") for h in (256, 512, 1024)],
    (517, 768, "bf16", "both", 0.1, "grad"),            # where a residual stream starts: dz goes back in bf16
    (28224, 768, "bf16", "both", 0.0, "grad"),
    (8192, 768, "f32", "y16", 0.0, "grad"),
    (8192, 768, "f32", "y32", 0.1, "grad"),
    (16397, 768, "bf16", "y16", 0.1, "grad"),
    (517, 768, "f32", "both", 0.1, None),
    (5120, 768, "bf16", "y32", 0.0, "frozen"),
]


@pytest.mark.parametrize("rows,H,res,outs,p,bias_kind", RES32_CASES)
def test_res32_layernorm_against_fp64(ops, rows, H, res, outs, p, bias_kind):
    """_BiasDropResLN32 (bevbert_layernorm_res32_fwd / _bwd with plain parameters): y32 against the fp64 LayerNorm, y16 the
    bf16 rounding of y32 bit for bit, and every gradient -- with one or both outputs driving the backward, an fp32 or a
    bf16 residual, dropout against the exported mask, and row counts on both sides of colwise_blocks()'s regimes."""
    from vln_bevbert_amd.ops_rowops import _BiasDropResLN32
    rnd = _gen(rows * 131 + H)
    x = rnd(rows, H).to(BF16).requires_grad_(True)
    residual = (2 * rnd(rows, H)).to(BF16 if res == "bf16" else torch.float32).requires_grad_(True)
    gamma = (1 + 0.1 * rnd(H)).requires_grad_(True)
    beta = (0.1 * rnd(H)).requires_grad_(True)
    bias = None if bias_kind is None else (0.1 * rnd(H)).requires_grad_(bias_kind == "grad")
    a = rnd(rows, H).to(BF16).float()            # exact in bf16: y16 receives a itself as its gradient
    b = rnd(rows, H)
    ops.RT.new_step(4242 + rows + H)
    off = ops.RT.offset
    y16, y32 = _BiasDropResLN32.apply(x, bias, residual, gamma, beta, 1e-12, p)
    keep = _keep(ops, rows * H, p, off, (rows, H))

    xd, rd, gd, bd, bid = (_leaf64(t) for t in (x, residual, gamma, beta, bias))
    yr = _ln_ref64(xd, bid, rd, gd, bd, keep, p)
    y_err = float((y32.double() - yr.detach()).abs().max()) / max(1.0, float(yr.detach().abs().max()))
    assert y_err <= 2e-5, y_err
    assert torch.equal(y16, y32.to(BF16)), "y16 is not the bf16 rounding of y32"

    loss, dy = 0, 0
    if outs in ("both", "y16"):
        loss, dy = loss + (y16.float() * a).sum(), dy + a.double()
    if outs in ("both", "y32"):
        loss, dy = loss + (y32 * b).sum(), dy + b.double()
    loss.backward()
    yr.backward(dy)
    errs = {"y": y_err}
    if res == "f32":
        errs["dz"] = rel_err(residual.grad, rd.grad)
        assert errs["dz"] <= 2e-5, errs
    else:
        errs["dz_bf16"] = bf16_rounding_ratio(residual.grad, rd.grad)
        assert errs["dz_bf16"] <= 1.0, errs
    errs["dx16"] = bf16_rounding_ratio(x.grad, xd.grad)
    assert errs["dx16"] <= 1.0, errs
    errs["dgamma"] = rel_err(gamma.grad, gd.grad)
    errs["dbeta"] = rel_err(beta.grad, bd.grad)
    assert errs["dgamma"] <= 1e-4 and errs["dbeta"] <= 1e-4, errs
    if bias_kind == "grad":
        errs["dbias"] = rel_err(bias.grad, bid.grad)
        assert errs["dbias"] <= 1e-4, errs
    elif bias_kind == "frozen":
        assert bias.grad is None
    report(f"res32 LN rows={rows} H={H} res={res} outs={outs} p={p} bias={bias_kind}", **errs)


# ----------------------------------------------------------------------------- deferred vs direct column reductions
LIN_CASES = ((28224, (768, 2304, 3072)), (5120, (1, 3, 30522)))
ROWS_A, ROWS_B = 28224, (28224, 5120)


class _Params(torch.nn.Module):
    """Parameters whose gradients take the two-stage column reductions: a plain LayerNorm, an fp32-residual LayerNorm used
    twice in one backward (shared gamma / beta / bias), the GELU and ReLU biases and Linear biases (weights frozen)."""

    def __init__(self):
        super().__init__()
        self.ln_a, self.ln_b = torch.nn.LayerNorm(768, eps=1e-12), torch.nn.LayerNorm(768, eps=1e-12)
        self.ln_a_in, self.ln_b_in = torch.nn.Parameter(torch.zeros(768)), torch.nn.Parameter(torch.zeros(768))
        self.gelu_b, self.relu_b = torch.nn.Parameter(torch.zeros(3072)), torch.nn.Parameter(torch.zeros(768))
        self.lins = torch.nn.ModuleList(torch.nn.Linear(16, c) for _, cs in LIN_CASES for c in cs)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for n, p in self.named_parameters():
                p.copy_((1.0 if n.endswith("ln_a.weight") or n.endswith("ln_b.weight") else 0.0)
                        + 0.2 * torch.randn(p.shape, generator=g))
        for lin in self.lins:
            lin.weight.requires_grad_(False)


def _gelu64(t):
    return 0.5 * t * (1 + torch.erf(t / math.sqrt(2)))


def _dgelu64(t):
    return 0.5 * (1 + torch.erf(t / math.sqrt(2))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)


def _deferred_inputs():
    rnd = _gen(99)
    inp = {"xa": rnd(ROWS_A, 768), "ra": rnd(ROWS_A, 768), "dya": rnd(ROWS_A, 768),
           "xg": (2 * rnd(ROWS_A, 3072)).to(BF16), "dg": rnd(ROWS_A, 3072).to(BF16),
           "xr": rnd(5120, 768).to(BF16), "dr": rnd(5120, 768).to(BF16),
           "xl": [rnd(r, 16).to(BF16) for r, cs in LIN_CASES for _ in cs],
           "dl": [rnd(r, c).to(BF16) for r, cs in LIN_CASES for c in cs]}
    for i, rows in enumerate(ROWS_B):
        inp[f"xb{i}"] = rnd(rows, 768).to(BF16)
        inp[f"rb{i}"] = 2 * rnd(rows, 768)
        inp[f"d16b{i}"] = rnd(rows, 768).to(BF16)
        inp[f"d32b{i}"] = rnd(rows, 768)
    return inp


def _deferred_step(ops, m, inp, prefill):
    """One backward through every op; returns the arena's gradients and the dropout offsets of the LayerNorms."""
    from vln_bevbert_amd.ops_rowops import _BiasDropResLN32
    m.arena.grads.copy_(prefill)
    ops.RT.scratch.reset()
    ops.RT.new_step(777)
    offs, outs, grads = {}, [], []
    offs["a"] = ops.RT.offset
    outs.append(ops.bias_dropout_residual_layernorm(inp["xa"], m.ln_a_in, inp["ra"], m.ln_a.weight, m.ln_a.bias, 1e-12,
                                                    0.1, training=True, inplace_z=False))
    grads.append(inp["dya"])
    for i in range(len(ROWS_B)):
        offs[f"b{i}"] = ops.RT.offset
        outs += list(_BiasDropResLN32.apply(inp[f"xb{i}"], m.ln_b_in, inp[f"rb{i}"], m.ln_b.weight, m.ln_b.bias, 1e-12, 0.1))
        grads += [inp[f"d16b{i}"], inp[f"d32b{i}"]]
    outs += [ops.bias_gelu(inp["xg"], m.gelu_b), ops.bias_relu(inp["xr"], m.relu_b)]
    grads += [inp["dg"], inp["dr"]]
    for lin, x, d in zip(m.lins, inp["xl"], inp["dl"]):
        outs.append(ops.linear(x, lin.weight, lin.bias))
        grads.append(d)
    torch.autograd.backward(outs, grads)
    m.arena.sync()
    torch.cuda.synchronize()
    return m.arena.grads.clone(), offs


def test_deferred_reductions_equal_direct_reductions_and_fp64(ops, monkeypatch):
    """Arena parameters with WgradStream.DEFER_FINALIZE (the default): first stages leave per-block partials in the scratch
    ring and ONE bevbert_multi_finalize folds them into the arena -- onto a non-zero prefill, the two records of the shared
    LayerNorm in successive launches; the 1- / 3- / 30 522-wide biases go through bevbert_colsum_any.  The result is the
    prefill plus the fp64 gradients, the same bits on a second run, and the same bits as the direct reductions
    (launch_finalize / bevbert_colsum), whose summation order multi_finalize_kernel reproduces."""
    from vln_bevbert_amd.arena import ParamArena
    torch.manual_seed(0)
    m = _Params()
    m.arena = ParamArena(m, DEV, BF16)
    inp = _deferred_inputs()
    prefill = torch.sin(torch.arange(m.arena.numel, device=DEV, dtype=torch.float32) * 0.37)
    res32 = ops.RT.res32
    try:
        ops.RT.res32 = False
        assert ops.WgradStream.DEFER_FINALIZE
        g1, offs = _deferred_step(ops, m, inp, prefill)
        g2, _ = _deferred_step(ops, m, inp, prefill)
        monkeypatch.setattr(ops.WgradStream, "DEFER_FINALIZE", False)
        g3, _ = _deferred_step(ops, m, inp, prefill)
    finally:
        ops.RT.res32 = res32
    assert torch.equal(g1, g2), "a second identical run gave other bits"
    diff = {n: float((g1[o:o + k] - g3[o:o + k]).abs().max()) for n, (o, k) in m.arena.slices.items()}
    assert torch.equal(g1, g3), f"deferred and direct reductions differ: {diff}"

    # fp64 references of every parameter gradient
    want = {}
    P = {n: _leaf64(p) for n, p in m.named_parameters()}
    ka = _keep(ops, ROWS_A * 768, 0.1, offs["a"], (ROWS_A, 768))
    ya = _ln_ref64(inp["xa"].double(), P["ln_a_in"], inp["ra"].double(), P["ln_a.weight"], P["ln_a.bias"], ka, 0.1)
    ya.backward(inp["dya"].double())
    for i, rows in enumerate(ROWS_B):
        kb = _keep(ops, rows * 768, 0.1, offs[f"b{i}"], (rows, 768))
        yb = _ln_ref64(inp[f"xb{i}"].double(), P["ln_b_in"], inp[f"rb{i}"].double(), P["ln_b.weight"], P["ln_b.bias"],
                       kb, 0.1)
        yb.backward(inp[f"d16b{i}"].double() + inp[f"d32b{i}"])
    for n in ("ln_a_in", "ln_a.weight", "ln_a.bias", "ln_b_in", "ln_b.weight", "ln_b.bias"):
        want[n] = P[n].grad
    want["gelu_b"] = (inp["dg"].double() * _dgelu64(inp["xg"].double() + P["gelu_b"].detach())).sum(0)
    want["relu_b"] = (inp["dr"].double() * (inp["xr"].double() + P["relu_b"].detach() > 0)).sum(0)
    for i, d in enumerate(inp["dl"]):
        want[f"lins.{i}.bias"] = d.double().sum(0)
    errs = {}
    for n, ref in want.items():
        o, k = m.arena.slices[n]
        got = g1[o:o + k].double() - prefill[o:o + k].double()
        errs[n] = float((got - ref.flatten()).abs().max() / ref.abs().max())
    assert max(errs.values()) <= 1e-4, errs
    for n, (o, k) in m.arena.slices.items():            # frozen weights: the prefill untouched
        if n not in want:
            assert torch.equal(g1[o:o + k], prefill[o:o + k]), n
    report("deferred reductions (rel to fp64)", **errs)


# ----------------------------------------------------------------------------- bias + GELU / ReLU
@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("rows,dtype", [(28224, BF16), (5120, BF16), (5120, torch.float32)])
def test_bias_activation_at_bench_shapes(ops, act, rows, dtype):
    """bevbert_bias_{gelu,relu}_fwd / _bwd at the FFN shapes of the bench (28 224 rows reach the capped-block branch of
    colwise_bwd_kernel) against fp64 erf-GELU / ReLU and their derivatives; for bf16 GELU, bias_gelu_fwd8_kernel against
    its 4-wide fallback (taken for an input that is not 16-byte aligned), bit for bit."""
    C = 3072
    rnd = _gen(rows + (act == "gelu"))
    x = (2 * rnd(rows, C)).to(dtype).requires_grad_(True)
    bias = rnd(C).requires_grad_(True)
    fn = ops.bias_gelu if act == "gelu" else ops.bias_relu
    y = fn(x, bias)
    dy = rnd(rows, C).to(dtype)
    y.backward(dy)
    t = x.detach().double() + bias.detach().double()
    yr = _gelu64(t) if act == "gelu" else torch.relu(t)
    dxr = dy.double() * (_dgelu64(t) if act == "gelu" else (t > 0).double())
    if dtype == BF16:
        errs = {"y": bf16_rounding_ratio(y, yr), "dx": bf16_rounding_ratio(x.grad, dxr)}
    else:       # fp32 arithmetic: a few ulp
        ratio = lambda g, r: float(((g.double() - r).abs() / (2.0 ** -20 * r.abs() + 1e-6 * float(r.abs().max()))).max())
        errs = {"y": ratio(y, yr), "dx": ratio(x.grad, dxr)}
    errs["dbias"] = rel_err(bias.grad, dxr.sum(0))
    assert errs["y"] <= 1.0 and errs["dx"] <= 1.0 and errs["dbias"] <= 1e-4, errs
    if act == "gelu" and dtype == BF16:
        buf = torch.empty(rows * C + 4, dtype=BF16, device=DEV)
        xv = buf[4:].view(rows, C)                       # 8-byte storage offset: not 16-byte aligned
        xv.copy_(x.detach())
        assert x.data_ptr() % 16 == 0 and xv.data_ptr() % 16 == 8
        with torch.no_grad():
            y4 = ops.bias_gelu(xv, bias.detach())
        assert torch.equal(y4, y.detach()), "bias_gelu_fwd8_kernel and the 4-wide kernel disagree"
    report(f"bias {act} rows={rows} {dtype}", **errs)
