"""CPU: what the float16 operand mode of the CLIP image encoder (clip_vit.py finalize(compute_dtype=torch.float16),
csrc/attn_fwd2.hip) has to achieve, from an emulation of exactly its arithmetic, and the conditions the GPU tests lean on.

The emulation is tests/clip_ref.py's forward with the data flow of clip_vit._encode_patches: GEMM and attention operands and
every stored activation rounded to the compute dtype, products summed in fp32, the residual stream, the LayerNorms, QuickGELU
and the softmax statistics in fp32, P rounded before the P V product and the row sum taken over the unrounded P.  Run with
bfloat16 it gives 0.66 .. 0.75 of the reference's own bfloat16 error, where the GPU's bf16 mode measures 0.61 .. 0.75: it is
a model of the device path.  With float16 (figures of this file, printed by the tests):

    case     x      xp_cols  xp_toks     (emulated rel-L2 / the reference's own fp16 rel-L2, tests/golden/clip_vit.npz)
    b16_l2   0.63   0.70     0.69
    b32_l2   0.70   0.77     0.75
    last key of every softmax left out: 6.2 .. 53 times the reference's own error

Attention (tests/attn_f16_cases.py holds inputs, bound and the emulation of the kernel): on the GPU test's inputs the
emulation needs at most 0.42 of the C16 = 4 units of the per-element bound (15 x 15; 0.12 at 577 x 577); a dropped key at a
tile edge leaves the bound by a factor of at least 5.8, a duplicated one by at least 9.5, a misplaced v row by at least 5.5
(worst element over the output, smallest over the edges of the shapes tried -- all three at 1 x 197, where one row has to
show it; 21 and more at 577 x 577, 36 and more at the encoder's 197 x 197)."""
import os

import numpy as np
import pytest
import torch

from tests import attn_f16_cases as AC
from tests import clip_ref as R
from tests.test_gpu_model import RES32_FACTOR       # the project's factor over the reference's own reduced-precision error

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("x", "xp_cols", "xp_toks")
EMULATED_CASES = ("b16_l2", "b32_l2")               # b16_l12 (12 blocks, 12 images) is the GPU test's; minutes on the CPU


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "clip_vit.npz"))


def emulated_forward(sd, cfg, u8, dtype, drop_last_key=False):
    """(x, x_patch) of the device path with ``dtype`` operands, on the CPU in fp32."""
    Rr, P, W, layers, heads, _ = cfg
    f = torch.float32

    def r(t):                                        # a stored activation / an operand: rounded to the compute dtype
        return t.to(dtype).to(f)
    w = {k: (r(v) if v.dim() >= 2 and not k.startswith("positional") or "in_proj_bias" in k else v.to(f)) for k, v in sd.items()}
    N = u8.shape[0]
    L = (Rr // P) ** 2 + 1
    conv = r(r(R.unfold(R.transform(u8), P)) @ w["conv1.weight"].reshape(W, -1).t())
    z = torch.cat([w["class_embedding"].expand(N, 1, W), conv.view(N, L - 1, W)], 1) + w["positional_embedding"]
    z = R._ln(z, w["ln_pre.weight"], w["ln_pre.bias"])
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        y = r(R._ln(z, w[p + "ln_1.weight"], w[p + "ln_1.bias"]))
        qkv = r(y @ w[p + "attn.in_proj_weight"].t() + w[p + "attn.in_proj_bias"])
        q, k, v = (t.view(N, L, heads, W // heads).transpose(1, 2) for t in qkv.split(W, -1))
        s = q @ k.transpose(-1, -2) / (W // heads) ** 0.5
        if drop_last_key:
            s[..., -1] = float("-inf")
        e = torch.exp(s - s.amax(-1, keepdim=True))
        a = r((r(e) @ v) / e.sum(-1, keepdim=True)).transpose(1, 2).reshape(N, L, W)
        z = z + (r(a @ w[p + "attn.out_proj.weight"].t()) + w[p + "attn.out_proj.bias"])
        y = r(R._ln(z, w[p + "ln_2.weight"], w[p + "ln_2.bias"]))
        t = r(R.quickgelu(r(y @ w[p + "mlp.c_fc.weight"].t()) + w[p + "mlp.c_fc.bias"]))
        z = z + (r(t @ w[p + "mlp.c_proj.weight"].t()) + w[p + "mlp.c_proj.bias"])
    cls = r(R._ln(z[:, 0], w["ln_post.weight"], w["ln_post.bias"]))
    return r(cls @ w["proj"]), z[:, 1:]


_RATIOS = {}


def _ratios(gold, case, dtype, drop_last_key=False):
    key = (case, dtype, drop_last_key)
    if key not in _RATIOS:
        cfg, n, seed = R.CASES[case]
        with torch.no_grad():
            x, xp = emulated_forward(R.state_dict(cfg), cfg, R.images(seed, n, cfg[0]), dtype, drop_last_key)
        cols, toks = R.sample(xp)
        own = "fp16" if dtype == torch.float16 else "bf16"
        _RATIOS[key] = {name: R.rel_l2(got.numpy(), gold[f"{case}_{name}"]) / float(gold[f"{case}_{own}_rel_l2_{name}"])
                        for name, got in zip(NAMES, (x, cols, toks))}
    return _RATIOS[key]


@pytest.mark.parametrize("case", EMULATED_CASES)
def test_emulated_fp16_operand_error_is_within_the_factor_of_the_references_own_fp16_error(gold, case):
    ratios = _ratios(gold, case, torch.float16)
    print(f"{case} fp16-operand emulation: rel-L2 / reference's own fp16 rel-L2 "
          + " ".join(f"{k}={v:.2f}" for k, v in ratios.items()) + f", gate {RES32_FACTOR}")
    assert max(ratios.values()) <= RES32_FACTOR


@pytest.mark.parametrize("case", EMULATED_CASES)
def test_emulation_without_the_last_key_leaves_the_gate(gold, case):
    """What the model gate on the GPU can see: one key dropped from every softmax (a wrong tail tile)."""
    ratios = _ratios(gold, case, torch.float16, drop_last_key=True)
    print(f"{case} fp16-operand emulation without the last key: " + " ".join(f"{k}={v:.1f}" for k, v in ratios.items())
          + f", gate {RES32_FACTOR}")
    assert max(ratios.values()) > RES32_FACTOR


def test_emulation_with_bfloat16_reproduces_the_measured_device_ratios(gold):
    """The bf16 mode measures 0.61 .. 0.75 of the reference's own bfloat16 error on the MI355X; the emulation
    has to land in the same place to count as a model of the device path: within 0.5 .. 1.0."""
    ratios = _ratios(gold, "b32_l2", torch.bfloat16)
    print("b32_l2 bf16-operand emulation: " + " ".join(f"{k}={v:.2f}" for k, v in ratios.items()))
    assert 0.5 <= min(ratios.values()) and max(ratios.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ attention
_REF = {}


def _ref(Lq, Lk, nh):
    if (Lq, Lk, nh) not in _REF:
        q, k, v = AC.make_inputs(Lq, Lk, nh)
        _REF[(Lq, Lk, nh)] = (q, k, v) + AC.reference64(q, k, v)
    return _REF[(Lq, Lk, nh)]


SHAPES = sorted({c[:3] for c in AC.cases()})


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-nh{s[2]}")
def test_attention_inputs_keep_every_probability_a_normal_fp16_number(shape):
    """Condition of the bound (no flush term): p / row maximum >= 2^-12 on every row of every case of the GPU test."""
    floor = _ref(*shape)[5]
    print(f"attn-f16 inputs {shape}: smallest probability / row maximum = 2^{np.log2(floor):.2f}")
    assert floor >= AC.P_FLOOR


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-nh{s[2]}")
def test_emulated_kernel_arithmetic_holds_the_per_element_bound(shape):
    q, k, v, o64, b_o, _ = _ref(*shape)
    got = AC.emulate(q, k, v)
    need = AC.units(got, o64, b_o)
    print(f"attn-f16 emulation {shape}: {need:.3f} of C16 = {AC.C16} units")
    assert bool(((got.double() - o64).abs() <= AC.bound(o64, b_o)).all())
    assert need <= 1.0, "P rounds once to fp16: ONE unit of 2^-11 sum p |v| is all an exact-fp32 kernel may use"


@pytest.mark.parametrize("shape", [(65, 65, 2), (129, 129, 2), (197, 197, 2), (65, 130, 2), (1, 197, 2), (577, 577, 2)],
                         ids=lambda s: f"{s[0]}x{s[1]}-nh{s[2]}")
def test_one_wrong_key_at_a_tile_edge_breaks_the_bound(shape):
    """A dropped, a duplicated and a misplaced key at every tile edge: the worst element leaves the bound, by the factors in
    the module docstring."""
    q, k, v, o64, b_o, _ = _ref(*shape)
    gate = AC.bound(o64, b_o)
    least = {}
    for kind in ("drop", "dup", "swap_v"):
        for j in AC.boundary_keys(shape[1]):
            over = float(((AC.emulate(q, k, v, **{kind: j}).double() - o64).abs() / gate).max())
            least[kind] = min(least.get(kind, float("inf")), over)
            assert over > 2.0, (kind, j, over)
    print(f"attn-f16 mutations {shape}: smallest worst-element error / bound " + " ".join(f"{n}={x:.1f}" for n, x in least.items()))
