"""The float16 operand mode of the CLIP image encoder on the GPU (csrc/vit.hip instantiated for _Float16, fp16 library GEMMs,
csrc/attn_fwd2.hip; clip_vit.py finalize(compute_dtype=torch.float16)): the row kernels against torch / fp64 math, the model
against the reference's recorded outputs within the project's factor of the reference's OWN fp16 error
(tests/golden/clip_vit.npz; tests/test_clip_vit_f16_host.py derives what to expect), capture, and the hand-over of an fp16
encoder's outputs to the fp32 / bf16 predictor.  Every figure is printed before it is asserted.

Tolerance of an fp16 result, per element: half an fp16 ulp of the fp64 value (2^-25 below 2^-14) -- the one rounding of the
store -- plus what the existing fp32 test of the same kernel allows its fp32 arithmetic (tests/test_gpu_clip_vit.py)."""
import numpy as np
import pytest
import torch

from tests import clip_ref as R
from tests.attn_f16_cases import half_ulp16
from tests.test_gpu_clip_vit import DEV, GOLDEN, LN_TOL, _ln64, _params      # noqa: F401  (the fp32 test's tolerances and inputs)
from tests.test_gpu_model import RES32_FACTOR, _record
from vln_bevbert_amd import clip_vit as V
from vln_bevbert_amd import ops_gemm

pytestmark = pytest.mark.gpu
F16 = torch.float16
LN32 = LN_TOL[torch.float32]
QG32 = 1e-6                 # test_bias_quickgelu_against_fp64_with_large_arguments: 1e-6 max(1, |y|)


@pytest.fixture(scope="module")
def gold():
    import os
    return np.load(os.path.join(GOLDEN, "clip_vit.npz"))


_MODELS = {}


def _model(case, max_images=None):
    cfg, n, _ = R.CASES[case]
    key = (case, max_images or n)
    if key not in _MODELS:
        m = V.ClipVisionTransformer(*cfg)
        m.load_state_dict(R.state_dict(cfg), strict=True)
        _MODELS[key] = m.finalize(DEV, F16, max_images or n)
    return _MODELS[key]


def _worst_f16(got, want, tol32):
    """Largest |got - want| / (half an fp16 ulp of want + tol32) over the elements; want fp64, tol32 a number or a tensor."""
    return float(((got.double().cpu() - want.cpu()).abs() / (half_ulp16(want.cpu()) + tol32)).max())


# ------------------------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("P", [16, 32])
@pytest.mark.parametrize("N", [1, 25])
def test_patchify_fp16_is_bit_equal_to_the_torch_transform_and_unfold(N, P, mapped):
    n_src = N + 3 if mapped else N
    u8 = R.images(7 + N + P, n_src)
    vmap = torch.tensor([(5 * i + 2) % n_src for i in range(N)], dtype=torch.int32) if mapped else None
    want = R.unfold(R.transform(u8 if vmap is None else u8[vmap.long()]), P).to(F16)
    got = V.patchify(u8.to(DEV), P, F16, None if vmap is None else vmap.to(DEV)).cpu()
    diff = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"patchify fp16 N={N} P={P} mapped={mapped}: {diff} of {got.numel()} values differ")
    assert got.dtype == F16 and got.shape == (N * (224 // P) ** 2, 3 * P * P) and diff == 0


# ------------------------------------------------------------------------------------------------ QuickGELU
@pytest.mark.parametrize("C", [768, 3072])
@pytest.mark.parametrize("rows", [1, 197])
def test_bias_quickgelu_fp16_against_fp64_large_arguments_and_overflow(rows, C):
    gen = torch.Generator().manual_seed(rows + C)
    x = 3 * torch.randn(rows, C, generator=gen)
    bias = 0.5 * torch.randn(C, generator=gen)
    special = torch.tensor([30.0, -30.0, 1e4, -1e4, 0.0, 65504.0, -65504.0, 60000.0])
    bias[:8] = torch.tensor([0, 0, 0, 0, 0, 1000.0, -1000.0, 6000.0])      # t = 66504, -66504, 66000: beyond fp16's 65504
    x[0, :8] = special
    x[rows - 1, :8] = special
    x = x.to(F16)
    got = V.bias_quickgelu(x.to(DEV), bias.to(DEV)).cpu()
    t = x.double() + bias.double()
    want = t * torch.sigmoid(1.702 * t)
    over = want.abs() >= 65520.0                    # rounds to inf in fp16 (nearest even past the largest finite number)
    assert got.dtype == F16 and int(over.sum()) == 2 * (1 if rows == 1 else 2)
    assert bool(torch.isinf(got[over]).all()) and bool((got[over] > 0).all()), "overflow goes to +inf as IEEE fp16 does"
    assert bool(torch.isfinite(got[~over]).all())
    ratio = _worst_f16(got[~over], want[~over], QG32 * want[~over].abs().clamp_min(1))
    print(f"quickgelu fp16 rows={rows} C={C}: worst error / (half an fp16 ulp + 1e-6 max(1, |y|)) = {ratio:.3f}")
    assert ratio <= 1.0
    assert float(got[0, 2]) == 1e4 and float(got[0, 3]) == 0.0 and float(got[0, 4]) == 0.0 and float(got[0, 6]) == 0.0


# ------------------------------------------------------------------------------------------------ residual + LayerNorm
@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("rows", [1, 197])
def test_bias_residual_prenorm_fp16_against_fp64(rows, H):
    gen = torch.Generator().manual_seed(rows * 7 + H)
    z0 = (2 * torch.randn(rows, H, generator=gen)).to(DEV)
    x = torch.randn(rows, H, generator=gen).to(F16).to(DEV)
    ((g, b),), (bias,) = _params(H, gen, 1)
    z32 = z0.clone()
    y = V.bias_residual_prenorm(z32, x, bias, g, b)
    zr = z0.double() + (x.double() + bias.double())
    ez, ry = float((z32.double() - zr).abs().max()), _worst_f16(y, _ln64(zr, g, b), LN32)
    print(f"bias_residual_prenorm fp16 rows={rows} H={H}: z32 err {ez:.2e}, y err / (half an fp16 ulp + {LN32}) = {ry:.3f}")
    assert z32.dtype == torch.float32 and y.dtype == F16
    assert ez < LN32 and ry <= 1.0


@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("N,L", [(1, 2), (3, 197)])
def test_bias_residual_final_form_fp16(N, L, H):
    gen = torch.Generator().manual_seed(N * 1000 + L + H)
    rows = N * L
    z0 = (2 * torch.randn(rows, H, generator=gen)).to(DEV)
    x = torch.randn(rows, H, generator=gen).to(F16).to(DEV)
    ((g, b),), (bias,) = _params(H, gen, 1)
    z32 = z0.clone()
    x_patch, cls = V.bias_residual_final(z32, x, bias, g, b, L)
    zr = (z0.double() + (x.double() + bias.double())).view(N, L, H)
    ep, rc = float((x_patch.double() - zr[:, 1:]).abs().max()), _worst_f16(cls, _ln64(zr[:, 0], g, b), LN32)
    print(f"final form fp16 N={N} L={L} H={H}: x_patch err {ep:.2e}, class rows err / (half an fp16 ulp + {LN32}) = {rc:.3f}")
    assert x_patch.shape == (N, L - 1, H) and x_patch.dtype == torch.float32 and cls.shape == (N, H) and cls.dtype == F16
    assert ep < LN32 and rc <= 1.0
    assert torch.equal(z32, z0), "the final form leaves the stream as it was"


@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("N,L", [(1, 2), (3, 197)])
def test_embed_prenorm_fp16_against_fp64(N, L, H):
    gen = torch.Generator().manual_seed(N * 100 + L + H)
    conv = torch.randn(N * (L - 1), H, generator=gen).to(F16).to(DEV)
    cls = (0.5 * torch.randn(H, generator=gen)).to(DEV)
    pos = (0.5 * torch.randn(L, H, generator=gen)).to(DEV)
    (pre, ln1), _ = _params(H, gen, 2)
    z32, y = V.embed_prenorm(conv, cls, pos, pre, ln1, L)
    tok = torch.cat([cls.double().expand(N, 1, H), conv.double().view(N, L - 1, H)], 1) + pos.double()
    zr = _ln64(tok, *pre).view(N * L, H)
    ez, ry = float((z32.double() - zr).abs().max()), _worst_f16(y, _ln64(zr, *ln1), LN32)
    print(f"embed_prenorm fp16 N={N} L={L} H={H}: z32 err {ez:.2e}, y err / (half an fp16 ulp + {LN32}) = {ry:.3f}")
    assert z32.dtype == torch.float32 and y.dtype == F16 and z32.shape == (N * L, H)
    assert ez < LN32 and ry <= 1.0


def test_row_kernel_wrappers_refuse_mismatched_dtypes_with_fp16_too():
    H, rows = 256, 8
    z32, x = torch.zeros(rows, H, device=DEV), torch.zeros(rows, H, device=DEV, dtype=F16)
    v = torch.zeros(H, device=DEV)
    assert V.bias_residual_prenorm(z32, x, v, v, v).dtype == F16
    for bad in (dict(z32=z32.half()), dict(x=torch.zeros(rows, 2 * H, device=DEV, dtype=F16)[:, ::2]), dict(gamma=v.half()),
                dict(y=torch.zeros(rows, H, device=DEV)), dict(y=torch.zeros(rows, H, device=DEV, dtype=torch.bfloat16))):
        with pytest.raises(ValueError):
            V.bias_residual_prenorm(**{**dict(z32=z32, x=x, bias=v, gamma=v, beta=v), **bad})
    with pytest.raises(ValueError):
        V.bias_residual_final(z32, x, v, v, v, 4, x_patch=torch.zeros(2, 3, H, device=DEV, dtype=F16))
    with pytest.raises(ValueError):
        V.bias_residual_final(z32, x, v, v, v, 4, cls_out=torch.zeros(2, H, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        V.bias_quickgelu(x, v.half())
    with pytest.raises(ValueError):
        V.bias_quickgelu(x, v, out=x.bfloat16())
    with pytest.raises(ValueError):
        V.embed_prenorm(x[:6], v, torch.zeros(4, H, device=DEV), (v, v), (v, v), 4, y=torch.zeros(8, H, device=DEV))
    with pytest.raises(ValueError):
        V.ClipVisionTransformer(*R.CASES["b32_l2"][0]).finalize(DEV, torch.float64)


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("case", list(R.CASES))
def test_model_fp16_operands_within_the_references_own_float16_error(gold, case):
    cfg, n, seed = R.CASES[case]
    m = _model(case)
    before = dict(ops_gemm.GEMM_FALLBACKS)
    with torch.no_grad():
        x, xp = m.encode_u8(R.images(seed, n, cfg[0]).to(DEV))
    assert dict(ops_gemm.GEMM_FALLBACKS) == before, "a GEMM of the fp16 encoder went through torch"
    assert x.dtype == F16 and xp.dtype == torch.float32
    assert x.shape == (n, cfg[5]) and xp.shape == (n, (cfg[0] // cfg[1]) ** 2, cfg[2])
    cols, toks = R.sample(xp)
    worst = 0.0
    for k, v in (("x", x), ("xp_cols", cols), ("xp_toks", toks)):
        err, own = R.rel_l2(v.float().cpu().numpy(), gold[f"{case}_{k}"]), float(gold[f"{case}_fp16_rel_l2_{k}"])
        print(f"{case} fp16 {k}: rel-L2 {err:.3e}, reference's own float16 {own:.3e}, ratio {err / own:.2f}, gate {RES32_FACTOR}")
        _record("clip_vit_f16", f"{case}.{k}", rel_l2=err, ref_own_fp16=own, ratio=err / own)
        worst = max(worst, err / own)
    assert worst <= RES32_FACTOR


def test_forward_on_normalised_floats_and_the_encoder_wrapper_take_fp16(gold):
    cfg, n, seed = R.CASES["b16_l2"]
    enc = V.ClipRGBEncoder(*cfg)
    enc.load_clip_state_dict({"visual." + k: v for k, v in R.state_dict(cfg).items()})
    enc.finalize(DEV, F16, n)
    vec, grid = enc({"rgb": R.images(seed, n, cfg[0]).to(DEV)})
    assert vec.dtype == torch.float32 and grid.dtype == torch.float32
    x2, xp2 = enc.model.visual(R.transform(R.images(seed, n, cfg[0])).to(DEV))
    assert x2.dtype == F16 and xp2.dtype == torch.float32
    assert torch.equal(x2.float(), vec) and torch.equal(xp2, grid), "the u8 kernel and the torch transform round to the same fp16 rows"
    own = float(gold["b16_l2_fp16_rel_l2_x"])
    assert R.rel_l2(vec.cpu().numpy(), gold["b16_l2_x"]) <= RES32_FACTOR * own
    enc.load_clip_state_dict({"visual." + k: v for k, v in R.state_dict(cfg).items()})
    with pytest.raises(RuntimeError, match="finalize"):
        enc({"rgb": R.images(seed, n, cfg[0]).to(DEV)})


# ------------------------------------------------------------------------------------------------ panorama
def test_encode_panorama_hands_an_fp16_encoders_outputs_to_the_fp32_predictor_and_the_map():
    from vln_bevbert_amd import waypoint as W
    from vln_bevbert_amd.ce_map import CEGraphMap
    from tests import waypoint_ref as WR
    B = 2
    cfg = R.CASES["b16_l2"][0]
    m = _model("b16_l2", B * 12)
    u8 = R.images(55, B * 12, cfg[0])
    gen = torch.Generator().manual_seed(5)
    depth = torch.rand(B, 12, 64, 64, 1, generator=gen) * 0.45 + 0.05
    rgb_embeds, rgb_grid, depth_grid = V.encode_panorama(m, u8.view(B, 12, 224, 224, 3).to(DEV), depth.to(DEV))
    assert rgb_embeds.shape == (B * 12, 512) and rgb_grid.shape == (B, 12, 196, 768) and depth_grid.shape == (B, 12, 14, 14)
    assert rgb_embeds.dtype == torch.float32 and rgb_grid.dtype == torch.float32 and depth_grid.dtype == torch.float32
    assert rgb_embeds.is_contiguous() and rgb_grid.is_contiguous()
    # the reference re-orders the images first and encodes them in that order; the widening is exact
    x_by_hand, xp_by_hand = m.encode_u8(R.clockwise(u8, B).to(DEV))
    assert x_by_hand.dtype == F16
    assert torch.equal(rgb_embeds, x_by_hand.float()) and torch.equal(rgb_grid.view(B * 12, 196, 768), xp_by_hand)
    assert not torch.equal(rgb_embeds[1], rgb_embeds[11])
    as_bf16 = V.encode_panorama(m, u8.view(B, 12, 224, 224, 3).to(DEV), depth.to(DEV), embeds_dtype=torch.bfloat16)[0]
    assert as_bf16.dtype == torch.bfloat16 and torch.equal(as_bf16, x_by_hand.to(torch.bfloat16))
    as_f16 = V.encode_panorama(m, u8.view(B, 12, 224, 224, 3).to(DEV), depth.to(DEV), embeds_dtype=F16)[0]
    assert as_f16.dtype == F16 and torch.equal(as_f16, x_by_hand)
    # handed on unchanged to an fp32 predictor step and to the map
    dep_embeds = torch.from_numpy(WR.synthetic(71, (B * 12, 128, 4, 4))).to(DEV, torch.float32)
    logits = torch.from_numpy(WR.synthetic(72, (B, 12, 120))).to(DEV)
    wp = W.waypoint_step(None, rgb_embeds, dep_embeds, cls_logits=logits)
    assert wp["pano_rgb"].dtype == torch.float32 and wp["vp_inputs"]["rgb_fts"].dtype == torch.float32
    assert torch.equal(wp["pano_rgb"][:, 0], rgb_embeds.view(B, 12, 512)[:, 0]) and int(wp["cand_count"].min()) >= 1
    cm = CEGraphMap(B, 32, DEV, loc_noise=0.5)
    vp = wp["vp_inputs"]
    pano = torch.randn(B, vp["nav_types"].shape[1], 32, generator=gen).to(DEV)
    cm.update(1, wp["cand_count"], wp["cand_angles"], wp["cand_distances"], pano.mean(1), pano, vp["nav_types"],
              cur_pos=np.array([[0.0, 0.0, 0.0], [5.0, 1.0, -2.0]]), heading=np.array([0.4, 2.0]))
    cm.remember_pano(rgb_grid, depth_grid)
    for b in range(B):
        assert torch.equal(cm.store["rgb"][b * cm.N].view(12, 196, 768), rgb_grid[b])
        assert torch.equal(cm.store["depth"][b * cm.N], depth_grid[b])


# ------------------------------------------------------------------------------------------------ capture, determinism
@pytest.mark.parametrize("N", [1, 12])
def test_captured_fp16_encoder_equals_eager_bit_for_bit_and_nothing_synchronises(N):
    cfg = R.CASES["b16_l2"][0]
    m = _model("b16_l2", 12)
    u8a, u8b = R.images(60 + N, N, cfg[0]).to(DEV), R.images(70 + N, N, cfg[0]).to(DEV)
    for _ in range(2):                                   # GEMM plans, workspaces
        m.encode_u8(u8a)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = m.encode_u8(u8a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    second = m.encode_u8(u8a)
    assert first[0].dtype == F16
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), "two eager runs differ"
    static = u8a.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.encode_u8(static)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        cap = m.encode_u8(static)
    static.copy_(u8b)
    g.replay()
    torch.cuda.synchronize()
    eager = m.encode_u8(u8b)
    assert torch.equal(eager[0], cap[0]) and torch.equal(eager[1], cap[1]), "replay differs from eager"
    assert not torch.equal(eager[0], first[0])
