"""csrc/vit.hip + vln_bevbert_amd/clip_vit.py on the GPU: the five kernels against torch / fp64 math, the model against the
reference's recorded outputs (tests/golden/clip_vit.npz, made by tests/golden/make_clip_vit_golden.py) in fp32 and with
bf16 operands, the state_dict / encoder interface, encode_panorama's view order and its hand-over to waypoint_step and
CEGraphMap.remember_pano, and capture / determinism / no host synchronisation.  Every figure is printed before it is
asserted."""
import os

import numpy as np
import pytest
import torch

from tests import clip_ref as R
from tests.helpers import read_shapes
from tests.test_gpu_model import RES32_FACTOR, _record      # the project's fp32-stream factor and its bf16 error log
from vln_bevbert_amd import clip_vit as V

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
FP32_GATE = 1e-3        # max-abs / absmax: the project's fp32 gate
LN_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}     # test_gpu_kernels.py::test_layernorm_fwd_bwd, forward


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "clip_vit.npz"))


_MODELS = {}


def _model(case, dtype, max_images=None):
    cfg, n, _ = R.CASES[case]
    key = (case, dtype, max_images or n)
    if key not in _MODELS:
        m = V.ClipVisionTransformer(*cfg)
        m.load_state_dict(R.state_dict(cfg), strict=True)
        _MODELS[key] = m.finalize(DEV, dtype, max_images or n)
    return _MODELS[key]


def _ln64(z, g, b, eps=1e-5):
    return torch.nn.functional.layer_norm(z.double(), (z.shape[-1],), g.double(), b.double(), eps)


def _params(H, gen, n):
    """n (gamma, beta) pairs and n bias-like vectors of width H, fp32, on the device."""
    gb = [((1 + 0.1 * torch.randn(H, generator=gen)).to(DEV), (0.1 * torch.randn(H, generator=gen)).to(DEV)) for _ in range(n)]
    return gb, [(0.1 * torch.randn(H, generator=gen)).to(DEV) for _ in range(n)]


# ------------------------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("P", [16, 32])
@pytest.mark.parametrize("N", [1, 25])
def test_patchify_is_bit_equal_to_the_torch_transform_and_unfold(N, P, mapped):
    """With a view map the N output images are drawn from N + 3 inputs in a scrambled order (for N = 1 the map still
    picks another image than the first)."""
    n_src = N + 3 if mapped else N
    u8 = R.images(7 + N + P, n_src)
    vmap = torch.tensor([(5 * i + 2) % n_src for i in range(N)], dtype=torch.int32) if mapped else None
    want = R.unfold(R.transform(u8 if vmap is None else u8[vmap.long()]), P)
    for dtype in (torch.float32, torch.bfloat16):
        got = V.patchify(u8.to(DEV), P, dtype, None if vmap is None else vmap.to(DEV)).cpu()
        diff = int((got != want.to(dtype)).sum())
        print(f"patchify N={N} P={P} mapped={mapped} {dtype}: {diff} of {got.numel()} values differ")
        assert got.shape == (N * (224 // P) ** 2, 3 * P * P) and diff == 0


def test_patchify_refuses_what_it_cannot_take():
    with pytest.raises(ValueError):
        V.patchify(torch.zeros(1, 224, 224, 3, device=DEV), 16, torch.float32)
    with pytest.raises(ValueError):
        V.patchify(torch.zeros(1, 224, 224, 3, dtype=torch.uint8, device=DEV), 14, torch.float32)


# ------------------------------------------------------------------------------------------------ QuickGELU
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [768, 3072])
@pytest.mark.parametrize("rows", [197, 591])
def test_bias_quickgelu_against_fp64_with_large_arguments(rows, C, dtype):
    gen = torch.Generator().manual_seed(rows + C)
    x = 3 * torch.randn(rows, C, generator=gen)
    bias = 0.5 * torch.randn(C, generator=gen)
    special = torch.tensor([30.0, -30.0, 1e4, -1e4, 0.0])
    bias[:5] = 0                                            # t = x + bias is the special value itself
    x[0, :5], x[rows - 1, :5], x[rows // 2, :5] = special, special, special
    x = x.to(dtype)
    got = V.bias_quickgelu(x.to(DEV), bias.to(DEV)).cpu()
    t = x.double() + bias.double()
    want = t * torch.sigmoid(1.702 * t)
    assert got.dtype == dtype and bool(torch.isfinite(got).all()), "QuickGELU produced a non-finite value"
    err = (got.double() - want).abs()
    if dtype == torch.float32:
        ratio = float((err / (1e-6 * want.abs().clamp_min(1))).max())
        print(f"quickgelu fp32 rows={rows} C={C}: worst error / (1e-6 max(1, |y|)) = {ratio:.3f}")
    else:       # one bf16 ulp of the fp64 value: 2^(exponent - 7)
        ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 7)
        ratio = float((err / ulp).max())
        print(f"quickgelu bf16 rows={rows} C={C}: worst error {ratio:.3f} bf16 ulp")
    assert ratio <= 1.0
    assert float(got[0, 2]) == float(x[0, 2]) and float(got[0, 3]) == 0.0 and float(got[0, 4]) == 0.0


# ------------------------------------------------------------------------------------------------ residual + LayerNorm
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("rows", [1, 197, 591])
def test_bias_residual_prenorm_against_fp64(rows, H, dtype):
    gen = torch.Generator().manual_seed(rows * 7 + H)
    z0 = (2 * torch.randn(rows, H, generator=gen)).to(DEV)
    x = torch.randn(rows, H, generator=gen).to(dtype).to(DEV)
    ((g, b),), (bias,) = _params(H, gen, 1)
    z32 = z0.clone()
    y = V.bias_residual_prenorm(z32, x, bias, g, b)
    zr = z0.double() + (x.double() + bias.double())
    ez, ey = float((z32.double() - zr).abs().max()), float((y.double() - _ln64(zr, g, b)).abs().max())
    print(f"bias_residual_prenorm rows={rows} H={H} {dtype}: z32 err {ez:.2e}, y err {ey:.2e}")
    assert z32.dtype == torch.float32 and y.dtype == dtype
    assert ez < LN_TOL[torch.float32] and ey < LN_TOL[dtype]


@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("rows", [1, 5, 9])
def test_bias_residual_prenorm_gives_the_bits_of_the_plain_layernorm(rows, H):
    """The ViT kernel and ln_fwd_kernel share one row body (ln_row_stats / ln_norm4): on the z32 the ViT kernel leaves,
    ops.layernorm gives the same fp32 bits, and for bf16 operands their bf16 rounding."""
    from vln_bevbert_amd import ops
    gen = torch.Generator().manual_seed(rows * 11 + H)
    z0 = (2 * torch.randn(rows, H, generator=gen)).to(DEV)
    x32 = torch.randn(rows, H, generator=gen).to(DEV)
    ((g, b),), (bias,) = _params(H, gen, 1)
    for x in (x32, x32.to(torch.bfloat16)):
        z32 = z0.clone()
        y = V.bias_residual_prenorm(z32, x, bias, g, b)
        plain = ops.layernorm(z32, g, b, V.LN_EPS)
        assert plain.dtype == torch.float32 and y.dtype == x.dtype
        assert torch.equal(y, plain.to(x.dtype)), (rows, H, x.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("N,L", [(1, 197), (3, 197), (2, 50)])
def test_bias_residual_final_form_skips_class_rows_and_normalises_them_only(N, L, H, dtype):
    gen = torch.Generator().manual_seed(N * 1000 + L + H)
    rows = N * L
    z0 = (2 * torch.randn(rows, H, generator=gen)).to(DEV)
    x = torch.randn(rows, H, generator=gen).to(dtype).to(DEV)
    ((g, b),), (bias,) = _params(H, gen, 1)
    z32 = z0.clone()
    x_patch, cls = V.bias_residual_final(z32, x, bias, g, b, L)
    zr = (z0.double() + (x.double() + bias.double())).view(N, L, H)
    ep = float((x_patch.double() - zr[:, 1:]).abs().max())
    ec = float((cls.double() - _ln64(zr[:, 0], g, b)).abs().max())
    print(f"final form N={N} L={L} H={H} {dtype}: x_patch err {ep:.2e}, class rows (ln_post) err {ec:.2e}")
    assert x_patch.shape == (N, L - 1, H) and x_patch.dtype == torch.float32 and cls.shape == (N, H) and cls.dtype == dtype
    assert ep < LN_TOL[torch.float32] and ec < LN_TOL[dtype]
    assert torch.equal(z32, z0), "the final form leaves the stream as it was"
    # the patch rows are NOT normalised: their row means are those of the stream
    assert float((x_patch.double().mean(-1) - zr[:, 1:].mean(-1)).abs().max()) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("N,L", [(1, 2), (1, 197), (3, 197)])
def test_embed_prenorm_against_fp64(N, L, H, dtype):
    """Rows 2, 197, 591: an image has its class row and at least one patch row, so one row alone does not occur."""
    gen = torch.Generator().manual_seed(N * 100 + L + H)
    conv = torch.randn(N * (L - 1), H, generator=gen).to(dtype).to(DEV)
    cls = (0.5 * torch.randn(H, generator=gen)).to(DEV)
    pos = (0.5 * torch.randn(L, H, generator=gen)).to(DEV)
    (pre, ln1), _ = _params(H, gen, 2)
    z32, y = V.embed_prenorm(conv, cls, pos, pre, ln1, L)
    tok = torch.cat([cls.double().expand(N, 1, H), conv.double().view(N, L - 1, H)], 1) + pos.double()
    zr = _ln64(tok, *pre).view(N * L, H)
    ez, ey = float((z32.double() - zr).abs().max()), float((y.double() - _ln64(zr, *ln1)).abs().max())
    print(f"embed_prenorm N={N} L={L} H={H} {dtype}: z32 err {ez:.2e}, y err {ey:.2e}")
    assert z32.dtype == torch.float32 and y.dtype == dtype and z32.shape == (N * L, H)
    assert ez < LN_TOL[torch.float32] and ey < LN_TOL[dtype]


# ------------------------------------------------------------------------------------------------ depth pooling
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("Hd", [256, 224, 15])
def test_depth_grid_pool_against_torch_adaptive_avg_pool(Hd, mapped):
    """Against F.adaptive_avg_pool2d on the CPU: 1e-6 relative to its float64 run, and to its float32 run with that run's
    own distance from the float64 one added (it sums a window one value after the other, which is itself up to 9e-7 off)."""
    N = 5
    gen = torch.Generator().manual_seed(Hd)
    depth = torch.rand(N, Hd, Hd, 1, generator=gen) * 0.95 + 0.05
    vmap = torch.tensor([3, 0, 4, 4, 1], dtype=torch.int32) if mapped else None
    src = depth if vmap is None else depth[vmap.long()]
    want = torch.nn.functional.adaptive_avg_pool2d(src.double().permute(0, 3, 1, 2), (14, 14))[:, 0]
    own = torch.nn.functional.adaptive_avg_pool2d(src.permute(0, 3, 1, 2), (14, 14))[:, 0]
    got = V.depth_grid_pool(depth.to(DEV), None if vmap is None else vmap.to(DEV)).cpu()
    err = float(((got.double() - want).abs() / want.abs()).max())
    own_err = float(((own.double() - want).abs() / want.abs()).max())
    err32 = float(((got.double() - own.double()).abs() / own.double().abs()).max())
    print(f"depth_grid_pool Hd={Hd} mapped={mapped}: relative error {err:.2e} against the float64 pool, {err32:.2e} against "
          f"the float32 pool (whose own distance from the float64 one is {own_err:.2e})")
    assert got.shape == (N, 14, 14) and err <= 1e-6 and err32 <= 1e-6 + own_err


# ------------------------------------------------------------------------------------------------ the model
def _run(case, dtype):
    cfg, n, seed = R.CASES[case]
    with torch.no_grad():
        x, xp = _model(case, dtype).encode_u8(R.images(seed, n, cfg[0]).to(DEV))
    cols, toks = R.sample(xp)
    return {"x": x.float().cpu().numpy(), "xp_cols": cols.float().cpu().numpy(), "xp_toks": toks.float().cpu().numpy()}, x, xp


@pytest.mark.parametrize("case", list(R.CASES))
def test_model_fp32_against_the_reference(gold, case):
    got, x, xp = _run(case, torch.float32)
    cfg, n, _ = R.CASES[case]
    assert x.shape == (n, cfg[5]) and xp.shape == (n, (cfg[0] // cfg[1]) ** 2, cfg[2]) and xp.dtype == torch.float32
    errs = {k: R.max_rel(v, gold[f"{case}_{k}"]) for k, v in got.items()}
    print(f"{case} fp32: max-abs / absmax {errs}")
    assert max(errs.values()) <= FP32_GATE


@pytest.mark.parametrize("case", list(R.CASES))
def test_model_bf16_operands_within_the_references_own_bfloat16_error(gold, case):
    got, x, xp = _run(case, torch.bfloat16)
    assert x.dtype == torch.bfloat16 and xp.dtype == torch.float32
    worst = 0.0
    for k, v in got.items():
        err, own = R.rel_l2(v, gold[f"{case}_{k}"]), float(gold[f"{case}_bf16_rel_l2_{k}"])
        print(f"{case} bf16 {k}: rel-L2 {err:.3e}, reference's own bfloat16 {own:.3e} (fp16 "
              f"{float(gold[f'{case}_fp16_rel_l2_{k}']):.3e}), ratio {err / own:.2f}, gate {RES32_FACTOR}")
        _record("clip_vit", f"{case}.{k}", rel_l2=err, ref_own_bf16=own, ratio=err / own)
        worst = max(worst, err / own)
    assert worst <= RES32_FACTOR


# ------------------------------------------------------------------------------------------------ interface
def test_state_dict_keys_and_the_encoder_interface(gold):
    cfg, n, seed = R.CASES["b16_l2"]
    assert [(k, tuple(v.shape)) for k, v in V.ClipVisionTransformer(*R.KEYS_CONFIG).state_dict().items()] == \
        list(read_shapes("clip_vit_keys.txt").items())
    enc = V.ClipRGBEncoder(*cfg)
    full = {"visual." + k: v for k, v in R.state_dict(cfg).items()}
    full.update({"transformer.resblocks.0.ln_1.weight": torch.ones(512), "token_embedding.weight": torch.zeros(8, 512),
                 "positional_embedding": torch.zeros(77, 512), "text_projection": torch.zeros(512, 512),
                 "ln_final.weight": torch.ones(512), "logit_scale": torch.zeros(())})
    enc.load_clip_state_dict(full)
    enc.finalize(DEV, torch.float32, n)
    vec, grid = enc({"rgb": R.images(seed, n, cfg[0]).to(DEV)})
    assert vec.dtype == torch.float32 and grid.dtype == torch.float32 and vec.shape == (n, 512) and grid.shape == (n, 196, 768)
    cols, toks = R.sample(grid)
    errs = [R.max_rel(vec.cpu().numpy(), gold["b16_l2_x"]), R.max_rel(cols.cpu().numpy(), gold["b16_l2_xp_cols"]),
            R.max_rel(toks.cpu().numpy(), gold["b16_l2_xp_toks"])]
    print(f"ClipRGBEncoder.forward b16_l2: max-abs / absmax {errs}")
    assert max(errs) <= FP32_GATE
    # the reference's signature on normalised float input gives the same pair
    x2, xp2 = enc.model.visual(R.transform(R.images(seed, n, cfg[0])).to(DEV))
    e2 = [R.max_rel(x2.cpu().numpy(), gold["b16_l2_x"]), R.max_rel(R.sample(xp2)[0].cpu().numpy(), gold["b16_l2_xp_cols"])]
    print(f"forward(normalised NCHW) b16_l2: max-abs / absmax {e2}")
    assert max(e2) <= FP32_GATE
    enc.model.visual.train()
    with pytest.raises(RuntimeError, match="forward-only"):
        enc({"rgb": R.images(seed, n, cfg[0]).to(DEV)})
    enc.model.visual.eval()
    with pytest.raises(ValueError, match="allocated for"):
        enc({"rgb": R.images(seed, n + 1, cfg[0]).to(DEV)})
    # new weights retire the operands finalize() built: no silent mix of old GEMM weights and new biases
    enc.load_clip_state_dict(full)
    with pytest.raises(RuntimeError, match="finalize"):
        enc({"rgb": R.images(seed, n, cfg[0]).to(DEV)})


def test_row_kernel_wrappers_refuse_tensors_the_kernels_would_overrun():
    H, rows = 256, 8
    z32, x = torch.zeros(rows, H, device=DEV), torch.zeros(rows, H, device=DEV, dtype=torch.bfloat16)
    v = torch.zeros(H, device=DEV)
    V.bias_residual_prenorm(z32, x, v, v, v)
    for bad in (dict(z32=z32.bfloat16()), dict(x=torch.zeros(rows, 2 * H, device=DEV, dtype=torch.bfloat16)[:, ::2]),
                dict(x=x[:4]), dict(bias=v[:128]), dict(gamma=v.bfloat16()), dict(y=torch.zeros(rows, H, device=DEV))):
        with pytest.raises(ValueError):
            V.bias_residual_prenorm(**{**dict(z32=z32, x=x, bias=v, gamma=v, beta=v), **bad})
    with pytest.raises(ValueError, match="whole number of images"):
        V.bias_residual_final(z32, x, v, v, v, 3)
    with pytest.raises(ValueError):
        V.bias_residual_final(z32, x, v, v, v, 4, x_patch=torch.zeros(2, 3, H, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        V.bias_quickgelu(x, v[:128])
    with pytest.raises(ValueError):
        V.bias_quickgelu(x, v, out=z32)
    with pytest.raises(ValueError):
        V.embed_prenorm(x, v, torch.zeros(4, H, device=DEV), (v, v), (v, v), 4)          # 8 rows, L - 1 = 3
    with pytest.raises(ValueError):
        V.embed_prenorm(x, v, torch.zeros(5, H, device=DEV, dtype=torch.bfloat16), (v, v), (v, v), 5)


# ------------------------------------------------------------------------------------------------ panorama
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encode_panorama_order_and_hand_over_to_waypoint_step_and_the_map(dtype):
    """Both operand dtypes: the outputs are bit-equal to the encoder run on images re-ordered by hand, and go unchanged into
    waypoint_step (with depth embeddings of the same dtype) and CEGraphMap.remember_pano.  fp32 also against the restatement."""
    from vln_bevbert_amd import waypoint as W
    from vln_bevbert_amd.ce_map import CEGraphMap
    from tests import waypoint_ref as WR
    B = 2
    cfg = R.CASES["b16_l2"][0]
    m = _model("b16_l2", dtype, B * 12)
    u8 = R.images(55, B * 12, cfg[0])
    gen = torch.Generator().manual_seed(5)
    depth = torch.rand(B, 12, 64, 64, 1, generator=gen) * 0.45 + 0.05
    rgb_embeds, rgb_grid, depth_grid = V.encode_panorama(m, u8.view(B, 12, 224, 224, 3).to(DEV), depth.to(DEV))
    assert rgb_embeds.shape == (B * 12, 512) and rgb_grid.shape == (B, 12, 196, 768) and depth_grid.shape == (B, 12, 14, 14)
    assert rgb_embeds.dtype == dtype and rgb_grid.dtype == torch.float32 and depth_grid.dtype == torch.float32
    assert rgb_embeds.is_contiguous() and rgb_grid.is_contiguous() and depth_grid.is_contiguous()
    # the reference re-orders the images first and encodes them in that order
    x_by_hand, xp_by_hand = m.encode_u8(R.clockwise(u8, B).to(DEV))
    assert torch.equal(rgb_embeds, x_by_hand) and torch.equal(rgb_grid.view(B * 12, 196, 768), xp_by_hand)
    assert not torch.equal(rgb_embeds[1], rgb_embeds[11])
    dref = torch.nn.functional.adaptive_avg_pool2d(R.clockwise(depth.view(B * 12, 64, 64, 1), B).double().permute(0, 3, 1, 2),
                                                   (14, 14)).view(B, 12, 14, 14)
    ed = float(((depth_grid.cpu().double() - dref).abs() / dref).max())
    print(f"encode_panorama {dtype}: depth grid against the re-ordered float64 pool {ed:.2e}")
    assert ed <= 1e-6
    if dtype == torch.float32:
        with torch.no_grad():
            x, xp = R.forward(R.state_dict(cfg), cfg, R.transform(R.clockwise(u8, B)))
        e = [R.max_rel(rgb_embeds.cpu().numpy(), x.numpy()), R.max_rel(rgb_grid.cpu().numpy(), xp.view(B, 12, 196, 768).numpy())]
        print(f"encode_panorama against the re-ordered restatement: embeds {e[0]:.2e} grid {e[1]:.2e}")
        assert e[0] <= FP32_GATE and e[1] <= FP32_GATE
        # view 1 of the simulator's order sits in slot 11, and differs from slot 1 (a missing re-ordering cannot pass)
        unordered = R.forward(R.state_dict(cfg), cfg, R.transform(u8[1:2]))[0]
        assert R.max_rel(rgb_embeds[11:12].cpu().numpy(), unordered.detach().numpy()) <= FP32_GATE
        assert R.max_rel(rgb_embeds[1:2].cpu().numpy(), unordered.detach().numpy()) > 10 * FP32_GATE
    # handed on unchanged
    dep_embeds = torch.from_numpy(WR.synthetic(71, (B * 12, 128, 4, 4))).to(DEV, dtype)
    logits = torch.from_numpy(WR.synthetic(72, (B, 12, 120))).to(DEV)
    wp = W.waypoint_step(None, rgb_embeds, dep_embeds, cls_logits=logits)
    assert wp["pano_rgb"].dtype == dtype and wp["vp_inputs"]["rgb_fts"].dtype == dtype
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
    assert int((cm.bev_inputs()["bev_fts"] != 0).any(2).sum()) >= 10 * B and cm.check_overflow() == 0


# ------------------------------------------------------------------------------------------------ capture, determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [1, 12])
def test_captured_encoder_equals_eager_bit_for_bit_and_nothing_synchronises(N, dtype):
    cfg = R.CASES["b16_l2"][0]
    m = _model("b16_l2", dtype, 12)
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
