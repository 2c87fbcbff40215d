"""csrc/depth_resnet.hip + vln_bevbert_amd/depth_resnet.py on the GPU: the kernels against fp64 torch math, the model against
the restatement's recorded fp64 outputs (tests/golden/depth_resnet.npz, made by tests/golden/make_depth_resnet_golden.py) in
fp32 and with bf16 operands, the view order and the hand-over to waypoint_step, and capture / determinism / no host
synchronisation.  Every figure is printed before it is asserted.

GroupNorm inputs are uniform within a group (offset and scale differ per image and group), so that the normalised values stay
inside +-1.74 and every output, the two-term forms included, below 8: LN_TOL is an absolute gate, and from 8 on half the
spacing of bfloat16 (2^-5) alone exceeds its 2e-2."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import clip_ref as CR
from tests import depth_resnet_ref as R
from tests.test_gpu_model import RES32_FACTOR, _record      # the project's fp32-stream factor and its bf16 error log
from vln_bevbert_amd import clip_vit as V
from vln_bevbert_amd import depth_resnet as D
from vln_bevbert_amd import ops_gemm

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
FP32_GATE = 1e-3        # max-abs / absmax: the project's fp32 gate
LN_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}     # test_gpu_kernels.py::test_layernorm_fwd_bwd, forward
GN_SHAPES = [(32, 16), (64, 16), (128, 16), (256, 16), (512, 16), (1024, 16), (128, 1)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "depth_resnet.npz"))


_MODELS = {}


def _model(case, dtype, max_images=None):
    layers, size, n, _ = R.CASES[case]
    key = (case, dtype, max_images or n)
    if key not in _MODELS:
        m = D.DepthResNetEncoder(size, layers=layers)
        m.load_state_dict(R.state_dict(case), strict=True)
        _MODELS[key] = m.finalize(DEV, dtype, max_images or n)
    return _MODELS[key]


def _max_rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("size", [32, 256])
@pytest.mark.parametrize("N", [1, 3])
def test_stem_against_fp64_pool_and_convolution(N, size, mapped):
    """With a view map the N output images are drawn from N + 3 inputs in a scrambled order.  The two outermost rings of
    output pixels (the ones whose 7 x 7 window reaches into the padding) are compared on their own."""
    n_src = N + 3 if mapped else N
    depth = R.depth_images(300 + N + size, n_src, size)
    gen = torch.Generator().manual_seed(N + size)
    w = torch.randn(32, 1, 7, 7, generator=gen) * (2.0 / 49) ** 0.5
    vmap = torch.tensor([(5 * i + 2) % n_src for i in range(N)], dtype=torch.int32) if mapped else None
    src = depth if vmap is None else depth[vmap.long()]
    want = F.conv2d(F.avg_pool2d(src.double().permute(0, 3, 1, 2), 2), w.double(), None, 2, 3).permute(0, 2, 3, 1)
    got = D.stem_conv(depth.to(DEV), D.stem_weight(w).to(DEV), None if vmap is None else vmap.to(DEV)).cpu()
    assert got.shape == (N, size // 4, size // 4, 32) and got.dtype == torch.float32
    ring = torch.ones(size // 4, size // 4, dtype=torch.bool)
    ring[2:-2, 2:-2] = False
    err, err_ring = _max_rel(got, want), _max_rel(got[:, ring], want[:, ring])
    print(f"stem N={N} {size} x {size} mapped={mapped}: max-abs / absmax {err:.2e}, border rings alone {err_ring:.2e}")
    assert err <= 1e-5 and err_ring <= 1e-5


def test_stem_refuses_what_it_cannot_take():
    w = torch.zeros(49, 32, device=DEV)
    with pytest.raises(ValueError):
        D.stem_conv(torch.zeros(1, 30, 30, 1, device=DEV), w)
    with pytest.raises(ValueError):
        D.stem_conv(torch.zeros(1, 32, 32, 1, device=DEV), w.t().contiguous())
    with pytest.raises(ValueError):
        D.stem_conv(torch.zeros(1, 32, 32, 1, device=DEV), w, torch.zeros(1, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------ GroupNorm
def _group_uniform(gen, N, HW, C, G, spread=1.0):
    """(N, HW, C) fp32, uniform within a group with a per-(image, group) offset in +-2 and scale in [0.5, 2] x spread."""
    u = torch.rand(N, HW, C, generator=gen) - 0.5
    off = (4 * torch.rand(N, 1, G, generator=gen) - 2).repeat_interleave(C // G, 2)
    sc = (0.5 + 1.5 * torch.rand(N, 1, G, generator=gen)).repeat_interleave(C // G, 2) * spread
    return u * 12 ** 0.5 * sc + off


def _affine(gen, C, negative=False):
    g = 1 + 0.3 * (2 * torch.rand(C, generator=gen) - 1)
    if negative:
        g[::3] *= -1
    return g.to(DEV), (0.3 * (2 * torch.rand(C, generator=gen) - 1)).to(DEV)


def _gn64(x, G, g, b):
    """fp64 group_norm of NHWC rows (N, HW, C) -> (N, HW, C)."""
    return F.group_norm(x.double().transpose(1, 2), G, g.double(), b.double(), D.GN_EPS).transpose(1, 2)


@pytest.mark.parametrize("HW", [16, 64, 1024, 4096])
@pytest.mark.parametrize("C,G", GN_SHAPES)
def test_group_norm_statistics_and_every_apply_form_against_fp64(C, G, HW):
    """N in {1, 3}, fp32 and bf16 (the largest input, 3 x 4096 x 1024 fp32, is 50 MB); the fp64 group_norm runs on the device
    on the values the kernels read.  The max-pool form reads fp32 and has negative gammas."""
    side = int(HW ** 0.5)
    for N in (1, 3):
        gen = torch.Generator().manual_seed(C * 7 + G + HW + N)
        x32, r32, o32 = (_group_uniform(gen, N, HW, C, G).to(DEV) for _ in range(3))
        r32 *= 0.5                                       # the plain residual is added as it is: |r| <= 2.8
        (g, b), (g2, b2), (gneg, bneg) = _affine(gen, C), _affine(gen, C), _affine(gen, C, negative=True)
        # the stem's form: fp32 in, either dtype out
        st = D.group_norm_stats(x32, G)
        pooled = F.relu(F.max_pool2d(_gn64(x32, G, gneg, bneg).transpose(1, 2).reshape(N, C, side, side), 3, 2, 1))
        for dtype in (torch.float32, torch.bfloat16):
            got = D.group_norm_relu_maxpool(x32.view(N, side, side, C), st, gneg, bneg, G, dtype)
            e = float((got.double().permute(0, 3, 1, 2) - pooled).abs().max())
            print(f"GN C={C} G={G} HW={HW} N={N} max-pool form -> {dtype}: err {e:.2e}")
            assert got.dtype == dtype and got.shape == (N, (side + 1) // 2, (side + 1) // 2, C) and e < LN_TOL[dtype]
        for dtype in (torch.float32, torch.bfloat16):
            x, r, o = x32.to(dtype), r32.to(dtype), o32.to(dtype)
            st, st2 = D.group_norm_stats(x, G), D.group_norm_stats(o, G)
            xg = x.double().view(N, HW, G, C // G)
            mean64, var64 = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
            em = float((st[0].double() - mean64).abs().max())
            er = float((st[1].double() * torch.sqrt(var64 + D.GN_EPS) - 1).abs().max())
            assert st[0].shape == (N, G) and st[0].dtype == torch.float32 and st[1].dtype == torch.float32
            y64 = _gn64(x, G, g, b)
            forms = {"relu": (D.group_norm_apply(x, st, g, b, G), F.relu(y64)),
                     "+residual": (D.group_norm_apply(x, st, g, b, G, residual=r), F.relu(y64 + r.double())),
                     "+downsample": (D.group_norm_apply(x, st, g, b, G, other=(o, st2, g2, b2)),
                                     F.relu(y64 + _gn64(o, G, g2, b2))),
                     "nchw": (D.group_norm_apply(x, st, g, b, G, nchw=True), F.relu(y64).transpose(1, 2))}
            errs = {k: float((got.double() - want).abs().max()) for k, (got, want) in forms.items()}
            top = max(float(want.max()) for _, want in forms.values())
            print(f"GN C={C} G={G} HW={HW} N={N} {dtype}: mean err {em:.2e}, rstd rel err {er:.2e}, apply forms {errs}, largest "
                  f"output {top:.2f}")
            assert em < LN_TOL[torch.float32] and er < LN_TOL[torch.float32]
            assert all(got.dtype == dtype and got.shape == want.shape for got, want in forms.values())
            assert top < 8 and max(errs.values()) < LN_TOL[dtype]


@pytest.mark.parametrize("C,G", [(32, 16), (1024, 16)])
def test_group_norm_does_not_cancel_on_a_large_mean(C, G):
    """fp32 values of mean 100 and unit spread, HW = 4096: 1e-4 on the normalised values.  A two-pass fp32 computation stays
    below 1e-5 on such data, one pass over x and x^2 gives 2e-4 to 1.6e-3."""
    HW = 4096
    for N in (1, 3):
        gen = torch.Generator().manual_seed(C + N)
        x = (100 + torch.randn(N, HW, C, generator=gen)).to(DEV)
        mean, rstd = D.group_norm_stats(x, G)
        one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        want = _gn64(x, G, one, zero)
        cpg = C // G
        own = (x.double() - mean.double().repeat_interleave(cpg, 1)[:, None]) * rstd.double().repeat_interleave(cpg, 1)[:, None]
        applied = D.group_norm_apply(x, (mean, rstd), one, zero, G)
        e_stats, e_apply = float((own - want).abs().max()), float((applied.double() - F.relu(want)).abs().max())
        print(f"cancellation C={C} G={G} N={N}: normalised values from the statistics {e_stats:.2e}, through the apply kernel "
              f"{e_apply:.2e}")
        assert e_stats < 1e-4 and e_apply < 1e-4


def test_group_norm_wrappers_refuse_tensors_the_kernels_would_overrun():
    x = torch.zeros(2, 16, 64, device=DEV)
    st = D.group_norm_stats(x, 16)
    v = torch.ones(64, device=DEV)
    D.group_norm_apply(x, st, v, v, 16)
    for bad in (dict(x=x[:, :, ::2]), dict(G=3), dict(gamma=v[:32]), dict(stats=(st[0][:1], st[1])), dict(residual=x[:1]),
                dict(residual=x.bfloat16()), dict(out=torch.zeros(2, 16, 64, device=DEV, dtype=torch.bfloat16)),
                dict(residual=x, nchw=True)):
        with pytest.raises(ValueError):
            D.group_norm_apply(**{**dict(x=x, stats=st, gamma=v, beta=v, G=16), **bad})
    with pytest.raises(ValueError):
        D.group_norm_stats(torch.zeros(2, 16, 48, device=DEV), 16)
    with pytest.raises(ValueError):
        D.group_norm_stats(torch.zeros(1, 4096, 64, device=DEV), 16, partial=torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        D.group_norm_relu_maxpool(torch.zeros(2, 4, 4, 64, device=DEV, dtype=torch.bfloat16), st, v, v, 16, torch.float32)


# ------------------------------------------------------------------------------------------------ row gather
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("side", [4, 8, 32])
def test_row_gather_is_bit_equal_to_unfold(side, C, dtype):
    """3 x 3 pad 1 with stride 1 and 2, and the strided 1 x 1, on 3 images: F.unfold of the same values (columns (c, ky, kx))
    permuted to (ky, kx, c)."""
    N = 3
    gen = torch.Generator().manual_seed(side + C)
    x = torch.randn(N, side, side, C, generator=gen).to(dtype)
    nchw = x.float().permute(0, 3, 1, 2)
    for k, stride in ((3, 1), (3, 2), (1, 2), (1, 1)):
        so = (side - 1) // stride + 1
        want = F.unfold(nchw, k, padding=(k - 1) // 2, stride=stride).view(N, C, k * k, so * so).permute(0, 3, 2, 1)
        want = want.reshape(N * so * so, k * k * C).to(dtype)
        got = D.gather_rows(x.to(DEV), k, stride).cpu()
        diff = int((got != want).sum())
        print(f"gather side={side} C={C} {dtype} k={k} stride={stride}: {diff} of {got.numel()} values differ")
        assert got.shape == want.shape and got.dtype == dtype and diff == 0
        assert int((want == 0).sum()) > 0 or k == 1


def test_row_gather_refuses_what_it_cannot_take():
    x = torch.zeros(1, 4, 4, 32, device=DEV)
    with pytest.raises(ValueError):
        D.gather_rows(x, 5, 1)
    with pytest.raises(ValueError):
        D.gather_rows(x, 3, 3)
    with pytest.raises(ValueError):
        D.gather_rows(torch.zeros(1, 4, 4, 4, device=DEV, dtype=torch.bfloat16), 3, 1)       # 8-byte pixels
    with pytest.raises(ValueError):
        D.gather_rows(x, 3, 1, out=torch.zeros(16, 32, device=DEV))


# ------------------------------------------------------------------------------------------------ the model
def _run(case, dtype):
    _, size, n, seed = R.CASES[case]
    before = dict(ops_gemm.GEMM_FALLBACKS)
    y = _model(case, dtype).encode(R.depth_images(seed, n, size).to(DEV))
    new = {k: v for k, v in ops_gemm.GEMM_FALLBACKS.items() if before.get(k) != v}
    return y, new


@pytest.mark.parametrize("case", list(R.CASES))
def test_model_fp32_against_the_golden(gold, case):
    y, fallbacks = _run(case, torch.float32)
    want = gold[case + "_out"]
    err = CR.max_rel(y.cpu().numpy(), want)
    print(f"{case} fp32: max-abs / absmax {err:.3e} (the restatement's own fp32 {float(gold[case + '_fp32_max_rel']):.3e}); "
          f"GEMMs through torch: {fallbacks}")
    assert y.shape == want.shape and y.dtype == torch.float32 and y.is_contiguous()
    assert err <= FP32_GATE
    assert not fallbacks


@pytest.mark.parametrize("case", list(R.CASES))
def test_model_bf16_operands_within_the_restatements_own_bfloat16_error(gold, case):
    y, fallbacks = _run(case, torch.bfloat16)
    want, own = gold[case + "_out"], float(gold[case + "_bf16_rel_l2"])
    err = CR.rel_l2(y.float().cpu().numpy(), want)
    print(f"{case} bf16: rel-L2 {err:.3e}, the restatement's own bfloat16 autocast {own:.3e}, ratio {err / own:.2f}, gate "
          f"{RES32_FACTOR}; GEMMs through torch: {fallbacks}")
    _record("depth_resnet", case, rel_l2=err, ref_own_bf16=own, ratio=err / own)
    assert y.shape == want.shape and y.dtype == torch.bfloat16 and y.is_contiguous()
    assert err / own <= RES32_FACTOR
    assert not fallbacks


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_production_shapes_take_no_gemm_fallback(dtype):
    _, fallbacks = _run("r50_256", dtype)
    print(f"r50_256 {dtype}: GEMMs through torch during the run: {fallbacks}; all so far: {dict(ops_gemm.GEMM_FALLBACKS)}")
    assert not fallbacks


def test_forward_has_the_references_signature():
    _, size, n, seed = R.CASES["shallow_128"]
    m = _model("shallow_128", torch.float32)
    depth = R.depth_images(seed, n, size).to(DEV)
    y = m({"depth": depth})
    assert torch.equal(y, m.encode(depth)) and y.shape == (n,) + m.output_shape
    feats = torch.ones(1, 512, 2, 2, device=DEV)
    assert m({"depth": depth, "depth_features": feats}) is feats
    with pytest.raises(ValueError, match="allocated for"):
        m.encode(R.depth_images(seed, n + 1, size).to(DEV))
    with pytest.raises(ValueError, match="depth images expected"):
        m.encode(torch.zeros(1, 64, 64, 1, device=DEV))


# ------------------------------------------------------------------------------------------------ view order, hand-over
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_view_order_and_hand_over_to_waypoint_step(dtype):
    from vln_bevbert_amd import waypoint as W
    from tests import waypoint_ref as WR
    B = 2
    m = _model("r50_256", dtype, B * 12)
    depth = R.depth_images(77, B * 12, 256)
    mapped = m.encode(depth.to(DEV), V.clockwise_view_map(B, DEV))
    by_hand = m.encode(CR.clockwise(depth, B).to(DEV))
    assert torch.equal(mapped, by_hand)
    assert not torch.equal(mapped[1], mapped[11]) and not torch.equal(mapped, m.encode(depth.to(DEV)))
    # both backbones on one view map
    cfg = CR.CASES["b16_l2"][0]
    vit = V.ClipVisionTransformer(*cfg)
    vit.load_state_dict(CR.state_dict(cfg), strict=True)
    vit.finalize(DEV, dtype, B * 12)
    u8 = CR.images(55, B * 12, cfg[0])
    out = D.encode_observations(vit, m, u8.view(B, 12, 224, 224, 3).to(DEV), depth.view(B, 12, 256, 256, 1).to(DEV))
    assert sorted(out) == ["depth_embeds", "depth_grid", "rgb_embeds", "rgb_grid"]
    for k, shape, dt in (("rgb_embeds", (B * 12, 512), dtype), ("rgb_grid", (B, 12, 196, 768), torch.float32),
                         ("depth_grid", (B, 12, 14, 14), torch.float32), ("depth_embeds", (B * 12, 128, 4, 4), dtype)):
        assert out[k].shape == shape and out[k].dtype == dt and out[k].is_contiguous(), k
    assert torch.equal(out["depth_embeds"], mapped)
    pano = V.encode_panorama(vit, u8.view(B, 12, 224, 224, 3).to(DEV), depth.view(B, 12, 256, 256, 1).to(DEV))
    assert all(torch.equal(out[k], t) for k, t in zip(("rgb_embeds", "rgb_grid", "depth_grid"), pano))
    # handed on unchanged: the candidate stage on given logits, and the predictor's classifier on the embeddings themselves
    logits = torch.from_numpy(WR.synthetic(72, (B, 12, 120))).to(DEV)
    wp = W.waypoint_step(None, out["rgb_embeds"], out["depth_embeds"], cls_logits=logits)
    assert wp["pano_rgb"].dtype == dtype and int(wp["cand_count"].min()) >= 1
    predictor = W.WaypointPredictor().finalize(DEV, dtype)
    cls = predictor.classifier_output(out["depth_embeds"])
    assert cls.shape == (B, 12, 120) and bool(torch.isfinite(cls).all())
    wp = W.waypoint_step(predictor, out["rgb_embeds"], out["depth_embeds"])
    assert wp["cand_count"].shape[0] == B and torch.equal(wp["pano_rgb"][:, 0], out["rgb_embeds"].view(B, 12, 512)[:, 0])


# ------------------------------------------------------------------------------------------------ capture, determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_encoder_equals_eager_bit_for_bit_and_nothing_synchronises(dtype):
    _, size, n, seed = R.CASES["r50_256"]
    m = _model("r50_256", dtype)
    da, db = R.depth_images(seed + 1, n, size).to(DEV), R.depth_images(seed + 2, n, size).to(DEV)
    for _ in range(2):                                   # GEMM plans, workspaces
        m.encode(da)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = m.encode(da)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    second = m.encode(da)
    assert torch.equal(first, second), "two eager runs differ"
    static = da.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.encode(static)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        cap = m.encode(static)
    static.copy_(db)
    g.replay()
    torch.cuda.synchronize()
    eager = m.encode(db)
    assert torch.equal(eager, cap), "replay differs from eager"
    keep = cap.clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, keep), "two replays differ"
    assert not torch.equal(eager, first)
