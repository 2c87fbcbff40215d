"""csrc/waypoint.hip + vln_bevbert_amd/waypoint.py on the GPU: the ring attention against fp64 math, the predictor
against the reference's recorded logits, the candidate stage and the panorama inputs against the reference's recorded
outputs (tests/golden/waypoint.npz, made by tests/golden/make_waypoint_golden.py), the training draw against the CPU
restatement (tests/waypoint_ref.py, pinned to the reference by tests/test_waypoint_host.py), capture / no-sync / the
list-shaped view, and the padded inputs through ImageEmbeddings.embed in the CE configuration.  Every figure is printed
before it is asserted."""
import os

import numpy as np
import pytest
import torch

from tests import waypoint_ref as R
from tests.helpers import rule_state_dict
from vln_bevbert_amd import waypoint as W

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
CHI2_63_P1E4 = 113.505    # chi-square quantile, 63 degrees of freedom, upper tail p = 1e-4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "waypoint.npz"))


@pytest.fixture(scope="module")
def inputs(gold):
    n = gold["logits"].shape[0]
    return (torch.from_numpy(R.synthetic(21, (n * 12, 512), ints=True)).to(DEV),
            torch.from_numpy(R.synthetic(22, (n * 12, 128, 4, 4), ints=True)).to(DEV))


@pytest.fixture(scope="module")
def cls_logits(gold):
    return R.unroll(torch.from_numpy(gold["logits"])).contiguous().to(DEV)


def _predictor(dtype):
    m = W.WaypointPredictor()
    m.load_state_dict(rule_state_dict("waypoint_keys.txt"), strict=True)
    return m.finalize(DEV, dtype)


def _np(t):
    return t.detach().float().cpu().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0.0))


# ------------------------------------------------------------------------------------------------ ring attention
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 16, 64])
def test_ring_attention_against_fp64_three_key_and_additive_mask_forms(B, dtype):
    g = torch.Generator().manual_seed(100 + B)
    qkv = (torch.randn(B, 12, 3 * 768, generator=g) * 1.5).to(dtype)
    got = W.ring_attention(qkv.to(DEV), 12).float().cpu().double()
    three, masked = R.ring_attention(qkv.float(), 12), R.ring_attention(qkv.float(), 12, masked=True)
    tol = (1e-4 if dtype == torch.float32 else 1e-2) * max(1.0, float(three.abs().max()))
    e3, em, forms = float((got - three).abs().max()), float((got - masked).abs().max()), float((three - masked).abs().max())
    print(f"ring_attn B={B} {dtype}: vs three-key {e3:.3e} vs -10000 form {em:.3e} (forms apart {forms:.3e}) tol {tol:.3e}")
    assert e3 < tol and em < tol


# ------------------------------------------------------------------------------------------------ predictor
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_predictor_logits_against_the_recorded_reference_logits(gold, dtype):
    depth = torch.from_numpy(R.synthetic(int(gold["net_depth_seed"]), (36, 128, 4, 4))).to(DEV)
    m = _predictor(dtype)
    got = _np(m(None, depth))
    want = gold["net_logits"]
    assert got.shape == want.shape == (3, 120, 12)
    print(f"predictor {dtype}: max abs err {_err(got, want):.3e} (absmax {np.abs(want).max():.3f})")
    if dtype == torch.float32:
        assert _err(got, want) < 1e-3
    else:
        from tests.test_gpu_model import bf16_close
        bf16_close(got, want, "waypoint_logits")


# ------------------------------------------------------------------------------------------------ candidates, eval
@pytest.fixture(scope="module")
def eval_out(cls_logits, inputs):
    return W.waypoint_step(None, inputs[0], inputs[1], cls_logits=cls_logits)


def _counted(gold):
    """Every (a) and (b) map; a (c) map only if every pick leads by a relative 1e-4 on the reference's probabilities."""
    keep = np.ones(len(gold["group"]), bool)
    keep[gold["group"] == 2] = gold["net_margins"] >= 1e-4
    assert (~keep).sum() <= 1
    return keep


def test_candidates_equal_the_recorded_reference_outputs(gold, eval_out):
    keep = _counted(gold)
    o = {k: _np(v) for k, v in eval_out.items() if torch.is_tensor(v)}
    n = len(keep)
    want_idx = [[] for _ in range(n)]
    for b, a, d in gold["output_map_nz"]:
        want_idx[b].append((int(a), int(d)))
    for b in np.nonzero(keep)[0]:
        k = int(gold["eval_cand_count"][b])
        assert int(o["cand_count"][b]) == k, b
        assert list(zip(o["cand_angle_idx"][b, :k].tolist(), o["cand_dist_idx"][b, :k].tolist())) == want_idx[b], b
        assert (o["cand_angle_idx"][b, k:] == -1).all() and (o["cand_dist_idx"][b, k:] == -1).all()
    assert (o["cand_img_idx"][keep] == gold["eval_cand_img_idx"][keep]).all()
    for key in ("cand_angle_fts", "cand_angles", "cand_distances"):
        e = _err(o[key][keep], gold["eval_" + key][keep])
        print(f"{key}: max abs err {e:.3e}")
        assert e <= 1e-6, key
    f = gold["feat_idx"]
    e = _err(o["heat"][f], gold["heat"])
    print(f"heat: max abs err {e:.3e}; sums {o['heat'].sum((1, 2)).min():.7f} .. {o['heat'].sum((1, 2)).max():.7f}")
    assert e <= 1e-6
    nz = gold["output_map_nz"]
    assert _err(o["heat"][nz[:, 0], nz[:, 1], nz[:, 2]], gold["output_map_val"]) <= 1e-6


def test_panorama_inputs_equal_the_recorded_reference_outputs(gold, eval_out):
    keep = _counted(gold)
    vp = {k: _np(v) for k, v in eval_out["vp_inputs"].items()}
    L = gold["vp_nav_types"].shape[1]
    assert vp["nav_types"].shape[1] == W.L_PAD == 17 and vp["nav_types"].dtype == np.int64 and vp["view_lens"].dtype == np.int64
    assert (vp["view_lens"][keep] == gold["vp_view_lens"][keep]).all()
    assert (vp["nav_types"][keep][:, :L] == gold["vp_nav_types"][keep]).all() and not vp["nav_types"][:, L:].any()
    f = gold["feat_idx"]
    fk = keep[f]
    figs = {"loc_fts": _err(vp["loc_fts"][keep][:, :L], gold["vp_loc_fts"][keep]),
            "pano_rgb": _err(_np(eval_out["pano_rgb"])[f][fk], gold["pano_rgb"][fk]),
            "pano_depth": _err(_np(eval_out["pano_depth"])[f][fk], gold["pano_depth"][fk]),
            "rgb_fts": _err(vp["rgb_fts"][f][fk][:, :L], gold["vp_rgb_fts"][fk]),
            "dep_fts": _err(vp["dep_fts"][f][fk][:, :L], gold["vp_dep_fts"][fk]),
            "pano_angle_fts": _err(_np(eval_out["pano_angle_fts"]), gold["pano_angle_fts"])}
    print("panorama inputs, max abs err:", figs)
    assert all(v <= 1e-6 for v in figs.values()), figs
    for k in ("rgb_fts", "dep_fts", "loc_fts"):                      # rows past view_lens are zero
        pad = np.arange(17)[None, :] >= vp["view_lens"][:, None]
        assert not vp[k][pad].any(), k
    # real-valued embeddings: the 4 x 4 mean against the restatement (the recorded inputs are whole numbers)
    B = 5
    rgb = torch.from_numpy(R.synthetic(31, (B * 12, 512))).to(DEV)
    dep = torch.from_numpy(R.synthetic(32, (B * 12, 128, 4, 4))).to(DEV)
    o = W.waypoint_step(None, rgb, dep, cls_logits=R.unroll(torch.from_numpy(gold["logits"][:B])).contiguous().to(DEV))
    want = R.stage(gold["logits"][:B], rgb.cpu(), dep.cpu())
    for k in ("pano_rgb", "pano_depth"):
        assert _err(_np(o[k]), want[k]) <= 1e-6, k
    for k in ("rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens"):
        assert _err(_np(o["vp_inputs"][k]), want[k]) <= 1e-6, k


def test_bf16_embeddings_keep_their_dtype_and_values(gold, inputs, cls_logits):
    rgb, dep = inputs[0][:48].bfloat16(), inputs[1][:48].bfloat16()         # whole numbers: exact in bf16
    o = W.waypoint_step(None, rgb, dep, cls_logits=cls_logits[:4])
    want = R.stage(gold["logits"][:4], rgb.float().cpu(), dep.float().cpu())
    assert o["vp_inputs"]["rgb_fts"].dtype == torch.bfloat16 and o["pano_depth"].dtype == torch.bfloat16
    assert _err(_np(o["vp_inputs"]["rgb_fts"]), want["rgb_fts"]) == 0
    assert _err(_np(o["vp_inputs"]["dep_fts"]), want["dep_fts"]) <= 2 ** -8 * 8         # one bf16 rounding of a mean < 8


# ------------------------------------------------------------------------------------------------ training draw
def test_training_draw(gold, inputs, cls_logits):
    B = len(gold["group"])
    o = W.waypoint_step(None, inputs[0], inputs[1], in_train=True, seed=5, t=3, cls_logits=cls_logits)
    rp, rand = _np(o["region_probs"]), _np(o["rand"])
    cnt = _np(o["cand_count"])
    assert (cnt == gold["eval_cand_count"]).all()
    e = _err(rp[64:], gold["way_heats_probs"])
    print(f"region_probs vs way_heats_probs: {e:.3e}")
    assert e <= 1e-6
    ev = R.stage(gold["logits"])
    assert _err(rp, ev["region_probs"]) <= 1e-6
    ang, dist = _np(o["cand_angle_idx"]), _np(o["cand_dist_idx"])
    left_out = total = 0
    for b in range(B):
        for k in range(int(cnt[b])):
            probs = gold["way_heats_probs"][b - 64, k] if b >= 64 else ev["region_probs"][b, k]
            act, gap = R.inverse_cdf(probs, float(rand[b, k]))
            total += 1
            if gap < 1e-5:
                left_out += 1
                continue
            assert (int(ang[b, k]), int(dist[b, k])) == R.draw_cell(int(ev["cand_angle_idx"][b, k]), act), (b, k)
    print(f"draws checked {total - left_out} of {total}")
    assert left_out <= 0.01 * total
    # everything behind the draw follows from the drawn cells exactly as in the restatement
    acts = np.zeros((B, 5), np.int64)
    for b in range(B):
        for k in range(int(cnt[b])):
            a0 = int(ev["cand_angle_idx"][b, k])
            img = ((a0 + 5) // 10) % 12
            acts[b, k] = (int(ang[b, k]) - ((img - 1) * 10 + 5 if img else 0)) * 12 + int(dist[b, k])
    want = R.stage(gold["logits"], inputs[0].cpu(), inputs[1].cpu(), acts=acts)
    assert (_np(o["cand_img_idx"]) == want["cand_img_idx"]).all()
    for key in ("cand_angle_fts", "cand_angles", "cand_distances"):
        assert _err(_np(o[key]), want[key]) <= 1e-6, key
    for key in ("nav_types", "view_lens", "loc_fts", "rgb_fts", "dep_fts"):
        assert _err(_np(o["vp_inputs"][key]), want[key]) <= 1e-6, key
    # the stream: a function of (seed, t); uniform
    again = W.waypoint_candidates(cls_logits, True, seed=5, t=3)
    other = W.waypoint_candidates(cls_logits, True, seed=5, t=4)
    assert torch.equal(again["rand"], o["rand"]) and not torch.equal(other["rand"], o["rand"])
    big = cls_logits[:64].repeat(63, 1, 1)[:4000]
    r = _np(W.waypoint_candidates(big, True, seed=9, t=0)["rand"]).reshape(-1)
    assert r.size == 20000 and r.min() >= 0.0 and r.max() < 1.0
    hist = np.bincount((r * 64).astype(np.int64), minlength=64)
    chi2 = float(((hist - r.size / 64) ** 2 / (r.size / 64)).sum())
    print(f"chi-square over 64 bins: {chi2:.1f} (threshold {CHI2_63_P1E4})")
    assert chi2 < CHI2_63_P1E4


# ------------------------------------------------------------------------------------------------ capture, sync, lists
def test_captured_step_equals_eager_and_nothing_synchronises(gold):
    m = _predictor(torch.float32)
    B = 8

    def make(seed):
        return (torch.from_numpy(R.synthetic(seed, (B * 12, 512))).to(DEV),
                torch.from_numpy(R.synthetic(seed + 1, (B * 12, 128, 4, 4))).to(DEV))
    rgb, dep = make(40)
    for _ in range(2):                                   # plans, workspaces, cached tables
        W.waypoint_step(m, rgb, dep, in_train=True, seed=1, t=2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        W.waypoint_step(m, rgb, dep, in_train=True, seed=1, t=2)
        W.waypoint_step(m, rgb, dep)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    srgb, sdep = rgb.clone(), dep.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        W.waypoint_step(m, srgb, sdep, in_train=True, seed=1, t=2)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        cap = W.waypoint_step(m, srgb, sdep, in_train=True, seed=1, t=2)
    rgb2, dep2 = make(50)
    srgb.copy_(rgb2)
    sdep.copy_(dep2)
    g.replay()
    torch.cuda.synchronize()
    eager = W.waypoint_step(m, rgb2, dep2, in_train=True, seed=1, t=2)

    def same(a, b, path=""):
        for k in a:
            if isinstance(a[k], dict):
                same(a[k], b[k], k + ".")
            else:
                assert torch.equal(a[k], b[k]), path + k
    same(eager, cap)
    assert int(eager["cand_count"].min()) >= 1


def test_to_reference_yields_the_recorded_list_shaped_outputs(gold, eval_out):
    keep = _counted(gold)
    ref = W.to_reference(eval_out)
    assert set(ref) == {"cand_rgb", "cand_depth", "cand_angle_fts", "cand_img_idxes", "cand_angles", "cand_distances",
                        "pano_rgb", "pano_depth", "pano_angle_fts", "pano_img_idxes"}
    L = gold["vp_nav_types"].shape[1]
    pos = {int(b): i for i, b in enumerate(gold["feat_idx"])}
    for b in np.nonzero(keep)[0]:
        k = int(gold["eval_cand_count"][b])
        assert isinstance(ref["cand_angles"][b], list) and len(ref["cand_angles"][b]) == k
        assert isinstance(ref["cand_distances"][b], list) and len(ref["cand_distances"][b]) == k
        assert ref["cand_angles"][b] == gold["eval_cand_angles"][b, :k].tolist() or \
            _err(ref["cand_angles"][b], gold["eval_cand_angles"][b, :k]) <= 1e-6
        assert ref["cand_distances"][b] == gold["eval_cand_distances"][b, :k].tolist()
        assert ref["cand_img_idxes"][b].dtype == np.int64 and ref["cand_img_idxes"][b].tolist() == gold["eval_cand_img_idx"][b, :k].tolist()
        assert tuple(ref["cand_angle_fts"][b].shape) == (k, 4) and _err(ref["cand_angle_fts"][b].numpy(), gold["eval_cand_angle_fts"][b, :k]) <= 1e-6
        assert tuple(ref["cand_rgb"][b].shape) == (k, 512) and tuple(ref["cand_depth"][b].shape) == (k, 128)
        if int(b) in pos:
            assert _err(_np(ref["cand_rgb"][b]), gold["vp_rgb_fts"][pos[int(b)], :k]) <= 1e-6
            assert _err(_np(ref["cand_depth"][b]), gold["vp_dep_fts"][pos[int(b)], :k]) <= 1e-6
    assert ref["pano_img_idxes"].tolist() == list(range(12)) and L <= 17


# ------------------------------------------------------------------------------------------------ consumer
def test_padded_inputs_through_image_embeddings_in_the_ce_configuration(gold, eval_out):
    from vln_bevbert_amd import weights
    from vln_bevbert_amd.config import BevBertConfig
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    cfg = BevBertConfig.ce(num_l_layers=2, num_x_layers=2, num_pano_layers=1, vocab_size=1200, max_position_embeddings=128)
    model = GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    model.finalize(DEV, torch.float32)
    model.eval()
    emb, typ = model.bert.img_embeddings, model.bert.embeddings.token_type_embeddings
    vp = {k: v[:16] for k, v in eval_out["vp_inputs"].items()}
    scale = 1.0 / 8.0                                     # the recorded embeddings are whole numbers in [-8, 8)
    L = int(vp["view_lens"].max())
    with torch.no_grad():
        full, _ = emb.embed(vp["rgb_fts"] * scale, vp["loc_fts"], vp["nav_types"], vp["view_lens"], typ,
                            view_dep_fts=vp["dep_fts"] * scale)
        ref, _ = emb.embed((vp["rgb_fts"] * scale)[:, :L].contiguous(), vp["loc_fts"][:, :L].contiguous(),
                           vp["nav_types"][:, :L].contiguous(), vp["view_lens"], typ,
                           view_dep_fts=(vp["dep_fts"] * scale)[:, :L].contiguous())
    assert full.shape[1] == 17 and ref.shape[1] == L < 17
    valid = (torch.arange(L, device=DEV)[None, :] < vp["view_lens"][:, None])
    e = float((full[:, :L] - ref).abs()[valid].max())
    e_all = float((full[:, :L] - ref).abs().max())
    print(f"embed: padded-to-17 vs batch-max padded, valid rows {e:.3e}, all first {L} columns {e_all:.3e}")
    assert e_all < 1e-4 * max(1.0, float(ref.abs().max()))
