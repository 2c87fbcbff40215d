"""Object-grounding navigation steps on the device: csrc/nav_obj.hip against torch restatements and the reference's own
outputs (tests/golden/nav_obj.npz, nav_tiny_rvr.npz: make_nav_obj_golden.py), the object branch of the fine-tune model
against the reference model, and object batches through the captured inference / training runners (nav_static.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import bevbert_ref as R
from tests.helpers import load_golden, max_abs, sub
from tests.test_gpu_model import FP32_TOL, bf16_close, bf16_grad_close          # the parity gates test_nav_api applies
from vln_bevbert_amd import nav_expert as NE
from vln_bevbert_amd import synthetic, weights
from vln_bevbert_amd.config import BevBertConfig
from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
from vln_bevbert_amd.nav_expert import ScanGraphs
from vln_bevbert_amd.nav_static import NavGraphRunner, nav_obj_variable

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
# the tiny REVERIE-style model of nav_tiny_rvr.npz (make_nav_obj_golden.RVR_TINY): a separate obj_linear
RVR_TINY = dict(image_feat_size=512, obj_feat_size=640, obj_prob_size=50, num_l_layers=1, num_x_layers=1)


@pytest.fixture(scope="module")
def gold():
    return load_golden("nav_obj")


@pytest.fixture(scope="module")
def graphs(gold, tmp_path_factory):
    raw = np.load(os.path.join(GOLDEN, "nav_scans.npz"))
    d = tmp_path_factory.mktemp("connectivity")
    paths = {}
    for s in gold["scans"]:
        s = str(s)
        ids, inc, un, pose = (raw[f"{s}/{k}"] for k in ("ids", "included", "unobstructed", "pose"))
        paths[s] = str(d / f"{s}_connectivity.json")
        with open(paths[s], "w") as f:
            json.dump([{"image_id": str(i), "included": bool(a), "unobstructed": [bool(x) for x in u],
                        "pose": [float(p) for p in po]} for i, a, u, po in zip(ids, inc, un, pose)], f)
    return ScanGraphs.from_connectivity(paths)


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------- 1. object rows
def _obj_variable_torch(pano, view_lens, obj_lens, Op):
    """agent_obj.py:343-349 in torch ops: slice each panorama's object rows, pad them with zero rows, build the mask."""
    rows = []
    for p, v, o in zip(pano, view_lens, obj_lens):
        rows.append(torch.cat([p[v:v + o].clone(), torch.zeros(Op - o, p.shape[1], dtype=p.dtype, device=p.device)], 0))
    mask = torch.arange(Op, device=pano.device)[None] < torch.as_tensor(obj_lens, device=pano.device)[:, None]
    return torch.stack(rows), mask


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [64, 768, 772])
def test_object_rows_and_their_adjoint_are_the_reference_copies_bit_for_bit(dtype, H):
    """B = 4, L = 12: one panorama's objects end exactly at L, one has none; 5 objects round up to Op = 8."""
    B, L, Op = 4, 12, 8
    vl, ol = (5, 7, 3, 8), (0, 5, 1, 4)
    g = torch.Generator().manual_seed(H)
    pano = torch.randn(B, L, H, generator=g).to(DEV, dtype).requires_grad_(True)
    w = torch.randn(B, Op, H, generator=g).to(DEV, dtype)
    w2 = torch.randn(B, L, H, generator=g).to(DEV, dtype)
    got = nav_obj_variable(pano, _t(vl), _t(ol), pad=4)
    obj, mask = got["obj_embeds"], got["obj_masks"]
    ref_obj, ref_mask = _obj_variable_torch(pano, vl, ol, Op)
    assert obj.shape == (B, Op, H) and mask.dtype == torch.bool
    assert torch.equal(obj, ref_obj) and torch.equal(mask, ref_mask)
    d, = torch.autograd.grad(obj, pano, w, retain_graph=True)
    d_ref, = torch.autograd.grad(ref_obj, pano, w, retain_graph=True)
    assert torch.equal(d, d_ref) and bool((d[0] == 0).all()) and bool((d[3, 8:] == w[3, :4]).all())
    # a second consumer of the panorama states (the map's node embeddings): autograd sums the two gradients
    other = pano * 0.5
    d, = torch.autograd.grad([obj, other], pano, [w, w2], retain_graph=True)
    d_ref, = torch.autograd.grad([ref_obj, other], pano, [w, w2])
    assert torch.equal(d, d_ref)
    # host lists spare the read-back and give the same tensors; the default pad is the loader's
    again = nav_obj_variable(pano.detach(), _t(vl), _t(ol), view_lens_host=list(vl), obj_lens_host=list(ol))
    assert torch.equal(again["obj_embeds"], obj) and torch.equal(again["obj_masks"], mask)


def test_object_rows_equal_the_references_nav_obj_variable(gold):
    pano = _t(gold["var_pano"])
    got = nav_obj_variable(pano, _t(gold["var_view_lens"]), _t(gold["var_obj_lens"]), pad=4)
    O = gold["var_obj_embeds"].shape[1]
    assert got["obj_embeds"].shape[1] == 8
    assert np.array_equal(got["obj_embeds"][:, :O].cpu().numpy(), gold["var_obj_embeds"])
    assert np.array_equal(got["obj_masks"][:, :O].cpu().numpy(), gold["var_obj_masks"])
    assert not bool(got["obj_masks"][:, O:].any()) and not bool(got["obj_embeds"][:, O:].any())
    none = nav_obj_variable(pano, _t(gold["var_view_lens"]), torch.zeros(4, dtype=torch.long, device=DEV))
    assert none["obj_embeds"].shape == (4, 4, 8) and not bool(none["obj_masks"].any()) and not bool(none["obj_embeds"].any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_object_row_kernels_clamp_lengths_that_do_not_fit(dtype):
    """The C entries with lengths the Python wrapper refuses: they are clamped to view_len in [0, L] and obj_len in
    [0, min(Op, L - view_len)], and the guard rows around both outputs keep their bytes."""
    B, L, Op, H = 4, 12, 8, 64
    vl, ol = _t([10, 3, -2, 20]), _t([5, 20, 3, 1])
    cvl, col = (10, 3, 0, 12), (2, 8, 3, 0)
    g = torch.Generator().manual_seed(1)
    pano = torch.randn(B, L, H, generator=g).to(DEV, dtype)
    obj_buf = torch.full((B + 2, Op, H), 7.0, dtype=dtype, device=DEV)
    mask_buf = torch.full((B + 2, Op), 3, dtype=torch.uint8, device=DEV)
    call("bevbert_obj_rows_fwd", ptr(pano), ptr(vl), ptr(ol), ptr(obj_buf[1:]), ptr(mask_buf[1:]), B, L, Op, H,
         dtype_code(pano), stream())
    ref_obj, ref_mask = _obj_variable_torch(pano, cvl, col, Op)
    assert torch.equal(obj_buf[1:B + 1], ref_obj) and torch.equal(mask_buf[1:B + 1].bool(), ref_mask)
    assert bool((obj_buf[[0, B + 1]] == 7).all()) and bool((mask_buf[[0, B + 1]] == 3).all())
    dobj = torch.randn(B, Op, H, generator=g).to(DEV, dtype)
    dp_buf = torch.full((B + 2, L, H), 7.0, dtype=dtype, device=DEV)
    call("bevbert_obj_rows_bwd", ptr(dobj), ptr(vl), ptr(ol), ptr(dp_buf[1:]), B, L, Op, H, dtype_code(dobj), stream())
    want = torch.zeros(B, L, H, dtype=dtype, device=DEV)
    for b, (v, o) in enumerate(zip(cvl, col)):
        want[b, v:v + o] = dobj[b, :o]
    assert torch.equal(dp_buf[1:B + 1], want) and bool((dp_buf[[0, B + 1]] == 7).all())


# ------------------------------------------------------------------------------------------------- 2. supervision
def _argmax_rows(logits, lens):
    """torch.argmax on the CPU over each row's valid slots (fp32 values of the logits as stored); -1 for an empty row."""
    lg = logits.float().cpu()
    return [int(torch.argmax(lg[b, :n])) if n > 0 else -1 for b, n in enumerate(lens)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_object_targets_equal_the_reference_and_the_slot_is_torch_argmax(gold, dtype):
    B, O = gold["sup_obj_logits"].shape
    N = int(gold["sup_cur"].max()) + 1
    logits = _t(gold["sup_obj_logits"]).to(dtype)
    lens = gold["sup_obj_len"].tolist()
    stop_og = torch.full((B, N), -9, dtype=torch.int32, device=DEV)
    out = NE.object_step(logits, _t(gold["sup_obj_ids"]), _t(gold["sup_obj_len"]), _t(gold["sup_gt_obj"]), _t(gold["sup_cur"]),
                         _t(gold["sup_end_vps"]), _t(gold["sup_n_end"]), _t(gold["sup_ended"]), stop_og)
    assert out["targets"].dtype == torch.int64 and out["targets"].cpu().numpy().tolist() == gold["sup_target"].tolist()
    slots = _argmax_rows(logits, lens)
    assert out["og_slot"].cpu().tolist() == slots and -1 in slots
    want = torch.full((B, N), -9, dtype=torch.int32)
    for b in range(B):
        if not gold["sup_ended"][b]:
            want[b, gold["sup_cur"][b]] = int(gold["sup_obj_ids"][b, slots[b]]) if slots[b] >= 0 else -1
    assert torch.equal(stop_og.cpu(), want)
    # the loss the targets feed is the existing one: rows without a target (and the row without objects) contribute nothing
    loss = NE.il_loss(logits, out["targets"])
    rows = [b for b, t in enumerate(gold["sup_target"]) if t >= 0]
    ref = torch.nn.functional.cross_entropy(logits.float().cpu()[rows], torch.from_numpy(gold["sup_target"][rows]),
                                            reduction="sum")
    # (fp32 sums of a handful of rows through the device's fast exp / log: a few ulp per row, 1e-4 relative is ample)
    assert abs(float(loss) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_object_slot_follows_torch_argmax_on_ties_masked_rows_and_nan(dtype):
    inf, nan = float("inf"), float("nan")
    rows = [[1.0, 3.0, -2.0, 3.0, 3.0, 0.0], [-inf, -inf, 2.0, -inf, -inf, -inf], [1.0, nan, 3.0, nan, 9.0, 0.0],
            [-inf, -inf, -inf, -inf, -inf, -inf], [4.0, 5.0, 6.0, 7.0, 8.0, 9.0], [0.5, 0.25, -inf, -inf, -inf, -inf],
            [nan, nan, nan, nan, nan, nan]]
    lens = [6, 6, 6, 3, 0, 2, 4]
    # more than one lane round: 150 slots with the maximum twice, in different rounds of the same lane and of another
    g = torch.Generator().manual_seed(8)
    wide = torch.randn(3, 150, generator=g)
    wide[0, [7, 71, 135]] = 50.0
    wide[1, [140, 12]] = 50.0
    wide[2, 149] = nan
    for logits, ln in ((torch.tensor(rows), lens), (wide, [150, 150, 150])):
        B, O = logits.shape
        logits = logits.to(DEV, dtype)
        ids = torch.arange(B * O, dtype=torch.int32, device=DEV).reshape(B, O) + 100
        stop_og = torch.full((B, 2), -9, dtype=torch.int32, device=DEV)
        z = torch.zeros(B, dtype=torch.int32, device=DEV)
        out = NE.object_step(logits, ids, _t(ln), z, z, torch.zeros(B, 1, dtype=torch.int32, device=DEV), z,
                             torch.zeros(B, dtype=torch.uint8, device=DEV), stop_og)
        slots = _argmax_rows(logits, ln)
        assert out["og_slot"].cpu().tolist() == slots
        assert stop_og[:, 0].cpu().tolist() == [100 + b * O + s if s >= 0 else -1 for b, s in enumerate(slots)]
        assert out["targets"].cpu().tolist() == [-100] * B            # n_end = 0: no goal viewpoint
    assert _argmax_rows(torch.tensor(rows), lens) == [1, 2, 1, 0, -1, 0, 0]


def test_stop_og_record_follows_the_dict_and_pred_obj_moves_only_on_just_ended_rows():
    """A scripted 4-step walk of B = 3 samples over N = 6 nodes: sample 0 comes back to node 0 at step 2 (the entry is
    overwritten), sample 1 stays put for a step, sample 2 ends after step 1 and has no objects at step 0."""
    B, N, O, T = 3, 6, 5, 4
    cur = [[0, 3, 5], [1, 3, 4], [0, 4, 4], [2, 5, 4]]
    ended = [[0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1]]
    lens = [[3, 5, 0], [2, 1, 4], [5, 0, 3], [1, 2, 2]]
    g = torch.Generator().manual_seed(21)
    stop_og = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    record = [dict() for _ in range(B)]
    z = torch.zeros(B, dtype=torch.int32, device=DEV)
    for t in range(T):
        logits = torch.randn(B, O, generator=g)
        ids = torch.randint(0, 1000, (B, O), generator=g, dtype=torch.int32)
        for b in range(B):
            logits[b, lens[t][b]:] = -float("inf")
        NE.object_step(logits.to(DEV), ids.to(DEV), _t(lens[t]), z, _t(cur[t], torch.int32),
                       torch.zeros(B, 1, dtype=torch.int32, device=DEV), z, _t(ended[t], torch.uint8), stop_og)
        for b in range(B):
            if not ended[t][b]:            # agent_obj.py:516-526
                record[b][cur[t][b]] = int(ids[b, torch.argmax(logits[b])]) if lens[t][b] > 0 else None
        want = [[-1 if record[b].get(n) is None else record[b][n] for n in range(N)] for b in range(B)]
        assert stop_og.cpu().tolist() == want, t
    assert len(record[0]) == 3 and record[2] == {5: None, 4: record[2][4]}
    pred = torch.tensor([77, 78, 79], dtype=torch.int32, device=DEV)
    NE.object_pick(_t([1, 0, 1], torch.uint8), _t([0, 4, -1], torch.int32), stop_og, pred)
    assert pred.cpu().tolist() == [record[0][0], 78, -1]
    NE.object_pick(_t([0, 1, 0], torch.uint8), _t([0, 5, 4], torch.int32), stop_og, pred)
    assert pred.cpu().tolist() == [record[0][0], -1 if record[1].get(5) is None else record[1][5], -1]


# ------------------------------------------------------------------------------------------------- 3. metrics
def test_reverie_eval_item_and_eval_metrics_match_the_reference(gold, graphs):
    items, avg = NE.nav_metrics_obj(graphs, _t(gold["met_scan"]), _t(gold["met_path"]), _t(gold["met_path_len"]),
                                    _t(gold["met_action_steps"]), _t(gold["met_gt"]), _t(gold["met_gt_len"]),
                                    _t(gold["met_goal_vps"]), _t(gold["met_n_goal"]), _t(gold["met_pred_obj"]),
                                    _t(gold["met_gt_obj"]))
    assert items.shape == (len(gold["met_scan"]), 8) and items.dtype == torch.float64 and avg.shape == (8,)
    av, per = NE.metrics_dicts_obj(items, avg)
    assert list(per) == list(NE.METRIC_FIELDS_OBJ) and list(av) == [str(k) for k in gold["met_avg_keys"]]
    for k in NE.METRIC_FIELDS_OBJ:
        np.testing.assert_allclose(np.asarray(per[k], dtype=np.float64), gold[f"met_item_{k}"], rtol=1e-12, atol=0, err_msg=k)
    for k, v in av.items():
        np.testing.assert_allclose(v, float(gold[f"met_avg_{k}"]), rtol=1e-12, atol=0, err_msg=k)
    # the length sums are the routine bevbert_nav_metrics uses: the same bits on the same paths
    r2r, _ = NE.nav_metrics(graphs, _t(gold["met_scan"]), _t(gold["met_path"]), _t(gold["met_path_len"]),
                            _t(gold["met_action_steps"]), _t(gold["met_gt"]), _t(gold["met_gt_len"]))
    assert torch.equal(r2r[:, 4], items[:, 2])
    bad, _ = NE.nav_metrics_obj(graphs, _t([7]), _t(gold["met_path"][:1]), _t(gold["met_path_len"][:1]),
                                _t(gold["met_action_steps"][:1]), _t(gold["met_gt"][:1]), _t(gold["met_gt_len"][:1]),
                                _t(gold["met_goal_vps"][:1]), _t(gold["met_n_goal"][:1]), _t(gold["met_pred_obj"][:1]),
                                _t(gold["met_gt_obj"][:1]))
    assert bool(bad.isnan().all())


# ------------------------------------------------------------------------------------------------- 4. model parity
def _nav_model(dtype, wrapped=False):
    from vln_bevbert_amd.nav_model import GlocalTextPathNavCMT, VLNBert
    cfg = BevBertConfig.tiny(**RVR_TINY)
    outer = VLNBert(cfg) if wrapped else None
    m = outer.vln_bert if wrapped else GlocalTextPathNavCMT(cfg)
    m.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    arena = m.finalize(DEV, dtype)
    return cfg, (outer.eval() if wrapped else m.eval()), arena


def _nav_inputs(cfg, pb, d, txt, txt_masks, dtype):
    """The navigation inputs test_nav_api builds from a synthetic batch (the map's node embeddings are given)."""
    B, G = d["gmap_lens"].shape[0], int(pb["gmap_lens"].max())
    lifted = R.lift_splat(cfg, pb)
    gimg = torch.randn(B, G, 768, generator=torch.Generator().manual_seed(99))
    gimg[:, 0] = 0
    return {"txt_embeds": txt, "txt_masks": txt_masks, "gmap_img_embeds": gimg.to(DEV),
            "gmap_step_ids": d["gmap_step_ids"], "gmap_pos_fts": d["gmap_pos_fts"],
            "gmap_masks": torch.arange(G, device=DEV)[None] < d["gmap_lens"][:, None],
            "gmap_pair_dists": d["gmap_pair_dists"], "gmap_visited_masks": d["gmap_visited_masks"],
            "gmap_vpids": pb["gmap_vpids"], "bev_fts": lifted["bev_fts"].to(DEV).to(dtype),
            "bev_pos_fts": lifted["bev_pos_fts"].to(DEV), "bev_masks": lifted["bev_masks"].to(DEV),
            "bev_nav_masks": d["bev_nav_masks"], "bev_cand_idxs": d["bev_cand_idxs"],
            "bev_cand_vpids": [[None] + c[-1] for c in pb["traj_cand_vpids"]], "obj_embeds": None, "obj_masks": None}


@pytest.mark.parametrize("dtype", DTYPES)
def test_object_branch_of_the_fine_tune_model_against_the_reference(dtype):
    g = load_golden("nav_tiny_rvr")
    cfg, model, arena = _nav_model(dtype)
    fp32 = dtype == torch.float32
    B = int(g["B"])
    pb = synthetic.make_batch(cfg, "sap", B, seed=int(g["seed"]), ragged=True)
    d = synthetic.batch_to(pb, DEV)

    def cmp(got, ref, step=None):
        got = got.detach().float().cpu()
        got = sub(got, step) if step else got.numpy()
        if fp32:
            assert max_abs(got, ref) < FP32_TOL
        else:
            bf16_close(got, ref, "nav")

    ends = torch.from_numpy(np.cumsum(pb["traj_step_lens"]) - 1).to(DEV)
    view_lens, obj_lens, L = d["traj_vp_view_lens"][ends], d["traj_vp_obj_lens"][ends], int(g["L"])
    assert view_lens.cpu().tolist() == g["view_lens"].tolist() and obj_lens.cpu().tolist() == g["obj_lens"].tolist()
    txt_masks = torch.arange(d["txt_ids"].shape[1], device=DEV)[None] < d["txt_lens"][:, None]
    arena.zero_grad()
    txt = model("language", {"txt_ids": d["txt_ids"], "txt_masks": txt_masks})
    pano, pm = model("panorama", {"view_img_fts": d["traj_view_img_fts"][ends], "obj_img_fts": d["traj_obj_img_fts"][ends],
                                  "loc_fts": d["traj_loc_fts"][ends][:, :L], "nav_types": d["traj_nav_types"][ends][:, :L],
                                  "view_lens": view_lens, "obj_lens": obj_lens})
    assert np.array_equal(pm.cpu().numpy(), g["pano_masks"])
    cmp(pano, g["pano_embeds_sub"], 5)
    ov = nav_obj_variable(pano, view_lens, obj_lens)
    O = g["obj_masks"].shape[1]
    assert ov["obj_embeds"].shape[1] == 4 and np.array_equal(ov["obj_masks"][:, :O].cpu().numpy(), g["obj_masks"])
    assert not bool(ov["obj_masks"][:, O:].any())
    cmp(ov["obj_embeds"][:, :O], g["obj_embeds"])
    nav = _nav_inputs(cfg, pb, d, txt, txt_masks, txt.dtype)
    nav.update(ov)
    out = model("navigation", nav)
    cmp(out["gmap_embeds"], g["nav_gmap_embeds_sub"], 3)
    for k in ("global", "local", "fused"):
        cmp(out[f"{k}_logits"], g[f"nav_{k}"])
    ol = out["obj_logits"]
    assert ol.dtype == torch.float32 and ol.shape == (B, 4) and bool(torch.isneginf(ol[:, O:]).all())
    assert np.array_equal(np.isfinite(ol[:, :O].detach().cpu().numpy()), np.isfinite(g["nav_obj"]))     # the -inf pattern
    cmp(ol[:, :O], g["nav_obj"])
    fl = out["fused_logits"]
    (ol[torch.isfinite(ol)].sum() + fl[torch.isfinite(fl)].sum()).backward()
    arena.sync()
    names = [k[6:] for k in g.files if k.startswith("grad::")]
    params = dict(model.named_parameters())
    for name in names:
        p, ref = params[name], g["grad::" + name]
        got = sub(p.main_grad.cpu(), 97 if p.numel() > 4096 else 1)
        scale = max(1e-6, float(np.abs(ref).max()))
        if fp32:
            assert max_abs(got, ref) < 2e-3 * scale + 1e-7, (name, max_abs(got, ref), scale)
        else:
            bf16_grad_close(got, ref, name)


# ------------------------------------------------------------------------------------------------- 5. captured inference
@pytest.mark.parametrize("dtype", DTYPES)
def test_object_batches_run_through_the_captured_inference_steps(dtype):
    """A 5-step episode of B = 4 with 0..5 objects per panorama, rolled out four times through one NavGraphRunner.  The
    object axis pads to 4 (three steps) or 8 (two steps), so each mode has two buckets; with six eager uses per bucket the
    first two passes are eager throughout, the buckets are captured in passes three and four, and every step of the fourth
    pass is a replay."""
    cfg, model, _ = _nav_model(dtype, wrapped=True)
    B, V, T = 4, 8, 5
    pb = synthetic.make_batch(cfg, "sap", B, seed=41, ragged=True)
    d = synthetic.batch_to(pb, DEV)
    g = torch.Generator().manual_seed(17)
    obj_lens = [[0, 5, 1, 4], [2, 0, 3, 1], [1, 0, 0, 0], [5, 5, 0, 2], [0, 2, 1, 0]]
    view_lens = [[8, 6, 7, 8], [7, 8, 8, 6], [8, 8, 6, 7], [6, 7, 8, 8], [8, 7, 6, 8]]
    steps = []
    for vl, ol in zip(view_lens, obj_lens):
        O, L = max(ol), max(v + o for v, o in zip(vl, ol))
        nav_types = torch.zeros(B, L, dtype=torch.long)
        for b in range(B):
            nav_types[b, :3] = 1
            nav_types[b, vl[b]:vl[b] + ol[b]] = 2
        steps.append(({"view_img_fts": torch.randn(B, V, cfg.image_feat_size, generator=g).to(DEV),
                       "obj_img_fts": torch.randn(B, O, cfg.obj_feat_size, generator=g).to(DEV),
                       "loc_fts": torch.randn(B, L, 7, generator=g).to(DEV), "nav_types": nav_types.to(DEV),
                       "view_lens": _t(vl), "obj_lens": _t(ol)}, vl, ol))
    with torch.no_grad():
        txt_masks = torch.arange(d["txt_ids"].shape[1], device=DEV)[None] < d["txt_lens"][:, None]
        txt = model("language", {"txt_ids": d["txt_ids"], "txt_masks": txt_masks})
        base = _nav_inputs(cfg, pb, d, txt, txt_masks, txt.dtype)
        keys = ("gmap_embeds", "global_logits", "local_logits", "fused_logits", "obj_logits")

        def rollout(pano_fn, nav_fn):
            outs = []
            for batch, vl, ol in steps:
                pe, pmask = pano_fn(batch)
                pe, pmask = pe.clone(), pmask.clone()
                assert pe.shape[1] == batch["loc_fts"].shape[1]
                nav = dict(base)
                nav.update(nav_obj_variable(pe, batch["view_lens"], batch["obj_lens"], view_lens_host=vl, obj_lens_host=ol))
                out = nav_fn(nav)
                outs.append({"pano_embeds": pe, "pano_masks": pmask, **{k: out[k].clone() for k in keys}})
            return outs

        runner = NavGraphRunner(model, eager_uses=6)
        passes = [rollout(runner.panorama, runner.navigation) for _ in range(4)]
        assert runner.graph_error is None, runner.graph_error
        assert runner.stats["captures"] >= 2 and runner.stats["replays"] > 0 and runner.stats["eager"] > 0, runner.stats
        assert runner.captured_graphs() == 4 and len(runner.buckets) == 4, list(runner.buckets)
        assert sorted(k[-1] for k in runner.buckets) == [4, 4, 8, 8]
        # the second eager pass (the library's GEMM plans have settled) against the replayed one: the same kernels on the
        # same buffers
        for t, (e, r) in enumerate(zip(passes[1], passes[3])):
            for k in e:
                assert torch.equal(e[k], r[k]), (t, k)
        plain = rollout(lambda b: model("panorama", b), lambda n: model("navigation", n))
    tol = 3e-2 if dtype == torch.bfloat16 else 1e-4          # the gate of scripts/bench_nav.py --check
    for t, (x, y) in enumerate(zip(passes[3], plain)):
        assert torch.equal(x["pano_masks"], y["pano_masks"])
        assert x["obj_logits"].shape == y["obj_logits"].shape == (B, max(4, -(-max(obj_lens[t]) // 4) * 4))
        for k in keys + ("pano_embeds",):
            a, b = x[k].float(), y[k].float()
            fin = torch.isfinite(b)
            assert a.shape == b.shape and torch.equal(torch.isfinite(a), fin) and not bool(torch.isnan(a).any()), (t, k)
            if k == "pano_embeds":          # rows beyond a panorama's own tokens are padding: masked everywhere downstream
                fin = fin & x["pano_masks"][..., None]
            assert float((a[fin] - b[fin]).abs().max()) <= tol * max(1.0, float(b[fin].abs().max())), (t, k)
        want = torch.arange(x["obj_logits"].shape[1])[None] < torch.tensor(obj_lens[t])[:, None]
        assert torch.equal(torch.isfinite(x["obj_logits"]).cpu(), want), t


# ------------------------------------------------------------------------------------------------- 6. captured training
def test_object_batches_run_through_the_captured_training_segments():
    """scripts/bench_nav.py --objects 5 --mode train --check: the whole chain (panorama -> map -> nav_obj_variable ->
    navigation -> object_step -> action_step -> object_pick -> losses) with one forward and one backward hipGraph per
    step and mode, against the same segments issued eagerly."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_nav.py"), "--objects", "5", "--batch", "4",
                        "--steps", "4", "--mode", "train", "--check"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["check"] == "ok" and rec["gradients_bitwise_equal"] and rec["graph_error"] is None, rec
    assert rec["captured_graphs"] >= 2 * 2 * 4 and rec["runner"]["replays"] >= 2 * 2 * 4, rec
    assert rec["loss_eager"] == rec["loss_graphs"] and rec["grad_norm"] > 0, rec
    assert rec["objects"] == 5 and rec["og_head_grad_norm"] > 0, rec
