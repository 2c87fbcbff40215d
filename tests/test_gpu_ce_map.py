"""csrc/ce_map.hip + vln_bevbert_amd/ce_map.py on the GPU against the reference's recorded outputs (tests/golden/ce_map.npz,
made by tests/golden/make_ce_map_golden.py from the reference's own GraphMap and trainer methods), after every step of
the three scripted episodes.  Integers exactly; float64 positions and distances to 1e-9 (device sin / cos / sqrt are
within a few ulp on coordinates under 100 m, summed over at most 16 terms: ~1e-13, and every discrete decision of the
file keeps a margin of 1e-6 or more); float32 features to 2e-6, the figure the discrete device map is held to.  Then the
training noise, both capacities, capture / no-sync, and one end-to-end step through the navigation forward.  Every
figure is printed before it is asserted."""
import os
import time

import numpy as np
import pytest
import torch

from tests import ce_map_ref as R
from vln_bevbert_amd.ce_map import CEGraphMap

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ce_map.npz")
DEV = "cuda"
F64_TOL, F32_TOL = 1e-9, 2e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def _err(a, b):
    return float(np.abs(np.asarray(_np(a), np.float64) - np.asarray(_np(b), np.float64)).max(initial=0.0))


def _inputs(gold, t, grids=False):
    i = {k[3:]: gold[k][t] for k in gold.files if k.startswith("in_")}
    d = {k: torch.from_numpy(i[k]).to(DEV) for k in ("cand_count", "cand_angles", "cand_distances", "avg_pano", "pano",
                                                      "nav_types", "a_t", "probs0", "cur_dist", "ghost_dist")}
    if grids:                                                       # 64 of the 768 channels keep the capture test light
        rgb, dep = _grids(t, gold["in_live"].shape[1])
        d["rgb_grid"], d["depth_grid"] = rgb[..., :64].contiguous(), dep
    return i, d


def _snapshot(m, live):
    """Device state in the layout of the golden file (rows of maps that are not live: as the file leaves them)."""
    t = {k: _np(v) for k, v in m.t.items()}
    lv = live[:, None]
    npos = np.where(t["g_alive"] > 0, t["g_npos"], 0)
    fr = np.where(np.arange(m.P)[None, None] < npos[..., None], t["g_fronts"], -1)
    n = t["n_nodes"]
    inside = (np.arange(m.N)[None, :, None] < n[:, None, None]) & (np.arange(m.N)[None, None, :] < n[:, None, None])
    return {"n_nodes": np.where(live, n, 0), "node_pos": np.where(lv[..., None] & (np.arange(m.N)[None, :, None] < n[:, None, None]), t["node_pos"], 0),
            "dist": np.where(lv[..., None] & inside, t["dist"], np.inf), "hops": np.where(lv[..., None] & inside, t["hops"], 0),
            "ghost_alive": (t["g_alive"] > 0) & lv, "ghost_mean": np.where((t["g_alive"] > 0)[..., None] & lv[..., None], t["g_mean"], 0),
            "ghost_aug": np.where((t["g_alive"] > 0)[..., None] & lv[..., None], t["g_aug"], 0),
            "ghost_nfronts": np.where(lv, npos, 0), "ghost_fronts": np.where(lv[..., None], fr, -1)}


def _grids(t, B):
    rgb, dep = R.grids(t, B)
    return torch.from_numpy(rgb).to(DEV), torch.from_numpy(dep).to(DEV)


def _drive(gold, m, steps=None, snap=True, pano=False):
    """The device map through the recorded episodes: per step, host copies of every output."""
    T = gold["in_live"].shape[0]
    out = []
    for t in range(T if steps is None else steps):
        i, d = _inputs(gold, t)
        o = {"cand_slot": m.update(t + 1, d["cand_count"], d["cand_angles"], d["cand_distances"], d["avg_pano"], d["pano"],
                                   d["nav_types"], cur_pos=i["cur_pos"], heading=i["heading"], live=i["live"])}
        if snap:
            torch.cuda.synchronize()
            o["state"] = _snapshot(m, i["live"])
        if pano:
            m.remember_pano(*_grids(t, m.B))
            o["bev_o2"] = m.bev_inputs(order=2)
            o["bev_fts_o2"], o["rows_live_o2"] = o["bev_o2"]["bev_fts"], o["bev_o2"]["grid_rows_live"]
            del o["bev_o2"]
        o.update(m.nav_gmap_variable())
        o.update(m.bev_inputs())
        m.record_stop_scores(d["probs0"])
        o["teacher"] = m.teacher_index(d["cur_dist"], d["ghost_dist"])
        o["rec"] = m.act(d["a_t"], last_step=t == T - 1)
        o["actions"] = m.to_reference(o["rec"])
        out.append({k: _np(v) for k, v in o.items()})
    return out


@pytest.fixture(scope="module")
def run(gold):
    T, B = gold["in_live"].shape
    m = CEGraphMap(B, gold["in_avg_pano"].shape[-1], DEV, loc_noise=float(gold["loc_noise"]),
                   merge_ghost=gold["merge_ghost"].tolist())
    out = _drive(gold, m, pano=True)
    assert m.check_overflow() == 0
    return out


@pytest.fixture(scope="module")
def ref(gold):
    return R.replay(gold)


# ------------------------------------------------------------------------------------------------ against the reference
def test_graph_state_after_every_step(gold, run):
    for t, o in enumerate(run):
        s = o["state"]
        assert np.array_equal(o["cand_slot"], gold["cand_slot"][t]), (t, o["cand_slot"], gold["cand_slot"][t])
        for k in ("n_nodes", "hops", "ghost_alive", "ghost_nfronts", "ghost_fronts"):
            assert np.array_equal(s[k], gold[k][t]), (t, k)
        fin = np.isfinite(gold["dist"][t])
        assert np.array_equal(np.isfinite(s["dist"]), fin), t
        e = (_err(s["node_pos"], gold["node_pos"][t]), _err(s["dist"][fin], gold["dist"][t][fin]),
             _err(s["ghost_mean"], gold["ghost_mean"][t]), _err(s["ghost_aug"], gold["ghost_mean"][t]))
        print(f"step {t}: node_pos {e[0]:.2e} shortest_dist {e[1]:.2e} ghost_mean {e[2]:.2e} ghost_aug (no noise) {e[3]:.2e}")
        assert max(e) <= F64_TOL


def test_navigation_variables_after_every_step(gold, run):
    for t, o in enumerate(run):
        for k in ("gmap_ids", "gmap_step_ids", "gmap_visited_masks", "gmap_masks", "no_vp_left"):
            assert o[k].shape == gold[k][t].shape and np.array_equal(o[k], gold[k][t]), (t, k)
        e = {k: _err(o[k], gold[k][t]) for k in ("gmap_img_fts", "gmap_pos_fts", "gmap_pair_dists")}
        print(f"step {t}:", {k: f"{v:.2e}" for k, v in e.items()})
        assert o["gmap_pos_fts"].dtype == np.float32 and o["gmap_pair_dists"].dtype == np.float32
        assert max(e.values()) <= F32_TOL


def test_bev_candidates_and_fusion_indices_after_every_step(gold, run, ref):
    K = gold["bev_cand_ids"].shape[-1]
    for t, (o, r) in enumerate(zip(run, ref)):
        live = gold["in_live"][t]
        assert o["bev_cand_ids"].shape[1] == K
        for k in ("bev_nav_masks", "bev_cand_count", "bev_cand_ids", "bev_cand_idxs"):
            assert np.array_equal(o[k], gold[k][t]), (t, k, o[k], gold[k][t])
        assert np.array_equal(o["src"], r["src"]) and np.array_equal(o["vis_c"], r["vis_c"][:, :K]), t
        assert o["bev_masks"].all() and o["bev_masks"].shape == gold["bev_nav_masks"][t].shape
        e = _err(o["bev_pos_fts"][live], gold["bev_pos_fts"][t][live])
        print(f"step {t}: bev_pos_fts {e:.2e}")
        assert e <= F32_TOL


def test_lifted_bev_features_equal_the_reference_lift_and_splat(gold, run):
    """The criterion of test_finetune_bev_from_store_rows_of_visited_neighbours: float32 BEV features agree exactly (a
    cell that differs in membership differs in its mean).  order = 1 as the trainer calls gather_node_pc (the current
    node only) and order = 2 (stored 1-hop neighbours too); every 16th channel and each cell's sum over all 768."""
    multi = 0
    for t, o in enumerate(run):
        live = gold["in_live"][t]
        for key, got in (("bev_fts", o["bev_fts"]), ("bev_fts_o2", o["bev_fts_o2"])):
            assert got.shape == (len(live), 121, 768) and got.dtype == np.float32
            e = (_err(got[live][:, :, ::16], gold[key][t][live]), _err(got[live].astype(np.float64).sum(2), gold[key + "_sum"][t][live]))
            filled = int((gold[key][t][live] != 0).any(2).sum())
            print(f"step {t} {key}: sampled channels {e[0]:.1e}, per-cell sums {e[1]:.1e}, {filled} filled cells")
            assert np.array_equal(got[live][:, :, ::16], gold[key][t][live]) and e[1] == 0.0, (t, key)
        assert np.array_equal(o["rows_live_o2"].sum(1)[live], gold["bev_nodes_o2"][t][live]), t
        assert np.array_equal(o["grid_rows_live"].sum(1)[live], np.ones(int(live.sum()))), t
        multi += int((gold["bev_nodes_o2"][t] > 1).sum())
    assert multi >= 5


def test_teacher_action_record_and_reference_dicts_after_every_step(gold, run):
    N = gold["node_pos"].shape[2]
    for t, o in enumerate(run):
        assert np.array_equal(o["teacher"], gold["teacher"][t]), (t, o["teacher"], gold["teacher"][t])
        rec = o["rec"]
        ints = rec[:, :5 + N].astype(np.int64)
        assert np.array_equal(ints.astype(np.float64), rec[:, :5 + N])
        live = gold["in_live"][t]
        assert np.array_equal(ints[:, 0], gold["act"][t]) and np.array_equal(ints[:, 4], gold["act_path_len"][t]), t
        assert np.array_equal(ints[live, 2], gold["act_target"][t][live]) and np.array_equal(ints[:, 3], gold["act_ghost"][t])
        assert np.array_equal(ints[:, 5:], gold["act_path"][t]), (t, ints[:, 5:], gold["act_path"][t])
        e = (_err(rec[live, 5 + N:8 + N], gold["act_target_pos"][t][live]), _err(rec[:, 8 + N:11 + N], gold["act_ghost_pos"][t]))
        print(f"step {t}: stop / front position {e[0]:.2e} ghost position {e[1]:.2e}")
        assert max(e) <= F64_TOL
        for b, a in enumerate(o["actions"]):
            if not live[b]:
                assert a is None
                continue
            a = a["action"]
            n = int(gold["act_path_len"][t, b])
            assert a["cur_vp"] == str(gold["n_nodes"][t, b] - 1) and a["act"] == gold["act"][t, b]
            assert [v for v, _ in a["back_path"]] == [str(v) for v in gold["act_path"][t, b, :n]]
            for v, p in a["back_path"]:
                assert _err(p, gold["node_pos"][t, b, int(v)]) <= F64_TOL
            if a["act"] == 0:
                assert a["stop_vp"] == str(gold["act_target"][t, b]) and _err(a["stop_pos"], gold["act_target_pos"][t, b]) <= F64_TOL
            else:
                assert a["front_vp"] == str(gold["act_target"][t, b]) and a["ghost_vp"] == f"g{gold['act_ghost'][t, b]}"
                assert _err(a["ghost_pos"], gold["act_ghost_pos"][t, b]) <= F64_TOL


# ------------------------------------------------------------------------------------------------ training noise
def test_ghost_aug_noise_is_clipped_planar_redrawn_seeded_and_used_by_the_features(gold):
    T, B = gold["in_live"].shape
    a = 0.3
    kw = dict(loc_noise=float(gold["loc_noise"]), merge_ghost=gold["merge_ghost"].tolist(), ghost_aug=a)
    runs = [_drive(gold, CEGraphMap(B, 32, DEV, seed=s, **kw)) for s in (7, 7, 8)]
    noise = [[{} for _ in range(B)] for _ in range(T)]
    drawn, moved, kept = 0, 0, 0
    for t in range(T):
        s0, s1, s2 = (r[t]["state"] for r in runs)
        assert np.array_equal(s0["ghost_aug"], s1["ghost_aug"]), "equal seeds, different draws"
        al = s0["ghost_alive"]
        assert np.array_equal(s0["ghost_mean"], s2["ghost_mean"]) and (not al.any() or not np.array_equal(s0["ghost_aug"], s2["ghost_aug"]))
        nz = s0["ghost_aug"] - s0["ghost_mean"]
        assert (nz[..., 1] == 0).all() and np.abs(nz).max(initial=0.0) <= a + 1e-12
        for b, g in zip(*np.nonzero(al)):
            noise[t][b][int(g)] = nz[b, g]
            drawn += 1
            if t and runs[0][t - 1]["state"]["ghost_alive"][b, g]:
                prev = runs[0][t - 1]["state"]
                moved += not np.array_equal(nz[b, g], prev["ghost_aug"][b, g] - prev["ghost_mean"][b, g])
                kept += 1
    allnz = np.concatenate([np.stack(list(n.values())) for row in noise for n in row if n])
    clipped = float((np.abs(allnz[:, [0, 2]]) >= a - 1e-9).mean())       # (mean + a) - mean is a only up to rounding
    print(f"{drawn} draws, {moved} of {kept} surviving ghosts redrawn; |noise| max {np.abs(allnz).max():.4f} (a = {a}); "
          f"clipped share {clipped:.2f} (normal: 0.32); mean {allnz[:, [0, 2]].mean():+.3f}")
    # the draws depend on the process-wide step salt, so the gates are statistical and wide: a surviving ghost keeps
    # its noise only if both components clip to the same side twice running (probability (2 * 0.1585 ** 2) ** 2 =
    # 0.0025), so fewer than half of ~30 redrawn has probability < 1e-30; the clipped share of 108 draws (mean 0.317, standard
    # deviation 0.045) is only required to be neither 0 nor 1
    assert drawn > 20 and kept > 10 and moved >= kept // 2 and 0.0 < clipped < 1.0
    # the features are built from the augmented positions: the restatement fed with the device's own noise
    want = R.replay(gold, noise=noise)
    for t, (o, r) in enumerate(zip(runs[0], want)):
        assert np.array_equal(o["gmap_ids"], r["gmap_ids"])
        e = (_err(o["gmap_pos_fts"], r["gmap_pos_fts"]), _err(o["gmap_pair_dists"], r["gmap_pair_dists"]),
             _err(o["state"]["ghost_aug"], r["state"]["ghost_aug"]))
        plain = _err(o["gmap_pos_fts"], gold["gmap_pos_fts"][t])
        print(f"step {t}: pos_fts {e[0]:.2e} pair_dists {e[1]:.2e} aug {e[2]:.2e}; pos_fts against the noise-free file {plain:.2e}")
        assert e[0] <= F32_TOL and e[1] <= F32_TOL and e[2] <= F64_TOL
        assert plain > 1e-3 or not o["state"]["ghost_alive"].any()


# ------------------------------------------------------------------------------------------------ capacities
@pytest.mark.parametrize("kw,steps", [(dict(node_capacity=2, ghost_capacity=40), 3), (dict(node_capacity=16, ghost_capacity=3), 1),
                                      (dict(node_capacity=16, ghost_capacity=80), 3)])
def test_overflow_of_either_capacity_sets_the_flag(gold, kw, steps):
    B = gold["in_live"].shape[1]
    m = CEGraphMap(B, 32, DEV, loc_noise=float(gold["loc_noise"]), merge_ghost=gold["merge_ghost"].tolist(), **kw)
    for t in range(steps):
        i, d = _inputs(gold, t)
        m.update(t + 1, d["cand_count"], d["cand_angles"], d["cand_distances"], d["avg_pano"], d["pano"], d["nav_types"],
                 cur_pos=i["cur_pos"], heading=i["heading"], live=i["live"])
        if t < steps - 1:                                           # the recorded actions name rows of complete maps
            m.nav_gmap_variable()
            m.act(d["a_t"])
    n, g = _np(m.t["n_nodes"]), _np(m.t["g_cnt"])
    flag = m.check_overflow()
    print(kw, "-> flag", flag, "nodes", n, "ghost ids", g)
    assert flag == (0 if kw["ghost_capacity"] == 80 else 1)
    assert n.max() <= kw["node_capacity"] and g.max() <= kw["ghost_capacity"]


def test_a_candidate_without_an_embedding_row_is_refused_with_the_flag(gold):
    B = gold["in_live"].shape[1]
    m = CEGraphMap(B, 32, DEV, loc_noise=float(gold["loc_noise"]), merge_ghost=gold["merge_ghost"].tolist())
    i, d = _inputs(gold, 0)
    nav = d["nav_types"].clone()
    nav[0, int(d["cand_count"][0]) - 1] = 0                         # map 0: one row of type 1 fewer than candidates
    slot = m.update(1, d["cand_count"], d["cand_angles"], d["cand_distances"], d["avg_pano"], d["pano"], nav,
                    cur_pos=i["cur_pos"], heading=i["heading"], live=i["live"])
    k = int(d["cand_count"][0])
    print("cand_slot of map 0:", slot[0].tolist(), "ghosts:", _np(m.t["g_cnt"]), "flag", m.check_overflow())
    assert m.check_overflow() == 1 and int(slot[0, k - 1]) == -1 and int(m.t["g_cnt"][0]) == k - 1
    assert np.array_equal(_np(slot[1:]), gold["cand_slot"][0][1:])


# ------------------------------------------------------------------------------------------------ capture, sync
def _step(m, d, last):
    o = {"cand_slot": m.update(0, d["cand_count"], d["cand_angles"], d["cand_distances"], d["avg_pano"], d["pano"], d["nav_types"])}
    m.remember_pano(d["rgb_grid"], d["depth_grid"])
    o["bev_fts_o2"] = m.bev_inputs(order=2)["bev_fts"]
    o.update(m.nav_gmap_variable())
    o.update(m.bev_inputs())
    m.record_stop_scores(d["probs0"])
    o["teacher"] = m.teacher_index(d["cur_dist"], d["ghost_dist"])
    o["rec"] = m.act(d["a_t"], last_step=last)
    return o


def test_captured_step_equals_eager_bit_for_bit_and_nothing_synchronises(gold):
    B = gold["in_live"].shape[1]
    kw = dict(loc_noise=float(gold["loc_noise"]), merge_ghost=gold["merge_ghost"].tolist(), ghost_aug=0.2, seed=3)
    eager, graphed = CEGraphMap(B, 32, DEV, **kw), CEGraphMap(B, 32, DEV, **kw)
    i0, static = _inputs(gold, 0, grids=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                    # step 0 of the graphed map doubles as the warm-up
        graphed.stage(1, i0["cur_pos"], i0["heading"], i0["live"])
        _step(graphed, static, False)
    torch.cuda.current_stream().wait_stream(s)
    eager.stage(1, i0["cur_pos"], i0["heading"], i0["live"])
    _step(eager, static, False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.stage(0, i0["cur_pos"], i0["heading"], i0["live"])
        cap = _step(graphed, static, False)
    stage_ms = []
    for t in (1, 2, 3):
        i, d = _inputs(gold, t, grids=True)
        for k in static:
            static[k].copy_(d[k])
        graphed.stage(t + 1, i["cur_pos"], i["heading"], i["live"], copy=False)
        g.replay()
        graphed.mark_replayed()
        if t == 3:                                                # stage included: it waits for no copy but the one before last
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            t0 = time.perf_counter()
            eager.stage(t + 1, i["cur_pos"], i["heading"], i["live"])
            stage_ms.append((time.perf_counter() - t0) * 1e3)
            want = _step(eager, d, False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for k in want:
            assert torch.equal(want[k], cap[k]), (t, k)
        for k in eager.t:
            assert torch.equal(eager.t[k], graphed.t[k]), (t, k)
    print("host time of stage():", [f"{x:.3f} ms" for x in stage_ms])
    assert int(want["gmap_masks"].sum()) > 3 * B and eager.check_overflow() == 0


# ------------------------------------------------------------------------------------------------ consumer
def test_one_step_from_waypoints_to_fused_logits_with_device_fusion_indices():
    from vln_bevbert_amd import waypoint as W, weights
    from vln_bevbert_amd.config import BevBertConfig
    from vln_bevbert_amd.nav_model import GlocalTextPathNavCMT
    from tests import waypoint_ref as WR
    from tests.helpers import rule_state_dict
    B = 2
    cfg = BevBertConfig.ce(num_l_layers=2, num_x_layers=2, num_pano_layers=1, vocab_size=1200, max_position_embeddings=128)
    model = GlocalTextPathNavCMT(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.finalize(DEV, torch.float32)
    model.eval()
    pred = W.WaypointPredictor()
    pred.load_state_dict(rule_state_dict("waypoint_keys.txt"), strict=True)
    pred.finalize(DEV, torch.float32)
    m = CEGraphMap(B, cfg.hidden_size, DEV, loc_noise=0.5)
    gen = torch.Generator().manual_seed(4)
    txt_ids = torch.randint(1, 1000, (B, 20), generator=gen).to(DEV)
    txt_masks = torch.ones(B, 20, dtype=torch.bool, device=DEV)
    pos = np.array([[0.0, 0.0, 0.0], [5.0, 1.0, -2.0]])
    with torch.no_grad():
        txt = model("language", {"txt_ids": txt_ids, "txt_masks": txt_masks})
        for t in range(2):                                          # the second step has visited neighbours and old ghosts
            rgb = torch.from_numpy(WR.synthetic(60 + t, (B * 12, 512))).to(DEV)
            dep = torch.from_numpy(WR.synthetic(70 + t, (B * 12, 128, 4, 4))).to(DEV)
            wp = W.waypoint_step(pred, rgb, dep)
            vp = wp["vp_inputs"]
            pano, pm = model.img_embeddings.embed(vp["rgb_fts"], vp["loc_fts"], vp["nav_types"], vp["view_lens"],
                                                  model.embeddings.token_type_embeddings, view_dep_fts=vp["dep_fts"])
            avg = (pano * pm.unsqueeze(2)).sum(1) / pm.sum(1, keepdim=True)
            m.update(t + 1, wp["cand_count"], wp["cand_angles"], wp["cand_distances"], avg, pano, vp["nav_types"],
                     cur_pos=pos, heading=np.array([0.4, 2.0]) + t)
            m.remember_pano(torch.from_numpy(WR.synthetic(80 + t, (B, 12, 196, 768))).to(DEV),
                            torch.from_numpy(np.abs(WR.synthetic(90 + t, (B, 12, 14, 14))) * 0.4).to(DEV))
            nav = m.nav_gmap_variable()
            bev = m.bev_inputs()
            bev_fts = bev["bev_fts"]
            assert int((bev_fts != 0).any(2).sum()) >= 10 * B
            args = dict(txt_embeds=txt, txt_masks=txt_masks, gmap_img_embeds=nav["gmap_img_fts"], gmap_step_ids=nav["gmap_step_ids"],
                        gmap_pos_fts=nav["gmap_pos_fts"], gmap_masks=nav["gmap_masks"], gmap_pair_dists=nav["gmap_pair_dists"],
                        gmap_visited_masks=nav["gmap_visited_masks"], bev_fts=bev_fts, bev_pos_fts=bev["bev_pos_fts"],
                        bev_masks=bev["bev_masks"], bev_nav_masks=bev["bev_nav_masks"], bev_cand_idxs=bev["bev_cand_idxs"],
                        obj_embeds=None, obj_masks=None)
            dev_out = model.forward_navigation_per_step(gmap_vpids=None, bev_cand_vpids=None,
                                                        sap_fusion=(bev["src"], bev["vis_c"]), **args)

            def names(ids, n):
                return [[None if i < 0 else (f"g{i - m.N}" if i >= m.N else str(i)) for i in row[:k]]
                        for row, k in zip(ids.tolist(), n.tolist())]
            host_out = model.forward_navigation_per_step(
                gmap_vpids=names(nav["gmap_ids"], nav["gmap_masks"].sum(1)),
                bev_cand_vpids=names(bev["bev_cand_ids"], bev["bev_cand_count"]), **args)
            a, b = dev_out["fused_logits"], host_out["fused_logits"]
            fin = torch.isfinite(b)
            print(f"step {t}: {int(fin.sum())} finite fused logits, candidates {bev['bev_cand_count'].tolist()}, "
                  f"max |device - host| {float((a[fin] - b[fin]).abs().max()):.1e}")
            assert torch.equal(a, b) and int(fin.sum()) >= 2 * B
            m.record_stop_scores(torch.softmax(a, 1)[:, 0])
            a_t = a.argmax(1)
            rec = m.act(a_t)
            for b_, act in enumerate(m.to_reference(rec)):          # move to the chosen ghost (or stay)
                if act["action"]["act"] == 4:
                    pos[b_] = act["action"]["ghost_pos"]
    assert m.check_overflow() == 0
