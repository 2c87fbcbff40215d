"""tests/ce_map_ref.py (the numpy restatement of the CE agent's ghost-node map) pinned to the reference's recorded outputs
(tests/golden/ce_map.npz, made by tests/golden/make_ce_map_golden.py from the reference's own GraphMap and trainer
methods).  CPU only.  Integers exactly, float64 to 1e-12 (same formulas, numpy against numpy + networkx), float32 features
to 2e-7 (float32 sin / cos of equal arguments)."""
import os

import numpy as np
import pytest

from tests import ce_map_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ce_map.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def run(gold):
    """The restatement driven through the recorded episodes: per step, its outputs."""
    return R.replay(gold)


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0.0))


def test_graph_state_equals_the_reference(gold, run):
    for t, o in enumerate(run):
        s = o["state"]
        for k in ("n_nodes", "hops", "ghost_alive", "ghost_nfronts", "ghost_fronts"):
            assert np.array_equal(s[k], gold[k][t]), (t, k)
        assert np.array_equal(o["cand_slot"], gold["cand_slot"][t]), t
        fin = np.isfinite(gold["dist"][t])
        assert np.array_equal(np.isfinite(s["dist"]), fin)
        e = (_err(s["node_pos"], gold["node_pos"][t]), _err(s["dist"][fin], gold["dist"][t][fin]),
             _err(s["ghost_mean"], gold["ghost_mean"][t]))
        print(f"step {t}: node_pos {e[0]:.1e} dist {e[1]:.1e} ghost_mean {e[2]:.1e}")
        assert max(e) <= 1e-12


def test_navigation_variables_equal_the_reference(gold, run):
    for t, o in enumerate(run):
        for k in ("gmap_ids", "gmap_step_ids", "gmap_visited_masks", "gmap_masks", "no_vp_left"):
            assert np.array_equal(o[k], gold[k][t]), (t, k)
        e = {k: _err(o[k], gold[k][t]) for k in ("gmap_img_fts", "gmap_pos_fts", "gmap_pair_dists")}
        print(f"step {t}:", e)
        assert e["gmap_img_fts"] == 0.0 and e["gmap_pos_fts"] <= 2e-7 and e["gmap_pair_dists"] <= 2e-7


def test_bev_candidates_equal_the_reference(gold, run):
    bev_pos = gold["bev_pos_fts"]
    for t, o in enumerate(run):
        for k in ("bev_nav_masks", "bev_cand_count"):
            assert np.array_equal(o[k], gold[k][t]), (t, k)
        K = gold["bev_cand_ids"].shape[-1]
        assert np.array_equal(o["bev_cand_ids"][:, :K], gold["bev_cand_ids"][t]) and (o["bev_cand_ids"][:, K:] == -1).all()
        assert np.array_equal(o["bev_cand_idxs"][:, :K], gold["bev_cand_idxs"][t])
        live = gold["in_live"][t]
        e = _err(o["bev_gpos_fts"][live], bev_pos[t][live][:, 0, :7])
        print(f"step {t}: start-node position features {e:.1e}")
        assert e <= 2e-7
        assert (bev_pos[t][live][:, :, :7] == bev_pos[t][live][:, :1, :7]).all()


def test_fusion_indices_equal_the_host_builder_on_string_ids(gold, run):
    from vln_bevbert_amd.pretrain_cmt import sap_fusion_indices
    N = gold["node_pos"].shape[2]

    def name(i):
        return None if i < 0 else (f"g{i - N}" if i >= N else str(i))
    for t, o in enumerate(run):
        for b in np.nonzero(gold["in_live"][t])[0]:
            n, c = int(o["gmap_masks"][b].sum()), int(o["bev_cand_count"][b])
            G, K = o["src"].shape[1], o["vis_c"].shape[1]
            src, vis = sap_fusion_indices([[name(i) for i in o["gmap_ids"][b, :n]]], [o["gmap_visited_masks"][b, :n]],
                                          [[name(i) for i in o["bev_cand_ids"][b, :c]]], G, K)
            assert np.array_equal(src[0], o["src"][b]) and np.array_equal(vis[0], o["vis_c"][b]), (t, b)


def test_teacher_and_actions_equal_the_reference(gold, run):
    for t, o in enumerate(run):
        assert np.array_equal(o["teacher"], gold["teacher"][t]), t
        for b, a in enumerate(o["actions"]):
            if a is None:
                assert gold["act"][t, b] == -1
                continue
            tgt = a["stop_vp"] if a["act"] == 0 else a["front_vp"]
            n = int(gold["act_path_len"][t, b])
            assert (a["act"], tgt, a.get("ghost_vp", -1), a["back_path"]) == \
                (gold["act"][t, b], gold["act_target"][t, b], gold["act_ghost"][t, b], gold["act_path"][t, b, :n].tolist())
            assert _err(a["stop_pos"] if a["act"] == 0 else a["front_pos"], gold["act_target_pos"][t, b]) <= 1e-12
            if a["act"] == 4:
                assert _err(a["ghost_pos"], gold["act_ghost_pos"][t, b]) <= 1e-12


def test_dijkstra_sums_in_path_order():
    # 0 - 1 - 2 with weights whose float64 sum depends on the order: dist[0][2] = (a + b), dist[2][0] = (b + a) equal, but
    # a three-edge path 0 - 1 - 2 - 3 distinguishes (a + b) + c from (c + b) + a
    a, b, c = 0.1, 0.2, 0.3
    W = np.full((4, 4), -1.0)
    for i, w in enumerate((a, b, c)):
        W[i, i + 1] = W[i + 1, i] = w
    d, h, p = R.dijkstra_all(W, 4)
    assert d[0, 3] == (a + b) + c and d[3, 0] == (c + b) + a and d[0, 3] != d[3, 0]
    assert h[0, 3] == 4 and h[1, 1] == 1 and p[0, 3] == 2 and p[3, 0] == 1
