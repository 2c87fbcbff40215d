"""Regenerate tests/golden/ce_map.npz from the reference's own code.

Build machine only (the reference is read from REF, imported -- not copied), with the stand-in technique of
make_waypoint_golden.py (its module finder is reused):
  * vlnce_baselines/models/graph_utils.py GraphMap (identify_node, update_graph, update_node_pc, delete_ghost, ...) on the
    real networkx; heading_from_quaternion is patched, in graph_utils and in the trainer module, to read the heading from
    a stand-in orientation (the orientation IS the heading);
  * vlnce_baselines/ss_trainer_BEV.py RLTrainer._nav_gmap_variable, _nav_bev_variable, _discretize_polar_relpos and
    _teacher_action_new on a stand-in ``self`` (gmaps, envs.num_envs / call_at, bev_dim = 11, bev_res = 1, bev_pos from the
    reference's bevpos_polar, config.VIDEO_OPTION = [] / IL.expert_policy = 'spl');
  * RLTrainer.lift and RLTrainer.splat themselves, on the reference's PointCloud projector (CPU), with torch_scatter's
    scatter_mean replaced by the stub make_golden.py defines: every step's panorama (grid features and depths from
    tests/ce_map_ref.grids) is lifted and stored with update_node_pc, _nav_bev_variable gathers with
    gather_node_pc(cur, order=1) as the trainer does, and the same gather + splat is repeated with order=2 so that the
    ``len(path) <= order`` choice is exercised on stored neighbours (bev_fts_o2).  Of the 768 channels every 16th is
    stored, next to each cell's sum over all channels;
  * the action block (ss_trainer_BEV.py:1110-1179) is inline code of ``rollout``: it is restated here line by line on the
    reference's own GraphMap objects (stop rule, np.argmax of node_stop_scores, front_to_ghost_dist, shortest_path[..][1:],
    prev_vp = front_vp, delete_ghost).
Three scripted episodes, B = 3, 6 steps, at most 5 candidates, H = 32, loc_noise 0.5; map 2 has merge_ghost off.  By
name (each asserted below): a candidate localized to an old node; a candidate localized to the current node itself; a
merge across two steps; a merge within one step; a ghost consumed and a later candidate at the same place getting a new
id; a change of the nearest front; both sides of the b[2] > a[2] branch; an episode ending early (map 2 stops at step
4; map 1 runs out of ghosts at step 3); no ghost left.  Margins that keep discrete decisions off rounding are asserted:
every _localize distance > 1e-3 from loc_noise, rival minima and rival path lengths > 1e-6 apart, every pre-round BEV
coordinate > 1e-3 from a half.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
B, T, C, H, L, N, LOC = 3, 6, 5, 32, 17, 16, 0.5
MERGE = (True, True, False)

# (position, heading, candidate targets (x, z), action: ghost id to go to / "stop")
EPISODES = [
    [((0, 0, 0), 0.3, [(2, 0), (0, 2.5), (-2, 0.5), (3, 3)], 0),
     ((2.05, 0.1, 0.05), 1.0, [(0.1, 0.1), (0.1, 2.6), (4, 0), (2.15, 0.15)], 4),
     ((4.0, 0.1, -0.1), 2.0, [(3.1, 2.8), (6, 0), (6.2, 0.2), (4, -2)], 3),
     ((3.0, 0.2, 2.95), 4.0, [(3, 5), (0.3, 2.4)], 7),
     ((3.1, 0.2, 5.0), 5.5, [(3.05, 2.9), (5, 6)], 8),
     ((5, 0.2, 6.1), 0.9, [(6, 7)], 9)],
    [((10, 1, 10), 0.0, [(12, 10)], 0),
     ((12.0, 1, 10.9), 3.0, [(12, 10), (14, 11)], 1),
     ((12.05, 1, 10.02), 1.5, [(12.0, 10.8), (14.1, 11.2)], 2),
     ((14, 1, 11), 0.7, [(12.1, 10.1)], 5)],
    [((-5, 0, -5), 6.0, [(-3, -5), (-3.2, -5.1), (-5, -3)], 1),
     ((-3.2, 0.05, -5.1), 2.2, [(-5, -3.1), (-1, -5), (-4.9, -5.05)], 4),
     ((-1, 0.05, -5), 0.1, [(-1, -7), (-1, -3)], 2),
     ((-5, 0, -3.05), 3.3, [(-5, -1)], 7),
     ((-5, 0, -1), 4.4, [(-7, -1)], "stop")],
]


def polar(pos, heading, tx, tz):
    """float32 (angle, distance) that estimate_cand_pos maps (close) to (tx, tz)."""
    dx, dz = pos[0] - tx, pos[2] - tz
    return np.float32((np.arctan2(dx, dz) - heading) % (2 * np.pi)), np.float32(np.hypot(dx, dz))


def main():
    spec = importlib.util.spec_from_file_location("make_waypoint_golden", os.path.join(HERE, "make_waypoint_golden.py"))
    mw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mw)
    assert os.path.isdir(mw.REF), "the reference is only mounted in the build container"
    mw.REAL = mw.REAL + ("vlnce_baselines.models.graph_utils", "vlnce_baselines.models.bev_utils")
    mw._stand_ins()
    for name in ("matplotlib", "matplotlib.pyplot"):               # imported by graph_utils, never used
        sys.modules[name] = mw._StubModule(name)
    if not hasattr(np, "int"):
        np.int = int
    from vlnce_baselines.models import graph_utils as gu
    from vlnce_baselines.models.bev_utils import bevpos_polar
    from vlnce_baselines import ss_trainer_BEV as trn
    gu.heading_from_quaternion = trn.heading_from_quaternion = lambda ori: ori
    from vlnce_baselines.models import bev_utils
    from torch.nn.utils.rnn import pad_sequence
    from tests import ce_map_ref as CR
    import math

    def scatter_mean(src, index, dim=0, dim_size=None):            # the stub of make_golden.py
        assert dim == 0
        out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype)
        out.index_add_(0, index, src)
        cnt = torch.zeros(dim_size, dtype=src.dtype)
        cnt.index_add_(0, index, torch.ones_like(index, dtype=src.dtype))
        cnt.clamp_(min=1)
        return out / cnt.view(-1, *([1] * (src.dim() - 1)))
    bev_utils.scatter_mean = scatter_mean
    projector = bev_utils.PointCloud(math.radians(90), 1, feature_map_height=14, feature_map_width=14, map_dim=11, map_res=1,
                                     world_shift_origin=torch.FloatTensor([0, 0, 0]), z_clip_threshold=0.5,
                                     device=torch.device("cpu"))

    rng = np.random.default_rng(5)
    inp = {"cur_pos": np.zeros((T, B, 3)), "heading": np.zeros((T, B)), "live": np.zeros((T, B), bool),
           "cand_count": np.zeros((T, B), np.int32), "cand_angles": np.zeros((T, B, C), np.float32),
           "cand_distances": np.zeros((T, B, C), np.float32),
           "avg_pano": (rng.integers(-16, 16, (T, B, H)) / 8).astype(np.float32),
           "pano": (rng.integers(-16, 16, (T, B, L, H)) / 8).astype(np.float32), "nav_types": np.zeros((T, B, L), np.int64),
           "a_t": np.zeros((T, B), np.int64), "probs0": rng.permutation(T * B).reshape(T, B).astype(np.float32) / (T * B + 1),
           "cur_dist": rng.uniform(0.5, 6.0, (T, B)), "ghost_dist": rng.permutation(T * B * 5 * N).reshape(T, B, 5 * N) * 0.01 + 2.0}
    inp["cur_dist"][2, 0] = 1.2                                    # the < 1.5 rule of the teacher
    G = 1 + N + 5 * N
    K = 16
    out = {"cand_slot": np.full((T, B, C), -1, np.int64), "n_nodes": np.zeros((T, B), np.int64),
           "node_pos": np.zeros((T, B, N, 3)), "dist": np.full((T, B, N, N), np.inf), "hops": np.zeros((T, B, N, N), np.int64),
           "ghost_alive": np.zeros((T, B, 5 * N), bool), "ghost_mean": np.zeros((T, B, 5 * N, 3)),
           "ghost_nfronts": np.zeros((T, B, 5 * N), np.int64), "ghost_fronts": np.full((T, B, 5 * N, 16), -1, np.int64),
           "gmap_ids": np.full((T, B, G), -1, np.int64), "gmap_step_ids": np.zeros((T, B, G), np.int64),
           "gmap_visited_masks": np.zeros((T, B, G), bool), "gmap_masks": np.zeros((T, B, G), bool),
           "gmap_img_fts": np.zeros((T, B, G, H), np.float32), "gmap_pos_fts": np.zeros((T, B, G, 7), np.float32),
           "gmap_pair_dists": np.zeros((T, B, G, G), np.float32), "no_vp_left": np.zeros((T, B), bool),
           "bev_nav_masks": np.zeros((T, B, 121), bool), "bev_cand_idxs": np.zeros((T, B, K), np.int64),
           "bev_cand_ids": np.full((T, B, K), -1, np.int64), "bev_cand_count": np.zeros((T, B), np.int64),
           "bev_pos_fts": np.zeros((T, B, 121, 10), np.float32), "teacher": np.full((T, B), -100, np.int64),
           "act": np.full((T, B), -1, np.int64), "act_target": np.full((T, B), -1, np.int64),
           "act_ghost": np.full((T, B), -1, np.int64), "act_path_len": np.zeros((T, B), np.int64),
           "bev_fts": np.zeros((T, B, 121, 48), np.float32), "bev_fts_sum": np.zeros((T, B, 121)),
           "bev_fts_o2": np.zeros((T, B, 121, 48), np.float32), "bev_fts_o2_sum": np.zeros((T, B, 121)),
           "bev_nodes_o2": np.zeros((T, B), np.int64),
           "act_path": np.full((T, B, N), -1, np.int64), "act_target_pos": np.zeros((T, B, 3)), "act_ghost_pos": np.zeros((T, B, 3))}
    seen = set()

    def vid(vp):                                                   # the reference's string ids -> integers
        return -1 if vp is None else (N + int(vp[1:]) if vp.startswith("g") else int(vp))

    gmaps = [gu.GraphMap(True, LOC, MERGE[b], 0) for b in range(B)]
    prev_vp = [None] * B
    done = [False] * B
    real_localize = gu.GraphMap._localize

    def spy_localize(self, qpos, kpos_dict, ignore_height=False):
        ds = sorted(float(((qpos - k) ** 2).sum() ** 0.5) for k in kpos_dict.values())
        if ds:
            assert abs(ds[0] - LOC) > 1e-3, ("localize margin", ds[0])
            assert len(ds) < 2 or ds[1] - ds[0] > 1e-6, ("rival minima", ds[:2])
        return real_localize(self, qpos, kpos_dict, ignore_height)
    gu.GraphMap._localize = spy_localize
    real_front = gu.GraphMap.front_to_ghost_dist

    def spy_front(self, ghost_vp):
        ds = sorted({f: gu.calc_position_distance(self.node_pos[f], self.ghost_aug_pos[ghost_vp])
                     for f in self.ghost_fronts[ghost_vp]}.values())
        assert len(ds) < 2 or ds[1] - ds[0] > 1e-6, ("rival fronts", ds[:2])
        return real_front(self, ghost_vp)
    gu.GraphMap.front_to_ghost_dist = spy_front
    real_disc = trn.RLTrainer._discretize_polar_relpos

    def spy_disc(self, rel):
        for v in (rel[:, 1] * np.sin(rel[:, 0]) / self.bev_res, rel[:, 1] * np.cos(rel[:, 0]) / self.bev_res):
            assert np.all(np.abs(np.abs(v - np.floor(v)) - 0.5) > 1e-3), ("BEV coordinate near a half", v)
        return real_disc(self, rel)

    for t in range(T):
        live = [b for b in range(B) if not done[b] and t < len(EPISODES[b])]
        inp["live"][t, live] = True
        cur_vp, cur_pos, cur_ori = [], [], []
        rgb_grid, depth_grid = (torch.from_numpy(x) for x in CR.grids(t, B))
        lstand = types.SimpleNamespace(envs=types.SimpleNamespace(num_envs=len(live)), projector=projector)
        pcs = trn.RLTrainer.lift(lstand, [np.array(EPISODES[b][t][0], dtype=np.float64) for b in live],
                                 [EPISODES[b][t][1] for b in live], rgb_grid[live], depth_grid[live]) if live else None
        for li, b in enumerate(live):
            pos, heading, targets, _ = EPISODES[b][t]
            pos = np.array(pos, dtype=np.float64)
            k = len(targets)
            inp["cur_pos"][t, b], inp["heading"][t, b], inp["cand_count"][t, b] = pos, heading, k
            for j, (tx, tz) in enumerate(targets):
                inp["cand_angles"][t, b, j], inp["cand_distances"][t, b, j] = polar(pos, heading, tx, tz)
            inp["nav_types"][t, b, :k] = 1
            gm = gmaps[b]
            ang, dis = inp["cand_angles"][t, b, :k].tolist(), inp["cand_distances"][t, b, :k].tolist()
            vp, cvp, cpos = gm.identify_node(pos, heading, ang, dis)
            before_nodes = {v: p.copy() for v, p in gm.node_pos.items()}
            before_ghosts = {g: list(f) for g, f in gm.ghost_fronts.items()}
            before_front = {g: gm.front_to_ghost_dist(g)[1] for g in gm.ghost_fronts} if t else {}
            pano = torch.from_numpy(inp["pano"][t, b])
            cemb = pano[torch.from_numpy(inp["nav_types"][t, b]) == 1]
            gm.update_graph(prev_vp[b], t + 1, vp, pos, torch.from_numpy(inp["avg_pano"][t, b]), cvp, cpos, cemb,
                            [(t, b, j) for j in range(k)])
            gm.update_node_pc(vp, pcs[0][li], pcs[1][li], pcs[2][li])
            # which id each candidate went to: replay _localize on the state before / after (the reference keeps no record)
            fronts_now = {g: list(f) for g, f in gm.ghost_fronts.items()}
            tokens = {tok: g for g, toks in gm.ghost_real_pos.items() for tok in toks}
            for j in range(k):
                if (t, b, j) in tokens:
                    g = tokens[(t, b, j)]
                    out["cand_slot"][t, b, j] = vid(g)
                    if g in before_ghosts:
                        seen.add("merge across two steps")
                    elif sum(tokens[(t, b, i)] == g for i in range(k) if (t, b, i) in tokens) > 1:
                        seen.add("merge within one step")
                else:
                    d = {v: np.linalg.norm(cpos[j] - p) for v, p in gm.node_pos.items()}
                    v = min(d, key=d.get)
                    assert d[v] < LOC
                    out["cand_slot"][t, b, j] = vid(v)
                    seen.add("localized to the current node itself" if v == vp else "localized to an old node")
                    assert v == vp or v in before_nodes
            for g in fronts_now:
                if g in before_front and gm.front_to_ghost_dist(g)[1] != before_front[g]:
                    seen.add("change of the nearest front")
            cur_vp.append(vp); cur_pos.append(pos); cur_ori.append(heading)
            # rival path lengths: every other way into v must be longer by > 1e-6
            for s in gm.shortest_dist:
                for v, dv in gm.shortest_dist[s].items():
                    path = gm.shortest_path[s][v]
                    for u, w in gm.graph_nx[v].items():
                        if u != v and (len(path) < 2 or u != path[-2]):
                            assert gm.shortest_dist[s][u] + w["weight"] - dv > 1e-6, ("rival path", s, v, u)
            nn = len(gm.node_pos)
            out["n_nodes"][t, b] = nn
            for v, p in gm.node_pos.items():
                out["node_pos"][t, b, int(v)] = p
            for x in gm.shortest_dist:
                for y, d in gm.shortest_dist[x].items():
                    out["dist"][t, b, int(x), int(y)] = d
                    out["hops"][t, b, int(x), int(y)] = len(gm.shortest_path[x][y])
            for g in gm.ghost_pos:
                gi = int(g[1:])
                out["ghost_alive"][t, b, gi] = True
                out["ghost_mean"][t, b, gi] = gm.ghost_mean_pos[g]
                f = [int(x) for x in gm.ghost_fronts[g]]
                out["ghost_nfronts"][t, b, gi] = len(f)
                out["ghost_fronts"][t, b, gi, :len(f)] = f
                if len(f) != len(set(f)):
                    seen.add("fronts with duplicates")
        if not live:
            continue
        stand = types.SimpleNamespace(
            gmaps=[gmaps[b] for b in live], bev_dim=11, bev_res=1, bev_pos=bevpos_polar(11)[None],
            config=types.SimpleNamespace(VIDEO_OPTION=[], IL=types.SimpleNamespace(expert_policy="spl")))
        stand.envs = types.SimpleNamespace(num_envs=len(live))
        stand._discretize_polar_relpos = lambda rel: spy_disc(stand, rel)
        stand.projector = projector
        stand.splat = lambda *a: trn.RLTrainer.splat(stand, *a)
        nav = trn.RLTrainer._nav_gmap_variable(stand, cur_vp, cur_pos, cur_ori)
        bev = trn.RLTrainer._nav_bev_variable(stand, cur_vp, cur_pos, cur_ori)
        assert bool(bev["bev_masks"].all())
        o2 = [gm.gather_node_pc(vp, order=2) for gm, vp in zip(stand.gmaps, cur_vp)]       # as _nav_bev_variable collates
        bev2, _, _ = stand.splat(cur_pos, cur_ori, pad_sequence([x[0] for x in o2], batch_first=True),
                                 pad_sequence([x[1] for x in o2], batch_first=True, padding_value=True),
                                 pad_sequence([x[2] for x in o2], batch_first=True))

        def call_at(i, name, args=None):
            if name == "current_dist_to_goal":
                return inp["cur_dist"][t, live[i]]
            g = [g for g, toks in stand.gmaps[i].ghost_real_pos.items() if args["pos"] in toks][0]
            return inp["ghost_dist"][t, live[i], int(g[1:])]
        stand.envs.call_at = call_at
        stand.envs.current_episodes = lambda: [None] * len(live)
        teacher = trn.RLTrainer._teacher_action_new(stand, nav["gmap_vp_ids"], nav["no_vp_left"]).numpy()
        for i, b in enumerate(live):
            gm, ids = gmaps[b], nav["gmap_vp_ids"][i]
            n = len(ids)
            out["gmap_ids"][t, b, :n] = [vid(v) for v in ids]
            out["gmap_step_ids"][t, b, :nav["gmap_step_ids"].shape[1]] = nav["gmap_step_ids"][i].numpy()
            out["gmap_visited_masks"][t, b, :nav["gmap_visited_masks"].shape[1]] = nav["gmap_visited_masks"][i].numpy()
            out["gmap_masks"][t, b, :nav["gmap_masks"].shape[1]] = nav["gmap_masks"][i].numpy()
            m = nav["gmap_img_fts"].shape[1]
            out["gmap_img_fts"][t, b, :m] = nav["gmap_img_fts"][i].numpy()
            out["gmap_pos_fts"][t, b, :m] = nav["gmap_pos_fts"][i].numpy()
            out["gmap_pair_dists"][t, b, :m, :m] = nav["gmap_pair_dists"][i].numpy()
            out["no_vp_left"][t, b] = nav["no_vp_left"][i]
            out["bev_nav_masks"][t, b] = bev["bev_nav_masks"][i].numpy()
            cv = bev["bev_cand_vpids"][i]
            out["bev_cand_count"][t, b] = len(cv)
            out["bev_cand_ids"][t, b, :len(cv)] = [vid(v) for v in cv]
            out["bev_cand_idxs"][t, b, :len(cv)] = bev["bev_cand_idxs"][i].numpy()[:len(cv)]
            out["bev_pos_fts"][t, b] = bev["bev_pos_fts"][i].numpy()
            out["teacher"][t, b] = teacher[i]
            for key, fts in (("bev_fts", bev["bev_fts"][i]), ("bev_fts_o2", bev2[i])):
                out[key][t, b], out[key + "_sum"][t, b] = fts[:, ::16].numpy(), fts.double().sum(1).numpy()
            out["bev_nodes_o2"][t, b] = o2[i][0].shape[0] // (12 * 196)
            if o2[i][0].shape[0] > 12 * 196:
                seen.add("order 2 gathers stored neighbours")
            if (bev["bev_fts"][i] != 0).any(1).sum() >= 10:
                seen.add("BEV cells filled")
            for v in ids[1:]:
                if not v.startswith("g"):
                    seen.add("b[2] > a[2]" if gm.node_pos[v][2] > cur_pos[i][2] else "b[2] <= a[2]")
            if nav["no_vp_left"][i]:
                seen.add("no ghost left")
            # ss_trainer_BEV.py:1083-1084, :1110-1179
            gm.node_stop_scores[cur_vp[i]] = float(inp["probs0"][t, b])
            want = EPISODES[b][t][3]
            a = 0 if want == "stop" or f"g{want}" not in ids else ids.index(f"g{want}")
            inp["a_t"][t, b] = a
            if a == 0 or t == T - 1 or nav["no_vp_left"][i]:
                vs = [(vp, s) for vp, s in gm.node_stop_scores.items()]
                stop_vp = vs[np.argmax([s[1] for s in vs])][0]
                back = gm.shortest_path[cur_vp[i]][stop_vp][1:]
                out["act"][t, b], out["act_target"][t, b], out["act_target_pos"][t, b] = 0, int(stop_vp), gm.node_pos[stop_vp]
                done[b] = True
                if t < T - 1:
                    seen.add("episode ending early")
            else:
                ghost_vp = ids[a]
                ghost_pos = gm.ghost_aug_pos[ghost_vp]
                _, front_vp = gm.front_to_ghost_dist(ghost_vp)
                back = gm.shortest_path[cur_vp[i]][front_vp][1:]
                out["act"][t, b], out["act_target"][t, b], out["act_target_pos"][t, b] = 4, int(front_vp), gm.node_pos[front_vp]
                out["act_ghost"][t, b], out["act_ghost_pos"][t, b] = int(ghost_vp[1:]), ghost_pos
                prev_vp[b] = front_vp
                gm.delete_ghost(ghost_vp)
                seen.add(("consumed", b, tuple(np.round(ghost_pos, 1))))
            out["act_path_len"][t, b] = len(back)
            out["act_path"][t, b, :len(back)] = [int(v) for v in back]
            if len(back) > 1:
                seen.add("multi-hop back_path")
    # a ghost consumed and a later candidate at the same place getting a new id: map 1, (12, 10)
    assert ("consumed", 1, (12.0, 1.0, 10.0)) in seen and out["cand_slot"][1, 1, 0] == N + 1 and out["cand_slot"][0, 1, 0] == N
    for name in ("localized to an old node", "localized to the current node itself", "merge across two steps",
                 "merge within one step", "change of the nearest front", "b[2] > a[2]", "b[2] <= a[2]",
                 "episode ending early", "no ghost left", "fronts with duplicates", "multi-hop back_path",
                 "order 2 gathers stored neighbours", "BEV cells filled"):
        assert name in seen, name
    assert not MERGE[2] and out["cand_slot"][0, 2, 1] == N + 1      # merge off: a new ghost next to ghost 0
    path = os.path.join(HERE, "ce_map.npz")
    np.savez_compressed(path, loc_noise=np.array(LOC), merge_ghost=np.array(MERGE), **{"in_" + k: v for k, v in inp.items()},
                        **out)
    print("ce_map.npz", os.path.getsize(path), "bytes; live:", inp["live"].sum(0), "nodes:", out["n_nodes"].max(0))


if __name__ == "__main__":
    main()
