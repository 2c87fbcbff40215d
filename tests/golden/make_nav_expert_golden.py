"""Regenerate tests/golden/nav_expert.npz and tests/golden/nav_scans.npz from the reference's own code.

Build machine only (the reference is read from REF, imported -- not copied):
  * utils/data.py load_nav_graphs + networkx all_pairs_dijkstra_path{,_length} (r2r/env.py:160-167);
  * r2r/agent.py GMapNavAgent._teacher_action_r4r on a stand-in `self` (args.ignoreid / expert_policy, env tables),
    for expert_policy 'spl' and 'ndtw', with imitation_learning False and True;
  * r2r/env.py R2RNavBatch._eval_item / eval_metrics on a stand-in env; r2r/eval_utils.py cal_dtw / cal_cls.
Stubs: MatterSim, cv2, line_profiler, jsonlines, h5py, torch_scatter and models.bev_visualize (imported at module
level, unused on these paths); torch.Tensor.cuda is the identity (the expert ends with .cuda()).

nav_scans.npz holds three scans' connectivity as arrays (image ids, included flags, unobstructed matrix, 4x4 poses);
the CPU test writes them back as <scan>_connectivity.json.  nav_expert.npz holds the networkx tables, the fixture states
(node indices in networkx node order) and the reference's outputs.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SCANS = ("8194nk5LbLH", "17DRP5sb8fy", "5ZKStnWn8Zo")   # 20, 44 and 163 included nodes
IGNOREID = -100


def _stubs():
    for name in ("MatterSim", "cv2", "line_profiler", "jsonlines", "h5py", "torch_scatter"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torch_scatter"].scatter_max = sys.modules["torch_scatter"].scatter_mean = None
    viz = sys.modules["models.bev_visualize"] = types.ModuleType("models.bev_visualize")   # opens a simulator on import
    viz.draw_ob = None
    sys.modules["line_profiler"].LineProfiler = lambda *a, **k: None
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(REF, "map_nav_src"))


def _scan_arrays(scan):
    with open(os.path.join(REF, "precompute_features/connectivity", f"{scan}_connectivity.json")) as f:
        data = json.load(f)
    return {"ids": np.array([x["image_id"] for x in data]), "included": np.array([x["included"] for x in data]),
            "unobstructed": np.array([x["unobstructed"] for x in data], dtype=bool),
            "pose": np.array([x["pose"] for x in data], dtype=np.float64)}


def _random_walk(rng, G, start, n):
    out = [start]
    for _ in range(n):
        nb = list(G.neighbors(out[-1]))
        out.append(nb[rng.integers(len(nb))])
    return out


def _gt_path(rng, G, sp, start, lo, hi):
    """A walk of lo..hi nodes through shortest paths between random waypoints (RxR-like), no immediate repeats."""
    nodes = list(G.nodes)
    want = int(rng.integers(lo, hi + 1))
    path = [start]
    while len(path) < want:
        w = nodes[rng.integers(len(nodes))]
        if w != path[-1] and w in sp[path[-1]]:
            path += sp[path[-1]][w][1:]
    return path[:want]


def main():
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    _stubs()
    import networkx as nx
    from utils.data import load_nav_graphs
    from r2r import agent as ref_agent
    from r2r import env as ref_env
    from r2r.eval_utils import cal_cls, cal_dtw

    raw = {s: _scan_arrays(s) for s in SCANS}
    with tempfile.TemporaryDirectory() as d:
        for s, a in raw.items():
            with open(os.path.join(d, f"{s}_connectivity.json"), "w") as f:
                json.dump([{"image_id": str(i), "included": bool(inc), "unobstructed": [bool(u) for u in un],
                            "pose": [float(p) for p in po]}
                           for i, inc, un, po in zip(a["ids"], a["included"], a["unobstructed"], a["pose"])], f)
        graphs = load_nav_graphs(d, SCANS)
    sp = {s: dict(nx.all_pairs_dijkstra_path(G)) for s, G in graphs.items()}
    sd = {s: dict(nx.all_pairs_dijkstra_path_length(G)) for s, G in graphs.items()}
    ids = {s: list(G.nodes) for s, G in graphs.items()}
    idx = {s: {vp: i for i, vp in enumerate(ids[s])} for s in SCANS}
    N = max(len(v) for v in ids.values())

    out = {}
    scans_npz = {}
    for si, s in enumerate(SCANS):
        for k, v in raw[s].items():
            scans_npz[f"{s}/{k}"] = v
        n = len(ids[s])
        dist = np.full((N, N), np.inf)
        flat, start = [], [0]
        for u in range(n):
            for v in range(n):
                dist[u, v] = sd[s][ids[s][u]].get(ids[s][v], np.inf)
                p = sp[s][ids[s][u]].get(ids[s][v], [])
                flat += [idx[s][x] for x in p]
                start.append(len(flat))
        out[f"dist_{si}"] = dist
        out[f"paths_{si}"] = np.array(flat, dtype=np.int16)
        out[f"path_start_{si}"] = np.array(start, dtype=np.int32)
        out[f"ids_{si}"] = np.array(ids[s])
    out["scans"] = np.array(SCANS)

    rng = np.random.default_rng(2024)

    class Args:
        ignoreid = IGNOREID
        expert_policy = "spl"

    class Env:
        shortest_distances = sd
        shortest_paths = sp

    stand_in = types.SimpleNamespace(args=Args(), env=Env())

    # ---------------- expert cases: one batch of B states per (policy, imitation, gt size)
    B = 24
    cases = [("spl", False, 4, 12), ("ndtw", False, 4, 12), ("ndtw", False, 20, 40), ("ndtw", False, 60, 100),
             ("spl", True, 4, 12), ("ndtw", True, 20, 40)]
    for ci, (policy, il, lo, hi) in enumerate(cases):
        Args.expert_policy = policy
        obs, vpids, ended, visited, trajs = [], [], [], [], []
        t = int(rng.integers(0, 5)) if il else 0
        for b in range(B):
            s = SCANS[b % 3] if hi <= 40 else SCANS[2]
            G = graphs[s]
            nodes = ids[s]
            start = nodes[rng.integers(len(nodes))]
            gt = _gt_path(rng, G, sp[s], start, max(lo, t + 1), max(hi, t + 1))
            if il:                          # the batch shares step t; cur = gt[t]
                if b % 5 == 4:
                    gt = gt[:t + 1]         # at the last ground-truth step: stop
                walk = gt[:t + 1]
                traj_segs = [[walk[0]]] + [[x] for x in walk[1:]]
                cur = walk[-1]
            else:
                walk = _random_walk(rng, G, start, int(rng.integers(0, 8 if hi <= 40 else 30)))
                traj_segs = [[walk[0]]] + [[x] for x in walk[1:]]
                cur = walk[-1]
                if b % 7 == 6:
                    cur = gt[-1]            # arrived: stop
                    traj_segs.append(sp[s][walk[-1]][cur][1:] or [cur])
            k = int(rng.integers(2, 12))
            cands = list(dict.fromkeys([nodes[rng.integers(len(nodes))] for _ in range(k)] + list(G.neighbors(cur))))
            if il and t < len(gt) - 1 and b % 6 != 5 and gt[t + 1] not in cands:
                cands.insert(int(rng.integers(len(cands) + 1)), gt[t + 1])
            vis = [False] + [bool(rng.random() < 0.3) for _ in cands]
            if b % 11 == 10:
                vis = [False] + [True] * len(cands)     # every candidate excluded: min_idx stays ignoreid
            obs.append({"scan": s, "viewpoint": cur, "gt_path": gt})
            vpids.append([None] + cands)
            ended.append(b % 9 == 8)
            visited.append(vis)
            trajs.append({"path": traj_segs})
        tgt = ref_agent.GMapNavAgent._teacher_action_r4r(stand_in, obs, vpids, ended, visited_masks=visited,
                                                         imitation_learning=il, t=t, traj=trajs).numpy()
        C = max(len(v) for v in vpids)
        Lg = max(len(o["gt_path"]) for o in obs)
        flat = [sum(tr["path"], []) for tr in trajs]
        Lt = max(len(f) for f in flat)
        pre = f"exp{ci}_"
        out[pre + "policy"] = np.array("imitation" if il else policy)
        out[pre + "scan"] = np.array([SCANS.index(o["scan"]) for o in obs], dtype=np.int32)
        out[pre + "cur"] = np.array([idx[o["scan"]][o["viewpoint"]] for o in obs], dtype=np.int32)
        out[pre + "t"] = np.array(t, dtype=np.int32)
        cand = np.full((B, C), -1, dtype=np.int32)
        vm = np.zeros((B, C), dtype=np.uint8)
        gta = np.full((B, Lg), -1, dtype=np.int32)
        tra = np.full((B, Lt), -1, dtype=np.int32)
        for b in range(B):
            s = obs[b]["scan"]
            for j, vp in enumerate(vpids[b][1:]):
                cand[b, j + 1] = idx[s][vp]
            vm[b, :len(visited[b])] = visited[b]
            gta[b, :len(obs[b]["gt_path"])] = [idx[s][x] for x in obs[b]["gt_path"]]
            tra[b, :len(flat[b])] = [idx[s][x] for x in flat[b]]
        out[pre + "cand"], out[pre + "visited"], out[pre + "gt"], out[pre + "traj"] = cand, vm, gta, tra
        out[pre + "gt_len"] = np.array([len(o["gt_path"]) for o in obs], dtype=np.int32)
        out[pre + "traj_len"] = np.array([len(f) for f in flat], dtype=np.int32)
        out[pre + "ended"] = np.array(ended, dtype=np.uint8)
        out[pre + "target"] = np.asarray(tgt, dtype=np.int64)
    out["n_expert_cases"] = np.array(len(cases))

    # ---------------- metrics: _eval_item + eval_metrics on random trajectories
    env = object.__new__(ref_env.R2RNavBatch)
    env.shortest_distances = sd
    env.gt_trajs = {}
    preds, scans_b, gts = [], [], []
    B = 40
    for b in range(B):
        s = SCANS[b % 3]
        G = graphs[s]
        start = ids[s][rng.integers(len(ids[s]))]
        gt = _gt_path(rng, G, sp[s], start, 3, 40 if b % 4 == 0 else 10)
        segs = [[start]]
        cur = start
        for _ in range(int(rng.integers(0, 10))):
            if rng.random() < 0.3:
                w = ids[s][rng.integers(len(ids[s]))]
                seg = sp[s][cur][w][1:]
                if seg:
                    segs.append(seg)
                    cur = w
            else:
                w = _random_walk(rng, G, cur, 1)[-1]
                segs.append([w])
                cur = w
        if b % 5 == 0:            # finish near / at the goal
            seg = sp[s][cur][gt[-1]][1:]
            if seg:
                segs.append(seg)
        env.gt_trajs[f"i{b}"] = (s, gt)
        preds.append({"instr_id": f"i{b}", "trajectory": segs})
        scans_b.append(s)
        gts.append(gt)
    avg, per = env.eval_metrics(preds)
    flat = [sum(p["trajectory"], []) for p in preds]
    Lp, Lg = max(map(len, flat)), max(map(len, gts))
    pa = np.full((B, Lp), -1, dtype=np.int32)
    ga = np.full((B, Lg), -1, dtype=np.int32)
    for b in range(B):
        s = scans_b[b]
        pa[b, :len(flat[b])] = [idx[s][x] for x in flat[b]]
        ga[b, :len(gts[b])] = [idx[s][x] for x in gts[b]]
    out["met_scan"] = np.array([SCANS.index(s) for s in scans_b], dtype=np.int32)
    out["met_path"], out["met_gt"] = pa, ga
    out["met_path_len"] = np.array(list(map(len, flat)), dtype=np.int32)
    out["met_gt_len"] = np.array(list(map(len, gts)), dtype=np.int32)
    out["met_action_steps"] = np.array([len(p["trajectory"]) - 1 for p in preds], dtype=np.int32)
    for k in ("nav_error", "oracle_error", "action_steps", "trajectory_steps", "trajectory_lengths", "success", "spl",
              "oracle_success", "DTW", "nDTW", "SDTW", "CLS"):
        out[f"met_item_{k}"] = np.array(per[k], dtype=np.float64)
    for k, v in avg.items():
        out[f"met_avg_{k}"] = np.array(v, dtype=np.float64)
    # cal_cls on its own (threshold 3.0)
    out["met_calcls"] = np.array([cal_cls(sd[s], f, g) for s, f, g in zip(scans_b, flat, gts)], dtype=np.float64)

    # long reference paths (65..100 nodes, RxR-like): the DTW crosses 64-lane blocks; cal_dtw + _eval_item per item
    s = SCANS[2]
    lp, lg, ld = [], [], []
    for b in range(8):
        start = ids[s][rng.integers(len(ids[s]))]
        gt = _gt_path(rng, graphs[s], sp[s], start, 65, 100)
        walk = _random_walk(rng, graphs[s], start, int(rng.integers(10, 60)))
        segs = [[walk[0]]] + [[x] for x in walk[1:]]
        lp.append([idx[s][x] for x in sum(segs, [])])
        lg.append([idx[s][x] for x in gt])
        ld.append([env._eval_item(s, segs, gt)[k] for k in ("DTW", "nDTW", "CLS")])
    out["long_path"] = np.array([r + [-1] * (max(map(len, lp)) - len(r)) for r in lp], dtype=np.int32)
    out["long_gt"] = np.array([r + [-1] * (max(map(len, lg)) - len(r)) for r in lg], dtype=np.int32)
    out["long_path_len"] = np.array(list(map(len, lp)), dtype=np.int32)
    out["long_gt_len"] = np.array(list(map(len, lg)), dtype=np.int32)
    out["long_DTW_nDTW_CLS"] = np.array(ld, dtype=np.float64)

    np.savez_compressed(os.path.join(HERE, "nav_expert.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "nav_scans.npz"), **scans_npz)
    for f in ("nav_expert.npz", "nav_scans.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
