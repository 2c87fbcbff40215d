"""ms per navigation step of the fine-tune supervision: device (csrc/nav_expert.hip: expert targets + action step + IL
loss) against the reference's Python expert (agent.py:371-417 restated over dict-of-dict tables, as env.py builds them).

Synthetic scan: a jittered grid graph (no connectivity files needed).  One JSON line per (policy, size).
  python scripts/bench_nav_expert.py [--batch 32] [--iters 50]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vln_bevbert_amd import nav_expert as NE  # noqa: E402


def grid_graphs(side=13, seed=0):
    rng = np.random.default_rng(seed)
    n = side * side
    pos = [(x + rng.uniform(-.2, .2), y + rng.uniform(-.2, .2), rng.uniform(0, .1)) for y in range(side) for x in range(side)]
    edges = [(i, i + 1) for i in range(n) if (i + 1) % side] + [(i, i + side) for i in range(n - side)]
    edges += [(i, i + side + 1) for i in range(n - side) if (i + 1) % side and rng.random() < .3]
    return NE.ScanGraphs.from_edges({"grid": ([f"v{i}" for i in range(n)], pos, edges)})


def states(g, B, C, gt_lo, gt_hi, traj_hi, seed):
    rng = np.random.default_rng(seed)
    n = len(g.ids[0])
    gts, trajs, curs, cands = [], [], [], []
    for _ in range(B):
        gt = [int(rng.integers(n))]
        want = int(rng.integers(gt_lo, gt_hi + 1))
        while len(gt) < want:
            gt += g.path(0, gt[-1], int(rng.integers(n)))[1:]
        gt = gt[:want]
        tr = [gt[0]]
        for _ in range(int(rng.integers(1, traj_hi + 1))):
            nb = [v for v, _ in g.adjacency[0][tr[-1]]]
            tr.append(nb[rng.integers(len(nb))])
        gts.append(gt)
        trajs.append(tr)
        curs.append(tr[-1])
        cands.append([-1] + list(rng.choice(n, C - 1, replace=False)))
    return gts, trajs, curs, cands


def host_expert(sd, sp, gts, trajs, curs, cands, policy):
    """_teacher_action_r4r (not imitation) with the reference's dict tables and cal_dtw."""
    out = []
    for gt, tr, cur, cand in zip(gts, trajs, curs, cands):
        if cur == gt[-1]:
            out.append(0)
            continue
        best, a = math.inf, -100
        for j, vp in enumerate(cand):
            if j == 0:
                continue
            if policy == "spl":
                d = sd[vp][gt[-1]] + sd[cur][vp]
            else:
                pred = tr + sp[cur][vp][1:]
                m = np.inf * np.ones((len(pred) + 1, len(gt) + 1))
                m[0][0] = 0
                for i in range(1, len(pred) + 1):
                    for k in range(1, len(gt) + 1):
                        m[i][k] = sd[pred[i - 1]][gt[k - 1]] + min(m[i - 1][k], m[i][k - 1], m[i - 1][k - 1])
                d = -np.exp(-m[len(pred)][len(gt)] / (3.0 * len(gt)))
            if d < best:
                best, a = d, j
        out.append(a)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cands", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = grid_graphs()
    n = len(g.ids[0])
    sd = {u: {v: float(g.dist[0, u, v]) for v in range(n)} for u in range(n)}
    sp = {u: {v: g.path(0, u, v) for v in range(n)} for u in range(n)}
    B, C = args.batch, args.cands
    for policy, (lo, hi, th) in (("spl", (4, 8, 14)), ("ndtw", (20, 40, 19))):
        gts, trajs, curs, cands = states(g, B, C, lo, hi, th, 1)
        Lg, Lt = max(map(len, gts)), max(map(len, trajs))
        pad = lambda rows, L: torch.tensor([r + [-1] * (L - len(r)) for r in rows], dtype=torch.int32, device=dev)
        t = dict(scan=torch.zeros(B, dtype=torch.int32, device=dev), cur=torch.tensor(curs, dtype=torch.int32, device=dev),
                 cand=pad(cands, C), visited=None, ended=torch.zeros(B, dtype=torch.uint8, device=dev),
                 gt=pad(gts, Lg), gt_len=torch.tensor(list(map(len, gts)), dtype=torch.int32, device=dev), t=0,
                 policy=policy, traj=pad(trajs, Lt), traj_len=torch.tensor(list(map(len, trajs)), dtype=torch.int32,
                                                                           device=dev))
        logits = torch.randn(B, C, device=dev)
        st = dict(ended=torch.zeros(B, dtype=torch.uint8, device=dev),
                  stop_scores=torch.zeros(B, n, dtype=torch.float32, device=dev),
                  stop_order=torch.zeros(B, n, dtype=torch.int32, device=dev),
                  n_stop=torch.zeros(B, dtype=torch.int32, device=dev))
        goal = torch.tensor([gt[-1] for gt in gts], dtype=torch.int32, device=dev)

        def device_step():
            tg = NE.expert_targets(g, t["scan"], t["cur"], t["cand"], t["visited"], t["ended"], t["gt"], t["gt_len"],
                                   0, policy, t["traj"], t["traj_len"])
            NE.il_loss(logits, tg)
            st["ended"].zero_()
            st["n_stop"].zero_()
            return NE.action_step(logits, "sample", 0, 20, cand=t["cand"], cur=t["cur"], goal=goal, **st), tg

        for _ in range(3):
            _, tg = device_step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            o, tg = device_step()
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / args.iters
        want = host_expert(sd, sp, gts, trajs, curs, [[None] + c[1:] for c in cands], policy)
        h_iters = max(1, args.iters // (10 if policy == "ndtw" else 1))
        t0 = time.perf_counter()
        for _ in range(h_iters):
            host_expert(sd, sp, gts, trajs, curs, [[None] + c[1:] for c in cands], policy)
        host_ms = (time.perf_counter() - t0) * 1e3 / h_iters
        print(json.dumps({"policy": policy, "batch": B, "cands": C, "gt_len": [lo, hi], "traj_max": Lt,
                          "device_ms_per_step": round(dev_ms, 4), "host_expert_ms_per_step": round(host_ms, 3),
                          "targets_equal": tg.cpu().tolist() == want}), flush=True)


if __name__ == "__main__":
    main()
