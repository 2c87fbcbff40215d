"""Time the CE agent's map stage: update + remember_pano + nav_gmap_variable + bev_inputs (lift and splat of the
current panorama included) + record_stop_scores + act per step, eager and
replayed from one hipGraph (single stream, no parallel branches), against the numpy restatement of the reference's
per-environment Python (tests/ce_map_ref.py; the reference itself adds two networkx Dijkstra runs per map and step).

    python scripts/bench_ce_map.py [--batch 16] [--steps 15] [--episodes 20] [--out FILE]     (default profiles/ce_map_bench.txt)

Episodes are random walks: every step has 3-5 candidates 1-3 m away, the agent takes the first ghost of the listing.
The figure to hold this stage against is the navigation forward it precedes (about 3.1 ms at this batch size)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ce_map_ref as R                      # noqa: E402
from vln_bevbert_amd.ce_map import CEGraphMap           # noqa: E402

H, L, C = 768, 17, 5
GRID = {}            # one panorama's grid features / depths, reused by every step (their values do not steer the walk)


def episode(rng, B, T):
    pos = rng.uniform(-20, 20, (B, 3)) * np.array([1, 0.05, 1])
    steps = []
    for t in range(T):
        k = rng.integers(3, C + 1, B).astype(np.int32)
        nav = (np.arange(L)[None] < k[:, None]).astype(np.int64)
        steps.append({"cur_pos": pos.copy(), "heading": rng.uniform(0, 2 * np.pi, B), "cand_count": k,
                      "cand_angles": rng.uniform(0, 2 * np.pi, (B, C)).astype(np.float32),
                      "cand_distances": (rng.integers(4, 13, (B, C)) / 4).astype(np.float32), "nav_types": nav,
                      "avg_pano": rng.standard_normal((B, H)).astype(np.float32),
                      "pano": rng.standard_normal((B, L, H)).astype(np.float32),
                      "probs0": rng.uniform(0, 1, B).astype(np.float32)})
        pos = pos + rng.uniform(-2.5, 2.5, (B, 3)) * np.array([1, 0.02, 1])
    return steps


def first_ghost(masks, visited):
    free = masks[:, 1:] & ~visited[:, 1:]
    return torch.where(free.any(1), free.long().argmax(1) + 1, torch.zeros_like(free[:, 0], dtype=torch.int64))


def device_step(m, d):
    m.update(0, d["cand_count"], d["cand_angles"], d["cand_distances"], d["avg_pano"], d["pano"], d["nav_types"])
    m.remember_pano(GRID["rgb"], GRID["depth"])
    nav = m.nav_gmap_variable()
    bev = m.bev_inputs()
    m.record_stop_scores(d["probs0"])
    return nav, bev, m.act(first_ghost(nav["gmap_masks"], nav["gmap_visited_masks"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_map_bench.txt"))
    a = ap.parse_args()
    B, T = a.batch, a.steps
    rng = np.random.default_rng(0)
    eps = [episode(rng, B, T) for _ in range(a.episodes)]
    dev = torch.device("cuda")
    keys = ("cand_count", "cand_angles", "cand_distances", "nav_types", "avg_pano", "pano", "probs0")
    gen = torch.Generator().manual_seed(0)
    GRID["rgb"] = torch.randn(B, 12, 196, H, generator=gen).to(dev)
    GRID["depth"] = (torch.rand(B, 12, 14, 14, generator=gen) * 0.5).to(dev)
    on_dev = [[{k: torch.from_numpy(s[k]).to(dev) for k in keys} for s in ep] for ep in eps]
    lines = [f"CE map stage, batch {B}, {T} steps per episode, {a.episodes} episodes, H = {H}, "
             f"{torch.cuda.get_device_name(0)}"]

    # ---- eager
    m = CEGraphMap(B, H, dev)
    def run_eager(n_eps):
        for ep, dep in zip(eps[:n_eps], on_dev):
            m.reset()
            for t, (s, d) in enumerate(zip(ep, dep)):
                m.stage(t + 1, s["cur_pos"], s["heading"])
                out = device_step(m, d)
        return out
    run_eager(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_eager(a.episodes)
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) * 1e3 / (a.episodes * T)
    assert m.check_overflow() == 0
    ghosts = float(m.t["g_alive"].sum()) / B

    # ---- one captured step
    mg = CEGraphMap(B, H, dev)
    static = {k: v.clone() for k, v in on_dev[0][0].items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mg.stage(1, eps[0][0]["cur_pos"], eps[0][0]["heading"])
        device_step(mg, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mg.stage(1, eps[0][0]["cur_pos"], eps[0][0]["heading"])
        cap = device_step(mg, static)
    def run_graph(n_eps):
        for ep, dep in zip(eps[:n_eps], on_dev):
            mg.reset()
            for t, (s, d) in enumerate(zip(ep, dep)):
                for k in keys:
                    static[k].copy_(d[k])
                mg.stage(t + 1, s["cur_pos"], s["heading"], copy=False)
                g.replay()
                mg.mark_replayed()
    run_graph(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_graph(a.episodes)
    torch.cuda.synchronize()
    graph_ms = (time.perf_counter() - t0) * 1e3 / (a.episodes * T)
    same = all(torch.equal(m.t[k], mg.t[k]) for k in m.t)
    assert mg.check_overflow() == 0
    # the device time of the replays alone, over the same walks (events around each replay; staging is outside them)
    pairs = []
    for ep, dep in zip(eps[:4], on_dev):
        mg.reset()
        for t, (s, d) in enumerate(zip(ep, dep)):
            for k in keys:
                static[k].copy_(d[k])
            mg.stage(t + 1, s["cur_pos"], s["heading"], copy=False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            mg.mark_replayed()
            pairs.append((e0, e1))
    torch.cuda.synchronize()
    replay_ms = sum(a_.elapsed_time(b_) for a_, b_ in pairs) / len(pairs)
    assert mg.check_overflow() == 0

    # ---- the numpy restatement of the reference's per-environment Python
    n_cpu = min(3, a.episodes)
    t0 = time.perf_counter()
    for ep in eps[:n_cpu]:
        r = R.CEMapRef(B, H)
        for t, s in enumerate(ep):
            r.update(t + 1, s["cur_pos"], s["heading"], np.ones(B, bool), s["cand_count"], s["cand_angles"], s["cand_distances"],
                     s["avg_pano"], s["pano"], s["nav_types"])
            nav = r.nav_gmap_variable()
            r.bev_inputs()
            r.record_stop_scores(s["probs0"])
            free = nav["gmap_masks"][:, 1:] & ~nav["gmap_visited_masks"][:, 1:]
            r.act(np.where(free.any(1), free.argmax(1) + 1, 0), False)
    cpu_ms = (time.perf_counter() - t0) * 1e3 / (n_cpu * T)
    lines += [f"  eager, host-timed (launch-bound)          {eager_ms:8.3f} ms / step",
              f"  one hipGraph, inputs staged + replay      {graph_ms:8.3f} ms / step",
              f"  one hipGraph, device time of the replay   {replay_ms:8.3f} ms / step",
              f"  numpy restatement on the host (no lift)   {cpu_ms:8.3f} ms / step",
              f"  state after the last episode: eager == graph: {same}; live ghosts per map {ghosts:.1f}",
              "  for comparison: the navigation forward this stage precedes takes about 3.1 ms"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
