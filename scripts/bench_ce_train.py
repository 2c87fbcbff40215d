"""Time the gradient path through the CE agent's map: one rollout of 15 steps forward (update + listing + action, with
the tape's record) and the backward of sum_t (w_t * gmap_img_fts[t]) into every step's avg_pano_embeds / pano_embeds.

    python scripts/bench_ce_train.py [--batch 16] [--steps 15] [--rounds 12] [--out FILE]    (default profiles/ce_train_bench.txt)

Two variants, run in turns in one process over the same random walks (scripts/bench_ce_map.py's):
  tape   ce_train.CEMapTape: one record launch per step, one adjoint launch per consumer step in backward;
  dicts  a plain-torch restatement that keeps the map's embeddings as live tensors in Python dicts, as the reference's
         GraphMap does (ss_trainer_BEV.py:1060-1066, :552-556): the device map still does the geometry, cand_slot and
         gmap_ids are read back every step, gmap_img_fts is stacked row by row and autograd does the rest.
Both give the same gradients (compared after the timing, max-abs difference printed).  Figures are host-timed medians
between synchronisations; the model's own forward and backward are not part of either."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vln_bevbert_amd.ce_map import CEGraphMap           # noqa: E402
from vln_bevbert_amd.ce_train import CEMapTape          # noqa: E402

H, L, C = 768, 17, 5


def episode(rng, B, T):
    pos = rng.uniform(-20, 20, (B, 3)) * np.array([1, 0.05, 1])
    steps = []
    for t in range(T):
        k = rng.integers(3, C + 1, B).astype(np.int32)
        steps.append({"cur_pos": pos.copy(), "heading": rng.uniform(0, 2 * np.pi, B), "cand_count": k,
                      "cand_angles": rng.uniform(0, 2 * np.pi, (B, C)).astype(np.float32),
                      "cand_distances": (rng.integers(4, 13, (B, C)) / 4).astype(np.float32),
                      "nav_types": (np.arange(L)[None] < k[:, None]).astype(np.int64),
                      "avg": rng.standard_normal((B, H)).astype(np.float32),
                      "pano": rng.standard_normal((B, L, H)).astype(np.float32)})
        pos = pos + rng.uniform(-2.5, 2.5, (B, 3)) * np.array([1, 0.02, 1])
    return steps


def first_ghost(masks, visited):
    free = masks[:, 1:] & ~visited[:, 1:]
    return torch.where(free.any(1), free.long().argmax(1) + 1, torch.zeros_like(free[:, 0], dtype=torch.int64))


class DictMap:
    """Live tensors in Python dicts around the device map (the embeddings the map itself holds are not used)."""

    def __init__(self, m):
        self.map = m
        self.counts = [torch.tensor(float(c), device=m.device) for c in range(m.P + 1)]

    def begin_episode(self):
        self.map.reset()
        self.nodes, self.ghosts = [{} for _ in range(self.map.B)], [{} for _ in range(self.map.B)]

    def update(self, step_id, count, ang, dis, avg, pano, nav_types, cur_pos, heading):
        m = self.map
        slot = m.update(step_id, count, ang, dis, avg, pano, nav_types, cur_pos=cur_pos, heading=heading)
        cur, sl = m.t["cur_vp"].tolist(), slot.tolist()
        for b in range(m.B):
            self.nodes[b][cur[b]] = avg[b]
            g = self.ghosts[b]
            for j, e in enumerate(sl[b]):                       # nav_types puts candidate j at row j in these walks
                if e >= m.N:
                    g[e] = [pano[b, j], 1] if e not in g else [g[e][0] + pano[b, j], g[e][1] + 1]
        return slot

    def nav_gmap_variable(self):
        m = self.map
        o = m.nav_gmap_variable()
        zero = o["gmap_img_fts"].new_zeros(m.H)
        rows = [zero if e < 0 else (self.nodes[b][e] if e < m.N else self.ghosts[b][e][0] / self.counts[self.ghosts[b][e][1]])
                for b, ids in enumerate(o["gmap_ids"].tolist()) for e in ids]
        o["gmap_img_fts"] = torch.stack(rows).view(m.B, m.G, m.H)
        return o


def rollout(mapper, ep, dev_ep, w):
    """Forward of one episode; returns (the leaves, the loss)."""
    mapper.begin_episode()
    m = mapper.map
    leaves, loss = [], None
    for t, (s, d) in enumerate(zip(ep, dev_ep)):
        avg, pano = d["avg"].clone().requires_grad_(True), d["pano"].clone().requires_grad_(True)
        mapper.update(t + 1, d["cand_count"], d["cand_angles"], d["cand_distances"], avg, pano, d["nav_types"],
                      cur_pos=s["cur_pos"], heading=s["heading"])
        nav = mapper.nav_gmap_variable()
        m.act(first_ghost(nav["gmap_masks"], nav["gmap_visited_masks"]), gmap_ids=nav["gmap_ids"])
        term = (nav["gmap_img_fts"] * w[t]).sum()
        loss = term if loss is None else loss + term
        leaves.append((avg, pano))
    return leaves, loss


def timed(mapper, ep, dev_ep, w):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    leaves, loss = rollout(mapper, ep, dev_ep, w)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    loss.backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_train_bench.txt"))
    a = ap.parse_args()
    B, T = a.batch, a.steps
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    eps = [episode(rng, B, T) for _ in range(4)]
    keys = ("cand_count", "cand_angles", "cand_distances", "nav_types", "avg", "pano")
    dev_eps = [[{k: torch.from_numpy(s[k]).to(dev) for k in keys} for s in ep] for ep in eps]
    gen = torch.Generator().manual_seed(1)
    variants = {"tape": CEMapTape(CEGraphMap(B, H, dev), T, C, L), "dicts": DictMap(CEGraphMap(B, H, dev))}
    w = torch.randn(T, B, variants["tape"].map.G, H, generator=gen).to(dev)
    times = {k: {"fwd": [], "bwd": []} for k in variants}
    grads = {}
    for r in range(2 + a.rounds):                                  # two warm-up rounds, then the variants in turns
        i = r % len(eps)
        for name, mapper in variants.items():
            f, b, leaves = timed(mapper, eps[i], dev_eps[i], w)
            if r >= 2:
                times[name]["fwd"].append(f)
                times[name]["bwd"].append(b)
            grads[name] = leaves
    diff = max(float((x.grad - y.grad).abs().max()) for p, q in zip(grads["tape"], grads["dicts"]) for x, y in zip(p, q))
    scale = max(float(x.grad.abs().max()) for p in grads["dicts"] for x in p)
    assert all(v.map.check_overflow() == 0 for v in variants.values())
    med = {k: {h: statistics.median(v) for h, v in t.items()} for k, t in times.items()}
    lines = [f"gradient path through the CE map, batch {B}, {T} steps per rollout, H = {H}, {a.rounds} rounds in turns "
             f"(medians, host-timed between synchronisations), {torch.cuda.get_device_name(0)}",
             "                                                    forward      backward   ms / rollout"]
    for k, label in (("tape", "CEMapTape (record + one adjoint launch per step)"), ("dicts", "live tensors in Python dicts (torch autograd)  ")):
        lines.append(f"  {label}  {med[k]['fwd']:9.3f}  {med[k]['bwd']:12.3f}")
    lines += [f"  backward: min / max over the rounds  tape {min(times['tape']['bwd']):.3f} / {max(times['tape']['bwd']):.3f}   "
              f"dicts {min(times['dicts']['bwd']):.3f} / {max(times['dicts']['bwd']):.3f}",
              f"  gradients of the two variants: max |difference| {diff:.3e} at max |gradient| {scale:.3e}",
              "  the forward columns include the device map's own work (update, listing, action), equal in both; the dicts"
              " variant adds two read-backs per step and one stack of B x G rows"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
