"""ms per call of the CE waypoint stage (vln_bevbert_amd.waypoint.waypoint_step), eager and replayed from a hipGraph,
next to a plain-torch restatement of the reference's mode-'waypoint' tail (per-sample nonzero / .cpu() / .tolist(), host
synchronisations included) on the same GPU in the same process.  Both sides run the same predictor network, so the
difference is the tail.  Prints one JSON line.

    python scripts/bench_waypoint.py [--batch 16] [--iters 50] [--dtype bf16|fp32] [--train]
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
from vln_bevbert_amd import waypoint as W  # noqa: E402
from vln_bevbert_amd import weights  # noqa: E402


def _nms(pred, max_predictions=5, sigma=(7.0, 5.0)):
    """Plain-torch arg-max + box suppression over (B, 1, H, W) the way the reference's helper executes."""
    shape = pred.shape
    out = torch.zeros_like(pred)
    flat_pred, supp = pred.reshape(shape[0], -1), pred.clone()
    flat_out = out.reshape(shape[0], -1)
    rows = torch.arange(shape[0])
    xs = torch.arange(shape[-1], device=pred.device, dtype=torch.float32)[None, None, :]
    ys = torch.arange(shape[-2], device=pred.device, dtype=torch.float32)[None, :, None]
    for _ in range(max_predictions):
        _, ix = torch.max(supp.reshape(shape[0], -1), dim=1)
        flat_out[rows, ix] = flat_pred[rows, ix]
        mu = torch.stack([ix % shape[-1], ix / shape[-1]], 1).float()
        xd = xs - mu[:, 0, None, None]
        xd = torch.min(xd.abs(), (xd + shape[-1]).abs())
        g = torch.logical_and(xd <= sigma[0], (ys - mu[:, 1, None, None]).abs() <= sigma[1]).float()
        supp *= 1 - g.unsqueeze(1)
    return out


def torch_tail(logits, rgb_embeds, depth_embeds, pano_fts, in_train):
    """The reference's tail behind the predictor, restated in plain torch with its host round trips."""
    B = logits.shape[0]
    rgb = rgb_embeds.reshape(B, 12, 512)
    rgb = torch.cat([rgb[:, :1], torch.flip(rgb[:, 1:], [1])], 1)
    dep = depth_embeds.reshape(B, 12, 128, 4, 4)
    dep = torch.cat([dep[:, :1], torch.flip(dep[:, 1:], [1])], 1).mean((-1, -2))
    x = torch.softmax(logits.reshape(B, -1), 1).reshape(B, 120, 12)
    omap = _nms(torch.cat([x[:, -1:], x, x[:, :1]], 1).unsqueeze(1)).squeeze(1)[:, 1:-1]
    if in_train:
        regional = torch.cat([logits[:, -5:], logits[:, :-5]], 1).reshape(B, 12, 10, 12)
    out = []
    for j in range(B):
        nz = omap[j].nonzero()
        a, d = nz[:, 0], nz[:, 1]
        if in_train:
            img = (a.cpu().numpy() + 5) // 10
            img[img == 12] = 0
            act = torch.distributions.Categorical(torch.softmax(regional[j][img].view(img.size, -1), 1)).sample()
            ptr = [(i - 1) * 10 + 5 if i != 0 else 0 for i in img]
            a = torch.tensor([int(w) // 12 + p for w, p in zip(act, ptr)])
            d = torch.tensor([int(w) % 12 for w in act])
        rad_c = a.cpu().float() / 120 * 2 * math.pi
        fts = torch.stack([rad_c.sin(), rad_c.cos(), torch.zeros_like(rad_c), torch.ones_like(rad_c)], 1)
        angles = (2 * math.pi - a.float() / 120 * 2 * math.pi).tolist()
        dists = ((d + 1) * 0.25).tolist()
        img = 12 - (a.cpu().numpy() + 5) // 10
        img[img == 12] = 0
        mask = np.zeros(12, dtype=bool)
        mask[img] = True
        out.append((torch.cat([rgb[j, img], rgb[j][~mask]]), torch.cat([dep[j, img], dep[j][~mask]]),
                    torch.cat([fts, pano_fts[~mask]]), [1] * len(angles) + [0] * int(12 - mask.sum()), angles, dists))
    L = max(len(o[3]) for o in out)

    def pad(ts):
        r = torch.zeros(B, L, ts[0].shape[1], dtype=ts[0].dtype, device=ts[0].device)
        for i, t in enumerate(ts):
            r[i, :t.shape[0]] = t
        return r
    return (pad([o[0] for o in out]), pad([o[1] for o in out]), pad([o[2] for o in out]).to(logits.device),
            torch.nn.utils.rnn.pad_sequence([torch.LongTensor(o[3]) for o in out], batch_first=True).to(logits.device),
            torch.LongTensor([len(o[3]) for o in out]).to(logits.device))


def _time(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--train", action="store_true", help="with the waypoint_aug draw")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    m = W.WaypointPredictor()
    m.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    m.finalize(dev, dt)
    g = torch.Generator().manual_seed(0)
    B = a.batch
    rgb = torch.randn(B * 12, 512, generator=g).to(dev, dt)
    dep = torch.randn(B * 12, 128, 4, 4, generator=g).abs().to(dev, dt)
    pano_fts = W.pano_angle_fts("cpu")

    def stage():
        return W.waypoint_step(m, rgb, dep, in_train=a.train, seed=1, t=0)

    def baseline():
        return torch_tail(m(None, dep), rgb.float(), dep.float(), pano_fts, a.train)

    def network():
        return m.classifier_output(dep)
    eager = _time(stage, a.iters)
    net = _time(network, a.iters)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage()
    replay = _time(graph.replay, a.iters)
    base = _time(baseline, max(5, a.iters // 5))
    print(json.dumps({"bench": "waypoint_step", "batch": B, "dtype": a.dtype, "in_train": a.train,
                      "eager_ms": round(eager, 4), "graph_replay_ms": round(replay, 4),
                      "predictor_only_eager_ms": round(net, 4), "torch_restatement_ms": round(base, 4),
                      "speedup_replay_vs_restatement": round(base / replay, 2)}))


if __name__ == "__main__":
    main()
