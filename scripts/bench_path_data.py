"""Cost of feeding R2R pre-training from tables (vln_bevbert_amd/path_data.py, csrc/path_data.hip).

  python scripts/bench_path_data.py --host            CPU only: ms per batch of PathBatchSource (table lookup + the
                                                       three draws + collate) and of StaticBatch.plan (``_host_side``)
  python scripts/bench_path_data.py --gpu             MI355X: the bevbert_pd_pano_rows launch alone (bytes over time),
                                                       then sustained samples/s through StreamingLoader against the same
                                                       trainer replaying resident batches, in alternating blocks

The world is fabricated at R2R scale from the three fixture scans of tests/golden/nav_scans.npz: ``--replicas`` copies of
them (44 -> 10 472 viewpoints) and ``--items`` items with paths of 4..7 nodes, candidates = graph neighbours.  Prefix
tables are built for one replica and tiled (replicas share geometry; rows and scan indices are offset).  Nothing of the
reference is read.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vln_bevbert_amd import path_data as pd  # noqa: E402
from vln_bevbert_amd.nav_expert import ScanGraphs  # noqa: E402


def world(replicas, n_items, seed=0, max_txt_len=80):
    """(data, tables) at scale.  Candidates: every graph neighbour, distinct view indices (36-token panoramas)."""
    rng = np.random.default_rng(seed)
    raw = np.load(os.path.join(ROOT, "tests", "golden", "nav_scans.npz"))
    base = sorted({k.split("/")[0] for k in raw.files})
    edges = {}
    for s in base:
        ids, inc, un, pose = (raw[f"{s}/{k}"] for k in ("ids", "included", "unobstructed", "pose"))
        e = [(i, j) for i in range(len(ids)) if inc[i] for j in range(len(ids)) if un[i, j] and inc[j]]
        edges[s] = ([str(x) for x in ids], pose[:, [3, 7, 11]], e)
    g0 = ScanGraphs.from_edges(edges)
    cands0 = {}
    for si, s in enumerate(base):
        for u, vp in enumerate(g0.ids[si]):
            nb = [g0.ids[si][v] for v, _ in g0.adjacency[si][u]]
            views = rng.choice(36, size=len(nb), replace=len(nb) > 36)
            cands0[f"{s}_{vp}"] = {n: [int(v), 1.0, float(rng.uniform(-.25, .25)), float(rng.uniform(-.25, .25))]
                                   for n, v in zip(nb, views)}
    per = -(-n_items // replicas)
    items0 = []
    while len(items0) < per:
        si = int(rng.integers(len(base)))
        n = len(g0.ids[si])
        p = g0.path(si, int(rng.integers(n)), int(rng.integers(n)))
        if not 4 <= len(p) <= 7:
            continue
        L = int(rng.integers(20, 120))
        items0.append({"instr_id": f"{len(items0)}_0", "scan": base[si], "path": [g0.ids[si][v] for v in p],
                       "heading": float(rng.uniform(0, 2 * np.pi)),
                       "instr_encoding": [101] + [int(x) for x in rng.integers(1996, 29000, size=L - 2)] + [102]})
    d0 = pd.R2RPathData(items0, g0, cands0, 768, max_txt_len=max_txt_len)
    t0 = time.perf_counter()
    tab0 = pd.PrefixTables(d0)
    build_s = time.perf_counter() - t0
    # ---- replicate: scans '<scan>@r', the same viewpoint ids, rows / scan indices offset
    ren = lambda s, r: f"{s}@{r}"
    graphs = ScanGraphs.__new__(ScanGraphs)
    graphs.__dict__.update(g0.__dict__)
    graphs.scans = [ren(s, r) for r in range(replicas) for s in base]
    graphs.scan_index = {s: i for i, s in enumerate(graphs.scans)}
    graphs.ids, graphs.positions, graphs.adjacency = g0.ids * replicas, g0.positions * replicas, g0.adjacency * replicas
    graphs.index = {(s, vp): j for s, l in zip(graphs.scans, graphs.ids) for j, vp in enumerate(l)}
    graphs.dist, graphs.pred = np.tile(g0.dist, (replicas, 1, 1)), np.tile(g0.pred, (replicas, 1, 1))
    graphs._hops, graphs._dev = np.tile(g0.hops, (replicas, 1, 1)), {}
    cands = {f"{ren(k.split('_', 1)[0], r)}_{k.split('_', 1)[1]}": v for r in range(replicas) for k, v in cands0.items()}
    items = [dict(it, scan=ren(it["scan"], r), instr_id=f"{r}x{it['instr_id']}") for r in range(replicas) for it in items0]
    data = pd.R2RPathData(items[:n_items], graphs, cands, 768, max_txt_len=max_txt_len)
    tab = pd.PrefixTables()
    P, Nk = len(tab0), len(tab0.pano.keys)
    for k in pd.PrefixTables.ARRAYS:
        a = getattr(tab0, k)
        if k in ("item_start", "pano_ptr", "gmap_ptr", "cand_ptr"):
            a = np.concatenate([a[:1]] + [a[1:] + r * a[-1] for r in range(replicas)])
        else:
            off = {"pano_rows": Nk, "scan": len(base)}.get(k, 0)
            a = np.concatenate([a + np.asarray(r * off, dtype=a.dtype) if off else a for r in range(replicas)])
        setattr(tab, k, a)
    t = tab0.pano
    tab.pano = pd.PanoTable(list(cands), np.tile(t.view_order, (replicas, 1)), np.tile(t.n_tokens, replicas),
                            np.tile(t.loc_fts, (replicas, 1, 1)), np.tile(t.nav_types, (replicas, 1)),
                            np.tile(t.cand_ids, (replicas, 1)))
    assert len(tab) == P * replicas and tab.pano.keys[Nk] == list(cands)[Nk]
    return data, tab, {"viewpoints": len(cands), "items": len(data), "prefixes": int(tab.item_start[len(data)]),
                       "tables_build_s_per_1k_prefixes": round(1000 * build_s / P, 2)}


def host(a):
    from vln_bevbert_amd.config import BevBertConfig
    from vln_bevbert_amd.static_step import StaticBatch
    data, tab, info = world(a.replicas, a.items)
    cfg = BevBertConfig(image_feat_size=768)
    src = pd.PathBatchSource(data, tab, ["mlm", "sap", "masksem"], a.batch, seed=1, end_vp_pos_ratio=0.2)
    it = iter(src)
    for _ in range(3):
        next(it)
    t_src = t_plan = 0.0
    sigs = set()
    for _ in range(a.steps):
        t0 = time.perf_counter()
        task, b, keys, rows = next(it)
        t1 = time.perf_counter()
        h = StaticBatch.plan(cfg, task, dict(b, pano_rows=rows))
        t2 = time.perf_counter()
        t_src, t_plan = t_src + t1 - t0, t_plan + t2 - t1
        sigs.add(h["signature"])
    print(json.dumps(dict(info, what="host cost per batch, one process (CPU)", batch=a.batch, batches=a.steps,
                          source_ms_per_batch=round(1e3 * t_src / a.steps, 2), host_side_ms_per_batch=round(1e3 * t_plan / a.steps, 2),
                          per_sample_ms=round(1e3 * (t_src + t_plan) / a.steps / a.batch, 3), shape_buckets_seen=len(sigs))))


def gpu(a):
    from vln_bevbert_amd import weights
    from vln_bevbert_amd.config import BevBertConfig
    from vln_bevbert_amd.feature_store import GridFeatureStore, ViewFeatureStore, pano_rows
    from vln_bevbert_amd.loader import BucketManager, StreamingLoader, quiet_gc
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    from vln_bevbert_amd.train import PretrainTrainer
    assert torch.cuda.is_available(), "--gpu needs the MI355X"
    dev = torch.device("cuda:0")
    data, tab, info = world(a.replicas, a.items)
    N = len(tab.pano.keys)
    g = torch.Generator(device=dev).manual_seed(3)
    store = ViewFeatureStore(tab.pano.keys, torch.randn(N, 36, 768, generator=g, device=dev).half(), dev)
    # ---- 1. the launch alone: a batch of 64 samples' panoramas
    src = pd.PathBatchSource(data, tab, ["sap"], a.batch, seed=2)
    _, b, _, rows = next(iter(src))
    Tp = -(-len(rows) // 32) * 32
    rows_h = np.concatenate([rows.numpy(), np.full(Tp - len(rows), -1, np.int32)])
    rows_d = torch.from_numpy(rows_h).to(dev)
    Vp, D, L = 36, 768, 7
    outs = (torch.empty(Tp, Vp, D, device=dev), torch.empty(Tp, Vp, L, device=dev),
            torch.empty(Tp, Vp, dtype=torch.int64, device=dev), torch.empty(Tp, dtype=torch.int64, device=dev))
    for _ in range(20):
        pano_rows(store, tab.pano, rows_h, rows_d, *outs)
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            pano_rows(store, tab.pano, rows_h, rows_d, *outs)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 100)
    real = int((rows_h >= 0).sum())
    nbytes = real * 36 * D * 2 + Tp * Vp * (D * 4 + L * 4 + 8) + real * 36 * (L * 4 + 2) + Tp * 12
    us = float(np.median(times)) * 1e3
    print(json.dumps({"what": "bevbert_pd_pano_rows alone (device events around 100 launches incl. the host-side checks, median "
                              "of 5)", "Tp": Tp, "real_panoramas": real, "Vp": Vp, "D": D, "store_rows": N,
                      "store_GiB": round(store.nbytes() / 2 ** 30, 2), "us_per_launch": round(us, 2),
                      "bytes_moved": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}), flush=True)
    if a.kernel_only:
        return
    # ---- 2. sustained through the loader against resident replays
    cfg = BevBertConfig(image_feat_size=768)
    model = GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    arena = model.finalize(dev, torch.bfloat16)
    model.train()
    model.set_dropout(0.1)
    tr = PretrainTrainer(model, arena, learning_rate=5e-5, warmup_steps=100, num_train_steps=100000)
    # the grid store is not what is measured here: 1024 rows, every viewpoint mapped onto one of them
    n_grid, P = 1024, 12 * cfg.grid_hw ** 2
    grid = GridFeatureStore([f"g{i}" for i in range(n_grid)], torch.randn(n_grid, P, 768, generator=g, device=dev).half(),
                            torch.rand(n_grid, 12, cfg.grid_hw, cfg.grid_hw, generator=g, device=dev) * 0.6,
                            torch.randint(0, cfg.sem_classes, (n_grid, P), generator=g, device=dev).to(torch.uint8), dev)
    cycle = ["mlm"] * 5 + ["sap"] * 5 + ["masksem"]
    batches = pd.PathBatchSource(data, tab, cycle, a.batch, seed=4, end_vp_pos_ratio=0.2)
    src = ((t, hb, [f"g{tab.pano.row[k] % n_grid}" for k in keys], rows) for t, hb, keys, rows in batches)
    mgr = BucketManager(cfg, dev, depth=2, max_buckets=64, grid_store=grid, view_store=store, pano_table=tab.pano)
    loader = StreamingLoader(src, mgr, prefetch=1)
    it = iter(loader)

    def run_loader(n):
        eager = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            task, sb = next(it)
            eager += sb.graph is None
            tr.step(task, sb)
            loader.release(sb)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, eager

    def run_resident(n):
        time.sleep(0.3)         # the producer fills the queue and blocks: the sets it holds are then marked in_use, the rest are idle
        sbs = [sb for bk in list(mgr.buckets.values()) for sb in bk["sets"] if sb.graph is not None and not sb.in_use]
        if not sbs:
            return float("nan"), 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            sb = sbs[k % len(sbs)]
            tr.step(sb.task, sb)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, len(sbs)
    t0 = time.perf_counter()
    warm = 0
    while warm < a.warm and time.perf_counter() - t0 < a.warm_seconds:
        run_loader(10)
        warm += 10
    quiet_gc()
    blocks = []
    for _ in range(a.blocks):
        s0 = dict(mgr.stats)
        l, eager = run_loader(a.steps)
        st = {k: mgr.stats[k] - s0.get(k, 0) for k in ("loader_s", "source_s", "wait_s", "queue_s", "buckets_created")}
        r, n_res = run_resident(a.steps)
        blocks.append(dict(loader_ms=round(l * 1e3, 3), resident_ms=round(r * 1e3, 3), eager_steps=int(eager),
                           resident_sets=n_res, **{k: round(v / a.steps * 1e3, 3) if k.endswith("_s") else v for k, v in st.items()}))
    loader.close()
    lm, rm = np.median([x["loader_ms"] for x in blocks]), np.median([x["resident_ms"] for x in blocks])
    print(json.dumps(dict(info, what="sustained: PathBatchSource -> StreamingLoader -> captured steps, against resident replays "
                                     "of the same trainer, alternating blocks, medians", batch=a.batch, steps_per_block=a.steps,
                          warmup_steps=warm, loader_samples_per_s=round(1e3 * a.batch / lm, 1), resident_samples_per_s=round(1e3 * a.batch / rm, 1),
                          vs_resident=round(float(rm / lm), 4), buckets=len(mgr.buckets), captured_graphs=mgr.captured_graphs(),
                          blocks=blocks)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--replicas", type=int, default=44)
    ap.add_argument("--items", type=int, default=14000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--warm-seconds", type=float, default=90.0)
    a = ap.parse_args()
    if a.host:
        host(a)
    if a.gpu:
        gpu(a)
    if not (a.host or a.gpu):
        ap.error("--host and/or --gpu")
