"""Regenerate tests/golden/path_data.npz from the reference's own data layer (pretrain_src/data/dataset.py
``R2RTextPathData``, tasks.py ``MlmDataset`` / ``SapDataset`` / ``MaskSemDataset`` and their collates), on the CPU.

Shims, installed before the reference is imported (the torch_scatter stub of make_golden.py is the precedent):
  * h5py: ``File`` is a dict-backed stand-in (``f[key][...]`` on numpy arrays registered per file name);
  * jsonlines: ``open`` yields one JSON object per line; cv2, MatterSim, torch_scatter: empty modules;
  * model.bev_visualize (opens the simulator and two HDF5 files at import): a module with a no-op ``draw_state``;
  * the numpy aliases the reference still uses: np.long, np.bool, np.int.

Fixture (all from SEED): the three real scans of nav_scans.npz written back as connectivity JSON; ``scanvp_cands`` gives
every viewpoint its graph neighbours as candidates with fabricated view indices / offsets, one viewpoint with two
candidates on ONE view index (37 tokens) and at least one viewpoint with a single candidate; a dozen items: shortest
paths of 2..7 nodes, one walk of more than 20 nodes that re-visits nodes, one single-node path, instructions shorter and
longer than max_txt_len.  View features encode identity (channel 0: the viewpoint's row in ``keys``, channel 1: the
view), so the golden stores (row, view) maps instead of features.

Recorded: ``get_input`` (return_act_label=True) for every prefix of every item -- the end index is forced through the
wrapped ``np.random.randint`` -- and one collated batch per task with every draw the reference consumed
(``random.random`` / ``random.choice`` / ``np.random.rand`` / ``np.random.randint``, per sample).

Usage:  python tests/golden/make_path_data_golden.py [--reference DIR]      (writes tests/golden/path_data.npz)
Also prints the reference's host cost per sample (get_input + task __getitem__ + collate) on this fixture.
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SEED = 20240917
IMAGE_FEAT, STORE_FEAT, MAX_TXT_LEN = 8, 10, 32
POS_RATIO, MASK_PROB, BATCH = 0.5, 0.15, 4
GRID = (12, 196, 768)


# ----------------------------------------------------------------------------- shims
_H5 = {}            # file name -> {key: array}


class _File:
    def __init__(self, name, mode="r"):
        self.d = _H5[name]

    def __enter__(self):
        return self.d

    def __exit__(self, *a):
        return False


class _Lines:
    def __init__(self, path):
        self.f = open(path)

    def __enter__(self):
        return (json.loads(l) for l in self.f if l.strip())

    def __exit__(self, *a):
        self.f.close()
        return False


def install_shims():
    for name in ("cv2", "MatterSim", "torch_scatter"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torch_scatter"].scatter_max = sys.modules["torch_scatter"].scatter_mean = None
    h5 = types.ModuleType("h5py")
    h5.File = _File
    sys.modules["h5py"] = h5
    jl = types.ModuleType("jsonlines")
    jl.open = lambda path, mode="r": _Lines(path)
    sys.modules["jsonlines"] = jl
    viz = types.ModuleType("model.bev_visualize")
    viz.draw_state = lambda *a, **k: None
    sys.modules["model.bev_visualize"] = viz
    for alias, t in (("long", np.int64), ("bool", np.bool_), ("int", np.int64)):
        if alias not in np.__dict__:
            setattr(np, alias, t)


# ----------------------------------------------------------------------------- fixture
def write_connectivity(d):
    raw = np.load(os.path.join(HERE, "nav_scans.npz"))
    scans = sorted({k.split("/")[0] for k in raw.files})
    for s in scans:
        ids, inc, un, pose = (raw[f"{s}/{k}"] for k in ("ids", "included", "unobstructed", "pose"))
        with open(os.path.join(d, f"{s}_connectivity.json"), "w") as f:
            json.dump([{"image_id": str(i), "included": bool(a), "unobstructed": [bool(x) for x in u],
                        "pose": [float(p) for p in po]} for i, a, u, po in zip(ids, inc, un, pose)], f)
    with open(os.path.join(d, "scans.txt"), "w") as f:
        f.write("\n".join(scans) + "\n")
    return scans


def make_fixture(graphs, shortest_paths, rng):
    """(scanvp_cands, items) -- see the module docstring."""
    cands = {}
    for scan, G in graphs.items():
        for vp in G.nodes:
            nb = list(G[vp])
            views = rng.choice(36, size=len(nb), replace=len(nb) > 36)
            cands[f"{scan}_{vp}"] = {
                n: [int(v), float(rng.uniform(0.5, 5)), float(rng.uniform(-0.25, 0.25)), float(rng.uniform(-0.25, 0.25))]
                for n, v in zip(nb, views)}
    single = [k for k, c in cands.items() if len(c) == 1]
    assert single, "no viewpoint with one candidate in the fixture scans"
    shared = next(k for k, c in cands.items() if 3 <= len(c) <= 30)
    first, second = list(cands[shared])[:2]
    cands[shared][second][0] = cands[shared][first][0]
    items = []

    def add(scan, path, n_txt):
        ids = [101] + [int(x) for x in rng.integers(1000, 29000, size=n_txt - 2)] + [102]
        items.append({"instr_id": f"{1000 + len(items)}_{len(items) % 3}", "scan": scan, "path": list(path),
                      "heading": float(rng.uniform(0, 2 * np.pi)), "instr_encoding": ids})
    scans = list(graphs)
    txt = [10, 50, 24, 33, 31, 32, 12, 45, 20, 28, 40, 16]
    # shortest paths of 2..7 nodes; two of them end next to / start at the special viewpoints
    for k, L in enumerate([2, 3, 4, 5, 6, 7, 3, 5, 4]):
        scan = scans[k % len(scans)]
        nodes = list(graphs[scan].nodes)
        if k == 6:
            scan, start = shared.split("_", 1)
            pool = [p for p in shortest_paths[scan][start].values() if len(p) == L]
        elif k == 7:
            scan, leaf = single[0].split("_", 1)
            pool = [p[::-1] for p in shortest_paths[scan][leaf].values() if len(p) == L]      # ends on the leaf
        else:
            pool = [p for u in nodes for p in shortest_paths[scan][u].values() if len(p) == L]
        add(scan, pool[int(rng.integers(len(pool)))], txt[k])
    # a walk of 24 nodes that re-visits: every third step goes back where it came from
    scan = scans[-1]
    walk = [list(graphs[scan].nodes)[5]]
    while len(walk) < 24:
        nb = list(graphs[scan][walk[-1]])
        if len(walk) >= 2 and len(walk) % 3 == 0:
            walk.append(walk[-2])
        else:
            walk.append(nb[int(rng.integers(len(nb)))])
    assert len(set(walk)) < len(walk)
    add(scan, walk, txt[9])
    add(scans[0], [list(graphs[scans[0]].nodes)[3]], txt[10])          # single node: 'pos' only
    add(scans[1], shortest_paths[scans[1]][list(graphs[scans[1]].nodes)[0]][list(graphs[scans[1]].nodes)[7]], txt[11])
    return cands, items, shared, single[0]


# ----------------------------------------------------------------------------- recording
class Draws:
    """Wraps the four generators the reference draws from; ``force`` overrides np.random.randint once."""

    def __init__(self):
        self.log = {"random": [], "choice": [], "rand": [], "randint": []}
        self.force = None
        self._orig = (random.random, random.choice, np.random.rand, np.random.randint)
        r, c, nr, ni = self._orig

        def rec(name, fn):
            def w(*a, **k):
                v = fn(*a, **k)
                self.log[name].append(v)
                return v
            return w

        def randint(*a, **k):
            v = ni(*a, **k)
            if self.force is not None:
                v, self.force = self.force, None
            self.log["randint"].append(int(v))
            return v
        random.random, random.choice = rec("random", r), rec("choice", c)
        np.random.rand, np.random.randint = rec("rand", nr), randint

    def take(self):
        out = {k: list(v) for k, v in self.log.items()}
        for v in self.log.values():
            v.clear()
        return out

    def restore(self):
        random.random, random.choice, np.random.rand, np.random.randint = self._orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("BEVBERT_REFERENCE"), help="checkout of MarSaKi/VLN-BEVBert")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or BEVBERT_REFERENCE) must name a checkout of the reference")
    install_shims()
    sys.path.insert(0, os.path.join(args.reference, "pretrain_src"))
    from data import dataset as ref_dataset, tasks as ref_tasks

    rng = np.random.default_rng(SEED)
    tmp = tempfile.mkdtemp()
    write_connectivity(tmp)
    from data.common import load_nav_graphs
    graphs, _, shortest_paths = load_nav_graphs(tmp)
    cands, items, shared, single = make_fixture(graphs, shortest_paths, rng)
    keys = list(cands)
    row = {k: i for i, k in enumerate(keys)}
    with open(os.path.join(tmp, "cands.json"), "w") as f:
        json.dump(cands, f)
    with open(os.path.join(tmp, "anno.jsonl"), "w") as f:
        for it in items:
            f.write(json.dumps(it) + "\n")
    fts = np.zeros((len(keys), 36, STORE_FEAT), dtype=np.float16)
    fts[:, :, 0] = np.arange(len(keys))[:, None]
    fts[:, :, 1] = np.arange(36)[None, :]
    fts[:, :, 2:] = rng.standard_normal((len(keys), 36, STORE_FEAT - 2)).astype(np.float16)
    _H5["img"] = {k: fts[i] for i, k in enumerate(keys)}
    grid_rgb, grid_dep = np.zeros(GRID, np.float16), np.zeros((12, 14, 14), np.float32)
    grid_sem = np.zeros((12, 14, 14), np.uint8)
    for name, arr in (("rgb", grid_rgb), ("depth", grid_dep), ("sem", grid_sem)):
        _H5[name] = {k: arr for k in keys}
    db = ref_dataset.R2RTextPathData([os.path.join(tmp, "anno.jsonl")], "img", "rgb", "depth", "sem",
                                     os.path.join(tmp, "cands.json"), tmp, image_feat_size=IMAGE_FEAT,
                                     image_prob_size=STORE_FEAT - IMAGE_FEAT, max_txt_len=MAX_TXT_LEN)
    draws = Draws()
    R = lambda vps: np.asarray([-1 if v is None else row[f"{scan}_{v}"] for v in vps], dtype=np.int32)
    out = {"keys": np.asarray(keys), "shared_view_key": np.asarray(shared), "single_cand_key": np.asarray(single),
           "image_feat_size": np.int64(IMAGE_FEAT), "store_feat_size": np.int64(STORE_FEAT),
           "max_txt_len": np.int64(MAX_TXT_LEN), "seed": np.int64(SEED), "pos_ratio": np.float64(POS_RATIO),
           "mask_prob": np.float64(MASK_PROB),
           "items": np.asarray(json.dumps(items)), "cands": np.asarray(json.dumps(cands))}

    # ---- every prefix of every item
    from vln_bevbert_amd.nav_expert import ScanGraphs
    from vln_bevbert_amd.path_data import R2RPathData
    twin = R2RPathData(items, ScanGraphs.from_connectivity(
        {s: os.path.join(tmp, f"{s}_connectivity.json") for s in graphs}), cands, IMAGE_FEAT, max_txt_len=MAX_TXT_LEN)
    rec = {}
    put = lambda k, v: rec.setdefault(k, []).append(np.asarray(v))
    n_tokens_max = 0
    for idx, item in enumerate(items):
        scan, n = item["scan"], len(item["path"])
        for e in range(n):
            if e == n - 1:
                s = db.get_input(idx, "pos", return_act_label=True)
            else:
                draws.force = e
                s = db.get_input(idx, "neg_in_gt_path", return_act_label=True)
            draws.take()
            assert all(x.dtype == np.float32 and x.shape[1] == IMAGE_FEAT for x in s["traj_view_img_fts"])
            # pre-round BEV coordinates must not sit on a cell boundary (k + 0.5): the cells then cannot hinge on the
            # last bit of a sine
            si = twin.graphs.scan_index[scan]
            xy = twin.bev_cand_xy(s["S_w2c"][0], si, db.get_cur_angle(scan, item["path"][:e + 1], item["heading"])[0],
                                  [twin.graphs.index[(scan, v)] for v in s["traj_cand_vpids"][-1]])
            assert (np.abs(xy - np.floor(xy) - 0.5) > 1e-4).all(), (idx, e, xy)
            put("idx", idx), put("end_idx", e), put("instr_id", s["instr_id"])
            put("instr_encoding", np.asarray(s["instr_encoding"], dtype=np.int64))
            put("view_lens", [len(x) for x in s["traj_view_img_fts"]])
            put("pano_node", np.concatenate([x[:, 0] for x in s["traj_view_img_fts"]]).astype(np.int32))
            put("pano_view", np.concatenate([x[:, 1] for x in s["traj_view_img_fts"]]).astype(np.int32))
            put("traj_loc_fts", np.concatenate(s["traj_loc_fts"], 0))
            put("traj_nav_types", np.concatenate([np.asarray(x, dtype=np.int64) for x in s["traj_nav_types"]]))
            put("cand_counts", [len(c) for c in s["traj_cand_vpids"]])
            put("traj_cand_vpids", R([v for c in s["traj_cand_vpids"] for v in c]))
            put("traj_vpids", R(s["traj_vpids"])), put("gmap_vpids", R(s["gmap_vpids"]))
            put("gmap_step_ids", np.asarray(s["gmap_step_ids"], dtype=np.int64))
            put("gmap_visited_masks", np.asarray(s["gmap_visited_masks"], dtype=np.int64))
            for k in ("gmap_pos_fts", "gmap_pair_dists", "T_c2w", "T_w2c", "S_w2c", "bev_cand_idxs", "bev_gpos_fts",
                      "global_act_labels", "local_act_labels"):
                put(k, s[k])
            n_tokens_max = max(n_tokens_max, max(rec["view_lens"][-1]))
    assert n_tokens_max == 37
    for k, v in rec.items():
        if v[0].dtype.kind == "U":
            out["prefix/" + k] = np.asarray([str(x) for x in v])
            continue
        nd = max(x.ndim for x in v)
        out["prefix/" + k] = np.concatenate([x.reshape(-1) for x in v])
        out["prefix/" + k + ".shape"] = np.asarray([x.shape + (0,) * (nd - x.ndim) for x in v], dtype=np.int32).reshape(len(v), nd)

    # ---- one collated batch per task, with the draws
    tok = types.SimpleNamespace(cls_token_id=101, sep_token_id=102, mask_token_id=103, pad_token_id=0)
    sets = {"mlm": (ref_tasks.MlmDataset(db, tok, POS_RATIO), ref_tasks.mlm_collate),
            "sap": (ref_tasks.SapDataset(db, tok, POS_RATIO), ref_tasks.sap_collate),
            "masksem": (ref_tasks.MaskSemDataset(db, tok, MASK_PROB, POS_RATIO), ref_tasks.masksem_collate)}
    single_idx = next(i for i, it in enumerate(items) if len(it["path"]) == 1)
    for t, (task, (ds, coll)) in enumerate(sets.items()):
        np.random.seed(SEED + t)
        random.seed(SEED + t)
        idxs = [int(i) for i in rng.permutation([i for i in range(len(items)) if i != single_idx])[:BATCH]]
        samples, logs = [], []
        for i in idxs:
            samples.append(ds[i])
            logs.append(draws.take())
        ends = [len(items[i]["path"]) - 1 if l["rand"][0] < POS_RATIO else l["randint"][0] for i, l in zip(idxs, logs)]
        b = coll(samples)
        out[f"{task}/idx"], out[f"{task}/end_idx"] = np.asarray(idxs), np.asarray(ends)
        for name in ("random", "choice", "rand", "randint"):
            out[f"{task}/draw.{name}"] = np.asarray([x for l in logs for x in l[name]], dtype=np.float64)
            out[f"{task}/draw.{name}.n"] = np.asarray([len(l[name]) for l in logs])
        for k, v in b.items():
            if k in ("rgbs", "depths", "sems"):
                continue
            if k == "traj_view_img_fts":
                out[f"{task}/pano_node"], out[f"{task}/pano_view"] = v[..., 0].numpy().astype(np.int32), v[..., 1].numpy().astype(np.int32)
                assert v.dtype == torch.float32 and v.shape[-1] == IMAGE_FEAT
            elif torch.is_tensor(v):
                out[f"{task}/{k}"] = v.numpy()
            elif k == "traj_step_lens":
                out[f"{task}/{k}"] = np.asarray(v)
        for bi, i in enumerate(idxs):           # id lists: rows of ``keys``
            scan = items[i]["scan"]
            out[f"{task}/traj_vpids.{bi}"] = R(b["traj_vpids"][bi])
            out[f"{task}/gmap_vpids.{bi}"] = R(b["gmap_vpids"][bi])
            out[f"{task}/cand_counts.{bi}"] = np.asarray([len(c) for c in b["traj_cand_vpids"][bi]])
            out[f"{task}/traj_cand_vpids.{bi}"] = R([v for c in b["traj_cand_vpids"][bi] for v in c])

    # ---- the reference's host cost per sample on this fixture (no disk: the HDF5 stand-in is a dict)
    ds, coll = sets["sap"]
    order = [i for i in range(len(items)) if i != single_idx]
    t0 = time.perf_counter()
    n = 0
    for _ in range(6):
        batch = [ds[order[(n + k) % len(order)]] for k in range(8)]
        coll(batch)
        n += 8
    dt = (time.perf_counter() - t0) / n
    db.get_scanvp_grid_feature = lambda scan, vp: (np.zeros((0,), np.float32), np.zeros((0,), np.float32), np.zeros((0,), np.uint8))
    t0 = time.perf_counter()
    m = 0
    for _ in range(20):
        for i in order:
            db.get_input(i, "neg_in_gt_path", return_act_label=True)
            m += 1
    dt_in = (time.perf_counter() - t0) / m
    draws.restore()
    print(f"reference host cost on this fixture: get_input + SapDataset item + sap_collate {dt * 1e3:.2f} ms/sample "
          f"(grid arrays of full size, widened and one-hot encoded as the reference does); get_input alone without the grid "
          f"arrays {dt_in * 1e3:.3f} ms/sample")
    path = os.path.join(HERE, "path_data.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(rec["idx"]), "prefixes,", len(items), "items")


if __name__ == "__main__":
    main()
