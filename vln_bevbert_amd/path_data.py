"""R2R pre-training inputs from tables: the host twin of the reference's data layer, and the batch source built on it.

The reference builds every sample in per-sample Python (pretrain_src/data/dataset.py:443-622 ``R2RTextPathData``,
tasks.py ``MlmDataset`` / ``SapDataset`` / ``MaskSemDataset`` and their collates): ordered dicts over the path,
``dict[scan][a][b]`` lookups in a G x G double loop, one ``calculate_vp_rel_pos_fts`` call per node, and the 36 view
features of every step shipped from the host.  All of it except three random draws (the end index, the MLM masks, the
MaskSEM masks) is a function of a path PREFIX -- an item plus an end index -- so it is computed once and kept:

    R2RPathData      the twin itself: ``get_input(idx, end_idx)`` restates dataset.py:489-578 as executed
    PanoTable        per viewpoint: view order, token count, traj_loc_fts rows, traj_nav_types (path-independent)
    PrefixTables     per prefix, CSR / padded numpy arrays: panorama rows, map nodes, step ids, visited masks,
                     gmap_pos_fts, bev_gpos_fts, T_c2w / T_w2c / S_w2c, bev_cand_idxs, the two labels, shape counts
    draw / mask_tokens / bev_mrc_masks / collate     the random draws and the three tasks' collates
    PathBatchSource  (task, host batch, grid keys, pano rows) for loader.BucketManager / StreamingLoader

The panorama tensors of a batch are not built here at all: a batch carries ``pano_rows`` and csrc/path_data.hip
(ops: ``pano_rows``) gathers them on the device from a resident feature_store.ViewFeatureStore and the PanoTable.

Quirks of the reference, kept as executed (each is marked [Qn] where it is restated):
  [Q1] get_gmap_inputs walks two ordered dicts: ``visited[vp] = t + 1`` overwrites on a re-visit (the node keeps its
       first position, takes the last step id); ``del unvisited[vp]`` followed by a later re-insertion moves a node to
       the end of the unvisited list.
  [Q2] ``cur_heading`` comes from the last edge of the FULL prefix, before the TRAIN_MAX_STEP = 20 truncation
       (``gt_path[:20] + [end_vp]``).
  [Q3] ``path_viewidxs=None``: every panorama's angles are relative to base view 12, whatever the agent's heading.
  [Q4] two candidates of a viewpoint may share a view index; ``used_viewidxs`` is a set, so such a panorama has more than
       36 tokens (every candidate is a token, the shared view is left out of the rest only once).
  [Q5] end-vp type 'neg_others' draws like 'neg_in_gt_path' (dataset.py:503).
  [Q6] bev_cand_idxs: fp32 arithmetic throughout, ``T_cand.transpose(0, 1)`` is numpy's axis permutation (0, 1), i.e. NO
       transpose; ``np.round`` rounds half to even; cells are clamped to the grid.
  [Q7] get_act_labels: 'stop' is decided by ``end_vp == path[-1]`` (true at an earlier visit of the last node too); the
       next viewpoint is looked up in the map and among the last panorama's candidates, and a label that finds
       nothing falls through to -100.
  [Q8] an item whose path has one node can only be drawn as 'pos': the reference's ``np.random.randint(0)`` raises for
       it; ``draw`` takes 'pos' there.
Random numbers: a numpy Generator owned by the source; it matches the reference's distributions, not its stream.
"""
import json
import math
import os
import types

import numpy as np
import torch

from . import synthetic
from .synthetic import pose_matrix

MAX_DIST = 30           # dataset.py:19-21
MAX_STEP = 10
TRAIN_MAX_STEP = 20
N_VIEWS = 36
VOCAB_RANGE = (1996, 29611)     # tasks.py:62
MASK_ID = 103
TASKS = ("mlm", "sap", "masksem")


# ----------------------------------------------------------------------------- data/common.py, as executed
def view_rel_angles(base_view=0):
    """get_view_rel_angles (common.py:51-68): (36, 2) fp32, headings accumulated in Python floats."""
    rel = np.zeros((N_VIEWS, 2), dtype=np.float32)
    base_heading = (base_view % 12) * math.radians(30)
    base_elevation = (base_view // 12 - 1) * math.radians(30)
    for ix in range(N_VIEWS):
        if ix == 0:
            heading = 0
            elevation = math.radians(-30)
        elif ix % 12 == 0:
            heading = 0
            elevation += math.radians(30)
        else:
            heading += math.radians(30)
        rel[ix, 0] = heading - base_heading
        rel[ix, 1] = elevation - base_elevation
    return rel


def angle_fts(headings, elevations, angle_feat_size):
    """get_angle_fts (common.py:43-49)."""
    fts = [np.sin(headings), np.cos(headings), np.sin(elevations), np.cos(elevations)]
    fts = np.vstack(fts).transpose().astype(np.float32)
    rep = angle_feat_size // 4
    if rep > 1:
        fts = np.concatenate([fts] * rep, 1)
    return fts


def rel_pos_fts(a, b, base_heading=0, base_elevation=0):
    """calculate_vp_rel_pos_fts (common.py:111-128): a, b are the fp64 position arrays of the graph nodes."""
    dx = b[0] - a[0]
    dy = b[1] - a[1]
    dz = b[2] - a[2]
    xy_dist = max(np.sqrt(dx ** 2 + dy ** 2), 1e-8)
    xyz_dist = max(np.sqrt(dx ** 2 + dy ** 2 + dz ** 2), 1e-8)
    heading = np.arcsin(dx / xy_dist)
    if b[1] < a[1]:
        heading = np.pi - heading
    heading -= base_heading
    elevation = np.arcsin(dz / xyz_dist)
    elevation -= base_elevation
    return heading, elevation, xyz_dist


# ----------------------------------------------------------------------------- the twin
class R2RPathData:
    """``R2RTextPathData`` without its files: annotation dicts, a nav_expert.ScanGraphs and the candidate table."""

    def __init__(self, items, graphs, scanvp_cands, image_feat_size, angle_feat_size=4, max_txt_len=100,
                 act_visited_node=False, bev_dim=21, bev_res=0.5, view_fts=None):
        """``scanvp_cands``: {'<scan>_<vp>': {cand vp: [view index, distance, rel. heading, rel. elevation]}} in file
        order.  ``view_fts``: optional {'<scan>_<vp>': (36, Ds) array}; with it ``get_input`` also returns the
        reference's ``traj_view_img_fts``, without it only the view order (``traj_view_idxs``)."""
        self.items = list(items)
        self.graphs = graphs
        self.scanvp_cands = scanvp_cands
        self.image_feat_size, self.angle_feat_size = image_feat_size, angle_feat_size
        self.max_txt_len, self.act_visited_node = max_txt_len, act_visited_node
        self.bev_dim, self.bev_res = bev_dim, bev_res
        self.view_fts = view_fts
        self.base_angles = view_rel_angles(12)          # all_point_rel_angles[12]
        self._pano, self._pos = {}, {}

    @classmethod
    def from_files(cls, anno_files, connectivity_dir, scanvp_cands_file, image_feat_size, **kw):
        """The reference's constructor arguments: .jsonl annotation files (one JSON object per line),
        ``<dir>/scans.txt`` + ``<scan>_connectivity.json``, and the candidate json."""
        from .nav_expert import ScanGraphs
        items = []
        for path in anno_files:
            with open(path) as f:
                items += [json.loads(line) for line in f if line.strip()]
        with open(os.path.join(connectivity_dir, "scans.txt")) as f:
            scans = [x.strip() for x in f if x.strip()]
        graphs = ScanGraphs.from_connectivity(
            {s: os.path.join(connectivity_dir, f"{s}_connectivity.json") for s in scans})
        with open(scanvp_cands_file) as f:
            cands = json.load(f)
        return cls(items, graphs, cands, image_feat_size, **kw)

    def __len__(self):
        return len(self.items)

    # ---- per viewpoint ------------------------------------------------------------------------------------------
    def pano(self, scan, vp):
        """One panorama of get_traj_pano_fts (dataset.py:587-620): (view order, loc_fts (n, angle + 3) fp32, nav types,
        candidate ids).  A function of the viewpoint alone [Q3]."""
        key = "%s_%s" % (scan, vp)
        hit = self._pano.get(key)
        if hit is not None:
            return hit
        order, view_angles, cand_vpids = [], [], []
        used = set()
        for k, v in self.scanvp_cands[key].items():
            used.add(v[0])                                   # [Q4] a set: a shared view index is counted once
            order.append(v[0])
            a = self.base_angles[v[0]]                       # [Q3]
            view_angles.append([a[0] + v[2], a[1] + v[3]])
            cand_vpids.append(k)
        order.extend([i for i in range(N_VIEWS) if i not in used])
        view_angles.extend([self.base_angles[i] for i in range(N_VIEWS) if i not in used])
        view_angles = np.stack(view_angles, 0)
        ang = angle_fts(view_angles[:, 0], view_angles[:, 1], self.angle_feat_size)
        box = np.array([[1, 1, 1]] * len(order)).astype(np.float32)
        loc = np.concatenate([ang, box], 1)
        nav = [1] * len(cand_vpids) + [0] * (N_VIEWS - len(used))
        hit = self._pano[key] = (np.asarray(order, dtype=np.uint8), loc, nav, cand_vpids)
        return hit

    # ---- per prefix ---------------------------------------------------------------------------------------------
    def _cur_angle(self, scan, path, start_heading):
        """get_cur_angle (dataset.py:245-256)."""
        if len(path) < 2:
            return start_heading, 0
        viewidx = self.scanvp_cands["%s_%s" % (scan, path[-2])][path[-1]][0]
        return (viewidx % 12) * math.radians(30), 0

    def _pos_row(self, si, cur, vp, heading, elevation):
        """One node of get_gmap_pos_fts: ([rel_heading, rel_elevation], [line, shortest, steps]), cached per
        (scan, current node, heading, node)."""
        key = (si, cur, vp, heading)
        hit = self._pos.get(key)
        if hit is None:
            g = self.graphs
            h, e, d = rel_pos_fts(g.positions[si][cur], g.positions[si][vp], base_heading=heading,
                                  base_elevation=elevation)
            hit = self._pos[key] = ([h, e], [d / MAX_DIST, g.dist[si, cur, vp] / MAX_DIST,
                                             int(g.hops[si, cur, vp]) / MAX_STEP])
        return hit

    def pos_fts(self, si, cur, nodes, heading, elevation):
        """get_gmap_pos_fts (dataset.py:362-384) over node indices (-1: the [stop] token)."""
        rel_angles, rel_dists = [], []
        for vp in nodes:
            if vp < 0:
                rel_angles.append([0, 0])
                rel_dists.append([0, 0, 0])
            else:
                a, d = self._pos_row(si, cur, vp, heading, elevation)
                rel_angles.append(a)
                rel_dists.append(d)
        rel_angles = np.array(rel_angles).astype(np.float32)
        rel_dists = np.array(rel_dists).astype(np.float32)
        return np.concatenate([angle_fts(rel_angles[:, 0], rel_angles[:, 1], self.angle_feat_size), rel_dists], 1)

    def gmap_walk(self, scan, path):
        """The ordered-dict walk of get_gmap_inputs (dataset.py:330-349) [Q1]: (vpids, step ids, visited masks)."""
        visited, unvisited = {}, {}
        for t, vp in enumerate(path):
            visited[vp] = t + 1
            if vp in unvisited:
                del unvisited[vp]
            for nxt in self.scanvp_cands["%s_%s" % (scan, vp)].keys():
                if nxt not in visited:
                    unvisited[nxt] = 0
        vpids = [None] + list(visited.keys()) + list(unvisited.keys())
        step_ids = [0] + list(visited.values()) + list(unvisited.values())
        if self.act_visited_node:
            masks = [0] + [1 if vp == path[-1] else 0 for vp in vpids[1:]]
        else:
            masks = [0] + [1] * len(visited) + [0] * len(unvisited)
        return vpids, step_ids, masks

    def pair_dists(self, si, nodes):
        """gmap_pair_dists (dataset.py:354-358): fp64 ``/ 30`` assigned into an fp32 array; row / column 0 ([stop]) zero."""
        n = np.asarray(nodes[1:], dtype=np.int64)
        out = np.zeros((len(nodes), len(nodes)), dtype=np.float32)
        sub = np.triu(self.graphs.dist[si][n[:, None], n[None, :]] / MAX_DIST, 1)       # [i, j] with i < j, mirrored
        out[1:, 1:] = sub + sub.T
        return out

    def bev_cand_xy(self, S_cand, si, heading, cand_nodes):
        """Candidate positions in BEV cells before rounding (dataset.py:420-432), fp32 [Q6]."""
        pos = self.graphs.positions[si]
        xyzhe = np.zeros([1, 5]).astype(np.float32)
        xyzhe[:, 3] = -heading
        T_cand = pose_matrix(xyzhe)[0]
        cand_pos = np.array([pos[vp] for vp in cand_nodes]).astype(np.float32)
        cand_pos = cand_pos[:, [0, 2, 1]] * np.array([1, 1, -1], dtype=np.float32)
        cand_pos = cand_pos - S_cand
        ones = np.ones([cand_pos.shape[0], 1]).astype(np.float32)
        cand_pos1 = np.concatenate([cand_pos, ones], axis=-1)
        cand_pos1 = np.dot(cand_pos1, T_cand.transpose(0, 1))          # [Q6] axes (0, 1): not a transpose
        cand_pos = cand_pos1[:, :3]
        return cand_pos[:, [0, 2]] / self.bev_res

    def bev_inputs(self, si, cur, heading, cand_nodes):
        """get_bev_inputs (dataset.py:397-440) without the grid features: T_c2w, T_w2c, S_w2c, bev_cand_idxs [Q6]."""
        pos = self.graphs.positions[si]
        x, y, z = pos[cur][:3]
        xyzhe = np.zeros([12, 5]).astype(np.float32)
        xyzhe[:, 0] = x
        xyzhe[:, 1] = z
        xyzhe[:, 2] = -y
        xyzhe[:, 3] = -np.arange(12) * np.radians(30)
        xyzhe[:, 4] = np.pi
        T_c2w = pose_matrix(xyzhe)
        S_w2c = xyzhe[:1, :3].copy()
        xyzhe = np.zeros([1, 5]).astype(np.float32)
        xyzhe[:, 3] = heading
        T_w2c = pose_matrix(xyzhe)
        cand_pos = self.bev_cand_xy(S_w2c[0], si, heading, cand_nodes).round() + (self.bev_dim - 1) // 2
        cand_pos[cand_pos < 0] = 0
        cand_pos[cand_pos >= self.bev_dim] = self.bev_dim - 1
        cand_pos = cand_pos.astype(np.int64)
        idxs = cand_pos[:, 1] * self.bev_dim + cand_pos[:, 0]
        idxs = np.insert(idxs, 0, (self.bev_dim * self.bev_dim - 1) // 2)
        return T_c2w, T_w2c, S_w2c, idxs

    @staticmethod
    def act_labels(item, end_vp, end_idx, gmap_vpids, last_cands):
        """R2RTextPathData.get_act_labels (dataset.py:471-487) [Q7]."""
        if end_vp == item["path"][-1]:
            return 0, 0
        g = l = -100
        nxt = item["path"][end_idx + 1]
        for k, vp in enumerate(gmap_vpids):
            if vp == nxt:
                g = k
                break
        for k, vp in enumerate(last_cands):
            if vp == nxt:
                l = k + 1
                break
        return g, l

    def draw(self, task, idxs, rng, end_vp_pos_ratio):
        """End indices of a batch with the reference's branch probabilities (tasks.py:74-78 MLM, :319-325 SAP, :630-634
        MaskSEM): one uniform picks 'pos' (r < ratio: the last node) or a negative, and a negative is uniform over
        ``path[:-1]`` -- for SAP both of its negative branches, since 'neg_others' draws like 'neg_in_gt_path' [Q5].
        A one-node path is always 'pos' [Q8]."""
        out = np.empty(len(idxs), dtype=np.int64)
        for k, i in enumerate(idxs):
            n = len(self.items[int(i)]["path"])
            r = rng.random()
            if r < end_vp_pos_ratio or n < 2:
                out[k] = n - 1
            else:       # SAP: r < 0.6 -> 'neg_in_gt_path', else 'neg_others'; the same draw either way [Q5]
                out[k] = int(rng.integers(n - 1))
        return out

    def get_input(self, idx, end_idx):
        """dataset.py:489-578 with ``return_act_label=True`` for the prefix ``path[:end_idx + 1]``; ``rgbs`` / ``depths``
        / ``sems`` are replaced by ``grid_key`` = '<scan>_<end_vp>'."""
        item = self.items[idx]
        scan, full = item["scan"], item["path"]
        si = self.graphs.scan_index[scan]
        node = lambda vp: self.graphs.index[(scan, vp)]
        start_vp, end_vp = full[0], full[end_idx]
        path = full[:end_idx + 1]
        heading, elevation = self._cur_angle(scan, path, item["heading"])       # [Q2] before the truncation
        if len(path) > TRAIN_MAX_STEP:
            path = path[:TRAIN_MAX_STEP] + [end_vp]
        panos = [self.pano(scan, vp) for vp in path]
        vpids, step_ids, masks = self.gmap_walk(scan, path)
        nodes = [-1] + [node(vp) for vp in vpids[1:]]
        last_cands = panos[-1][3]
        T_c2w, T_w2c, S_w2c, bev_cand_idxs = self.bev_inputs(si, node(end_vp), heading, [node(vp) for vp in last_cands])
        g_lab, l_lab = self.act_labels(item, end_vp, end_idx, vpids, last_cands)
        out = {
            "instr_id": item["instr_id"],
            "instr_encoding": item["instr_encoding"][:self.max_txt_len],
            "traj_view_idxs": [p[0] for p in panos],
            "traj_loc_fts": [p[1] for p in panos],
            "traj_nav_types": [p[2] for p in panos],
            "traj_cand_vpids": [p[3] for p in panos],
            "traj_vpids": path,
            "gmap_vpids": vpids,
            "gmap_step_ids": step_ids,
            "gmap_visited_masks": masks,
            "gmap_pos_fts": self.pos_fts(si, node(path[-1]), nodes, heading, elevation),
            "gmap_pair_dists": self.pair_dists(si, nodes),
            "grid_key": "%s_%s" % (scan, end_vp),
            "T_c2w": T_c2w,
            "T_w2c": T_w2c,
            "S_w2c": S_w2c,
            "bev_cand_idxs": bev_cand_idxs,
            "bev_gpos_fts": self.pos_fts(si, node(end_vp), [node(start_vp)], heading, elevation),
            "global_act_labels": g_lab,
            "local_act_labels": l_lab,
        }
        if self.view_fts is not None:
            out["traj_view_img_fts"] = [
                np.asarray(self.view_fts["%s_%s" % (scan, vp)]).astype(np.float32)[p[0]][:, :self.image_feat_size]
                for vp, p in zip(path, panos)]
        return out


# ----------------------------------------------------------------------------- tables
class PanoTable:
    """Per viewpoint, in the key order of ``scanvp_cands``: what a panorama contributes to a batch besides its features."""
    FIELDS = ("view_order", "n_tokens", "loc_fts", "nav_types")        # what the device gather reads

    def __init__(self, keys, view_order, n_tokens, loc_fts, nav_types, cand_ids=None):
        """``cand_ids``: (N, Cmax) candidate viewpoint ids in dict order, '' beyond a viewpoint's candidates (the id lists
        of ``traj_cand_vpids``); tables cut or tiled from others may leave it out."""
        self.keys = [str(k) for k in keys]
        self.row = {k: i for i, k in enumerate(self.keys)}
        self.view_order = np.ascontiguousarray(view_order, dtype=np.uint8)      # (N, Vmax): store view of token v
        self.n_tokens = np.ascontiguousarray(n_tokens, dtype=np.int32)          # (N)
        self.loc_fts = np.ascontiguousarray(loc_fts, dtype=np.float32)          # (N, Vmax, L)
        self.nav_types = np.ascontiguousarray(nav_types, dtype=np.uint8)        # (N, Vmax)
        self.cand_ids = None if cand_ids is None else np.asarray(cand_ids)
        self._dev, self._cands = {}, {}

    @classmethod
    def build(cls, data):
        keys = list(data.scanvp_cands)
        panos = [data.pano(*k.split("_", 1)) for k in keys]
        N, Vmax = len(keys), max(len(p[0]) for p in panos)
        L = panos[0][1].shape[1]
        order = np.zeros((N, Vmax), dtype=np.uint8)
        loc = np.zeros((N, Vmax, L), dtype=np.float32)
        nav = np.zeros((N, Vmax), dtype=np.uint8)
        n = np.zeros(N, dtype=np.int32)
        for i, (o, l, t, _) in enumerate(panos):
            n[i] = len(o)
            order[i, :len(o)], loc[i, :len(o)], nav[i, :len(t)] = o, l, t
        width = max(len(p[3]) for p in panos)
        return cls(keys, order, n, loc, nav, np.asarray([list(p[3]) + [""] * (width - len(p[3])) for p in panos]))

    def cands(self, row):
        """Candidate viewpoint ids of a row, as the list ``traj_cand_vpids`` holds (built once per row)."""
        hit = self._cands.get(row)
        if hit is None:
            hit = self._cands[row] = [str(c) for c in self.cand_ids[row] if c]
        return hit

    def pano(self, row):
        n = int(self.n_tokens[row])
        return self.view_order[row, :n], self.loc_fts[row, :n], self.nav_types[row, :n].tolist()

    def to(self, device):
        """The four arrays as device tensors (uploaded once per device)."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(getattr(self, f)).to(device) for f in self.FIELDS)
        return self._dev[key]


class PrefixTables:
    """Every prefix of every item.  Prefix ``p = item_start[idx] + end_idx``; ragged fields are CSR (``*_ptr``)."""
    ARRAYS = ("item_start", "scan", "end_node", "pano_ptr", "pano_rows", "pano_nodes", "gmap_ptr", "gmap_nodes",
              "gmap_step_ids", "gmap_visited_masks", "gmap_pos_fts", "bev_gpos_fts", "T_c2w", "T_w2c", "S_w2c", "cand_ptr",
              "bev_cand_idxs", "global_act_labels", "local_act_labels", "max_tokens", "txt_lens")

    def __init__(self, data=None):
        self.pano = None
        if data is not None:
            self._build(data)

    def _build(self, data):
        g = data.graphs
        self.pano = PanoTable.build(data)
        a = {k: [] for k in self.ARRAYS}
        a["item_start"].append(0)
        for k in ("pano_ptr", "gmap_ptr", "cand_ptr"):
            a[k].append(0)
        for idx, item in enumerate(data.items):
            scan = item["scan"]
            si = g.scan_index[scan]
            a["txt_lens"].append(len(item["instr_encoding"][:data.max_txt_len]))
            for e in range(len(item["path"])):
                s = data.get_input(idx, e)
                rows = [self.pano.row["%s_%s" % (scan, vp)] for vp in s["traj_vpids"]]
                a["scan"].append(si)
                a["end_node"].append(g.index[(scan, item["path"][e])])
                a["pano_rows"] += rows
                a["pano_nodes"] += [g.index[(scan, vp)] for vp in s["traj_vpids"]]
                a["pano_ptr"].append(len(a["pano_rows"]))
                a["gmap_nodes"] += [-1] + [g.index[(scan, vp)] for vp in s["gmap_vpids"][1:]]
                a["gmap_step_ids"] += s["gmap_step_ids"]
                a["gmap_visited_masks"] += s["gmap_visited_masks"]
                a["gmap_pos_fts"].append(s["gmap_pos_fts"])
                a["gmap_ptr"].append(len(a["gmap_nodes"]))
                for k in ("bev_gpos_fts", "T_c2w", "T_w2c", "S_w2c", "global_act_labels", "local_act_labels"):
                    a[k].append(s[k])
                a["bev_cand_idxs"].append(s["bev_cand_idxs"])
                a["cand_ptr"].append(a["cand_ptr"][-1] + len(s["bev_cand_idxs"]))
                a["max_tokens"].append(max(int(self.pano.n_tokens[r]) for r in rows))
            a["item_start"].append(len(a["scan"]))
        dt = {"scan": np.int16, "gmap_visited_masks": bool, "gmap_pos_fts": np.float32, "bev_gpos_fts": np.float32,
              "T_c2w": np.float32, "T_w2c": np.float32, "S_w2c": np.float32, "bev_cand_idxs": np.int64,
              "item_start": np.int64, "pano_ptr": np.int64, "gmap_ptr": np.int64, "cand_ptr": np.int64,
              "global_act_labels": np.int64, "local_act_labels": np.int64}
        for k, v in a.items():
            if k in ("gmap_pos_fts", "bev_cand_idxs"):
                v = np.concatenate(v, 0)
            setattr(self, k, np.ascontiguousarray(np.asarray(v), dtype=dt.get(k, np.int32)))

    def __len__(self):
        return len(self.scan)

    # ---- counts a shape signature needs: cheap, no sample is materialised
    def counts(self, p):
        """(panoramas, map nodes incl. [stop], candidates incl. [stop], widest panorama) of prefix p."""
        return (int(self.pano_ptr[p + 1] - self.pano_ptr[p]), int(self.gmap_ptr[p + 1] - self.gmap_ptr[p]),
                int(self.cand_ptr[p + 1] - self.cand_ptr[p]), int(self.max_tokens[p]))

    def save(self, path):
        arrs = {k: getattr(self, k) for k in self.ARRAYS}
        arrs.update({"pano." + f: getattr(self.pano, f) for f in PanoTable.FIELDS})
        arrs["pano.keys"], arrs["pano.cand_ids"] = np.asarray(self.pano.keys), self.pano.cand_ids
        with open(path, "wb") as f:
            np.savez(f, **arrs)

    @classmethod
    def load(cls, path):
        self = cls()
        with np.load(path, allow_pickle=False) as z:
            for k in cls.ARRAYS:
                setattr(self, k, z[k])
            self.pano = PanoTable(z["pano.keys"], *(z["pano." + f] for f in PanoTable.FIELDS), z["pano.cand_ids"])
        return self

    def sample(self, data, idx, end_idx, panos=True):
        """The ``get_input`` dict of a prefix, from the tables alone (``data`` supplies the id strings, the distance
        matrix and the instruction).  ``panos=False`` leaves the per-panorama arrays out: a by-reference batch carries
        ``pano_rows`` instead."""
        p = int(self.item_start[idx]) + end_idx
        g, item = data.graphs, data.items[idx]
        si = int(self.scan[p])
        ids = g.ids[si]
        rows = self.pano_rows[self.pano_ptr[p]:self.pano_ptr[p + 1]]
        g0, g1 = int(self.gmap_ptr[p]), int(self.gmap_ptr[p + 1])
        nodes = self.gmap_nodes[g0:g1]
        scan = g.scans[si]
        out = {
            "instr_id": item["instr_id"],
            "instr_encoding": item["instr_encoding"][:data.max_txt_len],
            "traj_cand_vpids": [self.pano.cands(int(r)) for r in rows],
            "traj_vpids": [ids[n] for n in self.pano_nodes[self.pano_ptr[p]:self.pano_ptr[p + 1]]],
            "traj_vp_view_lens": self.pano.n_tokens[rows].tolist(),
            "pano_rows": rows,
            "gmap_vpids": [None] + [ids[n] for n in nodes[1:]],
            "gmap_step_ids": self.gmap_step_ids[g0:g1].tolist(),
            "gmap_visited_masks": self.gmap_visited_masks[g0:g1].astype(np.int64).tolist(),
            "gmap_pos_fts": self.gmap_pos_fts[g0:g1],
            "gmap_pair_dists": data.pair_dists(si, nodes),
            "grid_key": "%s_%s" % (scan, ids[int(self.end_node[p])]),
            "T_c2w": self.T_c2w[p], "T_w2c": self.T_w2c[p], "S_w2c": self.S_w2c[p],
            "bev_cand_idxs": self.bev_cand_idxs[self.cand_ptr[p]:self.cand_ptr[p + 1]],
            "bev_gpos_fts": self.bev_gpos_fts[p],
            "global_act_labels": int(self.global_act_labels[p]),
            "local_act_labels": int(self.local_act_labels[p]),
        }
        if panos:
            tp = [self.pano.pano(r) for r in rows]
            out.update(traj_view_idxs=[t[0] for t in tp], traj_loc_fts=[t[1] for t in tp],
                       traj_nav_types=[t[2] for t in tp])
        return out


# ----------------------------------------------------------------------------- draws and tasks
def mask_tokens(u, repl, ids, mask_id=MASK_ID):
    """random_word (tasks.py:14-55) as a function of its draws: ``u[k]`` is token k's uniform, ``repl[k]`` the random
    token it takes if its draw lands in the 10 % replace branch.  Returns (tokens, labels), labels -1 where unmasked;
    if nothing was masked, token 0 is."""
    out, lab = [], []
    for k, tok in enumerate(ids):
        prob = u[k]
        if prob < 0.15:
            prob /= 0.15
            if prob < 0.8:
                out.append(mask_id)
            elif prob < 0.9:
                out.append(int(repl[k]))
            else:
                out.append(tok)
            lab.append(tok)
        else:
            out.append(tok)
            lab.append(-1)
    if all(o == -1 for o in lab):
        lab[0] = ids[0]
        out[0] = mask_id
    return out, lab


def bev_mrc_masks(u, mask_prob, pick=0):
    """_get_img_mask (tasks.py:167-173): cell k is masked if ``u[k] < mask_prob``; if none is, the reference draws ONE
    cell uniformly (``np.random.randint(num_images)``) -- ``pick`` is that draw."""
    m = np.asarray(u) < mask_prob
    if not m.any():
        m[int(pick)] = True
    return m


def collate(task, samples, bev_dim=21, txt_labels=None, mrc_masks=None):
    """mlm_collate / sap_collate / masksem_collate (tasks.py:116-163, :362-411, :672-720) over ``get_input`` dicts whose
    ``instr_encoding`` is what the task ships as ``txt_ids`` (already masked for MLM, with ``txt_labels`` the label
    lists).  Samples with ``traj_view_img_fts`` give the reference's full batch; samples without (PrefixTables.sample
    with ``panos=False``) give the by-reference host batch: no panorama tensors, ``pano_rows`` (T,) int32 instead.
    The padding and stacking is synthetic.collate's; only the text labels and the row list are added here."""
    by_ref = "traj_view_img_fts" not in samples[0]
    conv = []
    for k, s in enumerate(samples):
        c = dict(s)
        c["txt_ids"] = s["instr_encoding"]
        if by_ref:                  # zero-width stand-ins keep synthetic.collate's panorama code on its one path
            n = len(s["traj_vpids"])
            c.update(traj_view_img_fts=[np.zeros((0, 0), np.float32)] * n, traj_loc_fts=[np.zeros((0, 0), np.float32)] * n,
                     traj_nav_types=[[]] * n)
        else:
            c["traj_vp_view_lens"] = [len(x) for x in s["traj_view_img_fts"]]
        c["gmap_visited_masks"] = [bool(x) for x in s["gmap_visited_masks"]]
        if mrc_masks is not None:
            c["bev_mrc_masks"] = np.asarray(mrc_masks[k], dtype=bool)
        conv.append(c)
    cfg = types.SimpleNamespace(bev_dim=bev_dim, sem_classes=0, vocab_size=30522)
    name = task if not task.startswith("mlm") else "txt"      # MLM: the masking has been done by the caller
    b = synthetic.collate(conv, cfg, name, None)
    if task.startswith("mlm"):
        b["txt_labels"] = torch.from_numpy(synthetic._pad_stack([np.asarray(l, dtype=np.int64) for l in txt_labels], -1))
    if by_ref:
        for k in ("traj_view_img_fts", "traj_loc_fts", "traj_nav_types"):
            del b[k]
        b["pano_rows"] = torch.from_numpy(np.concatenate([s["pano_rows"] for s in samples]).astype(np.int32))
    return b


class PathBatchSource:
    """Iterate ``(task, host batch, grid keys, pano rows)``: what loader.StreamingLoader feeds to a BucketManager built
    with ``view_store=`` / ``pano_table=``.  Each batch is a lookup in the prefix tables plus the three draws; the host
    batch holds only the small tensors and the id lists StaticBatch's host side walks."""

    def __init__(self, data, tables, task_sampler, batch_size, seed, end_vp_pos_ratio=0.2, mask_prob=0.15,
                 n_batches=None, vocab_range=VOCAB_RANGE):
        """``task_sampler``: a callable ``rng -> task name`` or a sequence of task names cycled through.  Items are
        visited in shuffled epochs (a DataLoader with shuffle=True; an epoch's ragged last batch is dropped).
        ``vocab_range``: where MLM's random replacement tokens come from (tasks.py:62)."""
        self.vocab_range = tuple(vocab_range)
        self.data, self.tables, self.batch_size = data, tables, batch_size
        self.task_sampler = task_sampler
        self.rng = np.random.default_rng(seed)
        self.ratio, self.mask_prob, self.n_batches = end_vp_pos_ratio, mask_prob, n_batches

    def signature_counts(self, idxs, ends):
        """(total panoramas, widest panorama, widest map, most candidates, longest text) of a batch, from the cached
        counts alone."""
        c = np.array([self.tables.counts(int(self.tables.item_start[i]) + int(e)) for i, e in zip(idxs, ends)])
        return int(c[:, 0].sum()), int(c[:, 3].max()), int(c[:, 1].max()), int(c[:, 2].max()), \
            int(self.tables.txt_lens[idxs].max())

    def batch(self, task, idxs, ends=None):
        rng, data = self.rng, self.data
        if ends is None:
            ends = data.draw(task, idxs, rng, self.ratio)
        samples = [self.tables.sample(data, int(i), int(e), panos=False) for i, e in zip(idxs, ends)]
        labels = masks = None
        if task.startswith("mlm"):
            labels = []
            for s in samples:
                ids = s["instr_encoding"]
                s["instr_encoding"], lab = mask_tokens(rng.random(len(ids)), rng.integers(*self.vocab_range, size=len(ids)), ids)
                labels.append(lab)
        elif task.startswith("masksem"):
            n = data.bev_dim * data.bev_dim
            masks = [bev_mrc_masks(rng.random(n), self.mask_prob, rng.integers(n)) for _ in samples]
        b = collate(task, samples, data.bev_dim, txt_labels=labels, mrc_masks=masks)
        rows = b.pop("pano_rows")
        return task, b, [s["grid_key"] for s in samples], rows

    def __iter__(self):
        k, order = 0, np.zeros(0, dtype=np.int64)
        if len(self.data) < self.batch_size:
            raise ValueError("fewer items than a batch holds")
        while self.n_batches is None or k < self.n_batches:
            ts = self.task_sampler
            task = ts(self.rng) if callable(ts) else ts[k % len(ts)]
            if len(order) < self.batch_size:
                order = self.rng.permutation(len(self.data))
            idxs, order = order[:self.batch_size], order[self.batch_size:]
            yield self.batch(task, idxs)
            k += 1
