"""Fine-tune supervision on the device: DAgger expert targets, action selection, IL loss and navigation metrics
(csrc/nav_expert.hip).

The reference decides what to do with the logits of each navigation step in Python (map_nav_src/r2r/agent.py:371-417
``_teacher_action_r4r``, :529-612 feedback modes / stop rule / stop-node pick, agent_base.py:148 the IL criterion) and
scores finished trajectories with nested Python loops (r2r/env.py:309-378 ``_eval_item`` / ``eval_metrics``,
r2r/eval_utils.py ``cal_dtw`` / ``cal_cls``), with one ``.item()`` device sync per sample per step.  Here:

    ScanGraphs          host: connectivity graphs -> all-pairs shortest paths (fp64, networkx's own tie-breaking),
                        uploaded once as dist (S,N,N) f64 + pred (S,N,N) i16 tables padded to N = N_max
    expert_targets      bevbert_nav_expert      imitation / spl / ndtw targets (ndtw: wavefront DTW, one wave per cand.)
    action_step         bevbert_nav_action      softmax, stop scores, teacher / argmax / sample / expl_sample, stop rule
    il_loss             bevbert_nav_ce_fwd/bwd  CrossEntropyLoss(ignore_index=-100, reduction='sum')
    traj_append         bevbert_nav_traj_append FloydGraph.path of the agent map appended to the trajectory, scan indices
    nav_metrics         bevbert_nav_metrics     every field of _eval_item (fp64) + the eval_metrics batch means

Object grounding of the REVERIE / SOON agent (map_nav_src/reverie/agent_obj.py:384-400,516-526,597-604; reverie/env.py:360-411;
csrc/nav_obj.hip):

    object_step         bevbert_nav_obj_step    _teacher_object targets, torch.argmax's slot, the per-node 'og' record
    object_pick         bevbert_nav_obj_pick    traj[i]['pred_objid'] of the samples that just ended
    nav_metrics_obj     bevbert_nav_metrics_obj success by goal-viewpoint set, spl, rgs, rgspl (fp64) + eval_metrics' means

No call here reads anything back to the host: the caller decides when to copy the chosen nodes.
"""
import json
import os

import numpy as np
import torch

from . import lib
from .lib import call, ptr, stream

IGNOREID = -100
ERROR_MARGIN = 3.0
FEEDBACK = {"teacher": 0, "argmax": 1, "sample": 2, "expl_sample": 3}
EXPERT = {"imitation": 0, "spl": 1, "ndtw": 2}
# per-item metric columns of bevbert_nav_metrics (include/bevbert_hip.h)
METRIC_FIELDS = ("nav_error", "oracle_error", "action_steps", "trajectory_steps", "trajectory_lengths", "success",
                 "spl", "oracle_success", "DTW", "nDTW", "SDTW", "CLS")
INT_FIELDS = ("action_steps", "trajectory_steps")
# eval_metrics' averaged dict: key -> (per-item column, scale)
AVG_FIELDS = (("action_steps", "action_steps", 1.0), ("steps", "trajectory_steps", 1.0),
              ("lengths", "trajectory_lengths", 1.0), ("nav_error", "nav_error", 1.0),
              ("oracle_error", "oracle_error", 1.0), ("sr", "success", 100.0),
              ("oracle_sr", "oracle_success", 100.0), ("spl", "spl", 100.0), ("nDTW", "nDTW", 100.0),
              ("SDTW", "SDTW", 100.0), ("CLS", "CLS", 100.0))
MAX_DTW_ROWS = 1023          # prediction length bound of the ndtw expert's DTW (one LDS column per wave)


def _euclid(p, q):
    """utils/data.py:34-38, same Python float expression (pow(x, 0.5), not math.sqrt)."""
    return ((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 + (p[2] - q[2]) ** 2) ** 0.5


def _dijkstra_tree(adj, n, s):
    """networkx._dijkstra_multisource from one source with paths: a (dist, counter) heap, a node is re-queued only on a
    strictly shorter distance, neighbours in adjacency insertion order.  Returns (dist, pred) of its path tree."""
    from heapq import heappop, heappush
    dist = [float("inf")] * n
    done = [False] * n
    seen = {s: 0}
    pred = [-1] * n
    fringe = [(0, 0, s)]
    c = 1
    while fringe:
        d, _, v = heappop(fringe)
        if done[v]:
            continue
        done[v] = True
        dist[v] = d
        for u, w in adj[v]:
            vu = d + w
            if done[u]:
                continue
            if u not in seen or vu < seen[u]:
                seen[u] = vu
                heappush(fringe, (vu, c, u))
                c += 1
                pred[u] = v
    dist[s] = 0.0
    return dist, pred


class ScanGraphs:
    """Navigation graphs of a set of scans and their all-pairs shortest paths.

    ``ids[s]`` lists scan s's viewpoints in networkx's node order (first appearance in an added edge); ``index`` maps
    (scan, viewpoint id) -> that position.  ``dist[s, u, v]`` (fp64) equals ``nx.all_pairs_dijkstra_path_length`` and
    ``pred[s, u, v]`` (int16, -1 = none) is the predecessor of v on ``nx.all_pairs_dijkstra_path``'s path from u."""

    def __init__(self, scans, ids, adjacency, positions):
        self.scans = list(scans)
        self.scan_index = {s: i for i, s in enumerate(self.scans)}
        self.ids = [list(x) for x in ids]
        self.positions = [np.asarray(p, dtype=np.float64) for p in positions]
        self.adjacency = adjacency
        self.index = {(s, vp): j for s, l in zip(self.scans, self.ids) for j, vp in enumerate(l)}
        self.n_max = max(len(l) for l in self.ids)
        if self.n_max > 32767:
            raise ValueError("pred is int16: at most 32767 nodes per scan")
        S, N = len(self.scans), self.n_max
        self.dist = np.full((S, N, N), np.inf)
        self.pred = np.full((S, N, N), -1, dtype=np.int16)
        for si, adj in enumerate(adjacency):
            n = len(self.ids[si])
            for u in range(n):
                d, p = _dijkstra_tree(adj, n, u)
                self.dist[si, u, :n] = d
                self.pred[si, u, :n] = p
        self._dev = {}

    # ------------------------------------------------------------------ construction
    @staticmethod
    def _add_edge(order, adj, u, v, w):
        """nx.Graph.add_edge: new nodes appended in (u, v) order; an existing edge keeps its place, takes the new weight."""
        for x in (u, v):
            if x not in adj:
                adj[x] = {}
                order.append(x)
        adj[u][v] = w
        adj[v][u] = w

    @classmethod
    def _finish(cls, scans, per_scan):
        ids, adjs, poss = [], [], []
        for order, adj, pos in per_scan:
            k = {vp: i for i, vp in enumerate(order)}
            ids.append(order)
            adjs.append([[(k[v], w) for v, w in adj[u].items()] for u in order])
            poss.append([pos[vp] for vp in order])
        return cls(scans, ids, adjs, poss)

    @classmethod
    def from_connectivity(cls, paths):
        """utils/data.py:31-56 (load_nav_graphs): `paths` maps scan -> connectivity json file (or is a list of
        '<scan>_connectivity.json' paths).  Keeps included nodes and unobstructed edges between them."""
        if not isinstance(paths, dict):
            paths = {os.path.basename(p).split("_connectivity")[0]: p for p in paths}
        per_scan = []
        for scan, path in paths.items():
            with open(path) as f:
                data = json.load(f)
            order, adj, pos = [], {}, {}
            for i, item in enumerate(data):
                if not item["included"]:
                    continue
                for j, conn in enumerate(item["unobstructed"]):
                    if conn and data[j]["included"]:
                        p, q = item["pose"], data[j]["pose"]
                        pos[item["image_id"]] = (p[3], p[7], p[11])
                        cls._add_edge(order, adj, item["image_id"], data[j]["image_id"],
                                      _euclid((p[3], p[7], p[11]), (q[3], q[7], q[11])))
            per_scan.append((order, adj, pos))
        return cls._finish(list(paths), per_scan)

    @classmethod
    def from_edges(cls, graphs):
        """Synthetic graphs: `graphs` maps scan -> (ids, positions (n,3), edges [(i, j), ...] in insertion order);
        edges are weighted by the Euclidean distance of the positions, as from_connectivity does."""
        per_scan = []
        for scan, (ids, positions, edges) in graphs.items():
            positions = [tuple(float(c) for c in p) for p in positions]
            order, adj = [], {}
            for i, j in edges:
                cls._add_edge(order, adj, ids[i], ids[j], _euclid(positions[i], positions[j]))
            pos = {vp: positions[i] for i, vp in enumerate(ids)}
            per_scan.append((order, adj, pos))
        return cls._finish(list(graphs), per_scan)

    # ------------------------------------------------------------------ host queries
    def path(self, scan, u, v):
        """Node indices of networkx's shortest path u -> v in scan `scan` (index), from the pred table."""
        out = [v]
        p = self.pred[scan]
        while out[-1] != u:
            nxt = int(p[u, out[-1]])
            if nxt < 0:
                raise ValueError(f"no path {u} -> {v} in scan {self.scans[scan]}")
            out.append(nxt)
        return out[::-1]

    def node(self, scan, vp):
        return self.index[(scan, vp)]

    @property
    def hops(self):
        """(S, N, N) int16: edges on the shortest path u -> v (``len(shortest_paths[u][v]) - 1``), -1 where there is none.
        Built on first use from the pred table: a node is one hop further than its predecessor."""
        if getattr(self, "_hops", None) is None:
            S, N = len(self.scans), self.n_max
            h = np.full((S, N, N), -1, dtype=np.int16)
            for si, ids in enumerate(self.ids):
                k = np.arange(len(ids))
                h[si, k, k] = 0
            has = self.pred >= 0
            parent = np.where(has, self.pred, 0).astype(np.int64)
            while True:
                ph = np.take_along_axis(h, parent, axis=2)
                new = np.where(has & (ph >= 0), ph + 1, h).astype(np.int16)
                if np.array_equal(new, h):
                    break
                h = new
            self._hops = h
        return self._hops

    def to(self, device):
        """(dist, pred) on `device`, uploaded once per device."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.dist).to(device), torch.from_numpy(self.pred).to(device))
        return self._dev[key]


# ---------------------------------------------------------------------- device entry points
def _in(x, dtype, device, shape, name):
    """A read-only kernel input as a contiguous `dtype` tensor on `device` of `shape` (a no-op when it already is one):
    int64 ids (torch's default) become the int32 the kernels read, strided rows become dense."""
    if x is None:
        return None
    if torch.is_tensor(x) and x.device != device:
        raise lib.BevBertHipError(f"{name}: on {x.device}, expected {device}")
    x = torch.as_tensor(x, device=device)
    if tuple(x.shape) != tuple(shape):
        raise lib.BevBertHipError(f"{name}: shape {tuple(x.shape)}, expected {tuple(shape)}")
    return x.to(dtype).contiguous()


def _device(*xs):
    """The device of the first tensor argument (the caller's), else the current HIP device."""
    for x in xs:
        if torch.is_tensor(x):
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _inout(x, dtype, device, shape, name):
    """A tensor the kernel updates in place: it must already be a contiguous `dtype` tensor on `device` of `shape`."""
    if not (torch.is_tensor(x) and x.dtype == dtype and x.device == device and tuple(x.shape) == tuple(shape)
            and x.is_contiguous()):
        got = (x.dtype, x.device, tuple(x.shape), x.is_contiguous()) if torch.is_tensor(x) else type(x)
        raise lib.BevBertHipError(f"{name}: updated in place, needs a contiguous {dtype} {tuple(shape)} tensor on "
                                  f"{device}; got {got}")
    return x


def expert_targets(graphs, scan, cur, cand, visited, ended, gt, gt_len, t, policy, traj=None, traj_len=None, out=None):
    """`_teacher_action_r4r` for a batch (agent.py:371-417).  All tensors on the device, node ids are scan indices:
    scan/cur/ended/gt_len (B,), cand (B,C) (slot 0 = [stop], -1 = padding), visited (B,C) u8 or None, gt (B,Lg),
    traj (B,Lt) + traj_len (B,) the flattened trajectory so far (ndtw only).  policy: 'imitation' | 'spl' | 'ndtw'.
    Returns int64 (B,) targets, IGNOREID for ended samples and when every candidate is excluded."""
    dev = _device(cur, scan, cand, gt)
    dist, pred = graphs.to(dev)
    B, C = torch.as_tensor(cand).shape
    Lg = torch.as_tensor(gt).shape[1]
    i32, u8 = torch.int32, torch.uint8
    scan, cur, gt_len = (_in(x, i32, dev, (B,), n) for x, n in ((scan, "scan"), (cur, "cur"), (gt_len, "gt_len")))
    cand, gt = _in(cand, i32, dev, (B, C), "cand"), _in(gt, i32, dev, (B, Lg), "gt")
    visited, ended = _in(visited, u8, dev, (B, C), "visited"), _in(ended, u8, dev, (B,), "ended")
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=dev)
    _inout(out, torch.int64, dev, (B,), "out")
    Lt = 0
    if policy == "ndtw":
        Lt = torch.as_tensor(traj).shape[1]
        traj, traj_len = _in(traj, i32, dev, (B, Lt), "traj"), _in(traj_len, i32, dev, (B,), "traj_len")
        if Lt + graphs.n_max > MAX_DTW_ROWS:
            raise lib.BevBertHipError(f"ndtw expert: trajectory capacity {Lt} + {graphs.n_max} nodes > {MAX_DTW_ROWS}")
    else:
        traj = traj_len = None
    call("bevbert_nav_expert", ptr(dist), ptr(pred), graphs.n_max, len(graphs.scans), ptr(scan), ptr(cur), ptr(cand),
         ptr(visited), ptr(ended), ptr(gt), ptr(gt_len), Lg, ptr(traj), ptr(traj_len), Lt, B, C, int(t),
         EXPERT[policy], ptr(out), stream())
    return out


def action_step(logits, feedback, t, max_action_len, targets=None, cand=None, cur=None, goal=None, ended=None,
                no_vp_left=None, masks=None, stop_scores=None, stop_order=None, n_stop=None, expl_max_ratio=0.6,
                seed=0, outs=None):
    """One navigation step's decision (agent.py:523-534, 559-612) for B samples:

    logits (B,C) fp32 / bf16 with -inf on masked slots; cand (B,C) i32 node ids (scan indices) of the slots;
    cur / goal (B,) i32 current and goal node; ended (B,) u8 is updated in place; no_vp_left (B,) u8;
    masks (B,C) u8 = gmap_masks & ~visited (expl_sample); stop_scores (B,N) f32, stop_order (B,N) i32 and n_stop (B,) i32
    are the per-episode node_stop_scores dict (insertion order), updated in place.

    Returns a dict of device tensors: a_t (B,) int64, node (B,) i32 (the next node, -1 = the sample does not move),
    just_ended (B,) u8 (the sample stops this step: the stop rule, no_vp_left or the last step), stop_node (B,) i32 (the
    stop-node pick of just-ended samples, else -1), entropy (B,) f32, rand (B,) f32 (the uniform draw of `sample` / the
    explore draw of `expl_sample`).  `ended` is set wherever node == -1, as agent.py:615 does: a live sample whose slot
    has no viewpoint (slot 0 away from the goal in teacher / sample mode) ends in place, just_ended = 0.  Stops are
    signalled by just_ended, not by node == -1."""
    B, C = logits.shape
    dev = logits.device
    if dev.type != "cuda" or logits.dtype not in (torch.float32, torch.bfloat16):
        raise lib.BevBertHipError("action_step: fp32 / bf16 device logits only")
    N = _inout(stop_scores, torch.float32, dev, (B, stop_scores.shape[1]), "stop_scores").shape[1]
    _inout(stop_order, torch.int32, dev, (B, N), "stop_order")
    _inout(n_stop, torch.int32, dev, (B,), "n_stop")
    _inout(ended, torch.uint8, dev, (B,), "ended")
    i32, u8 = torch.int32, torch.uint8
    cand = _in(cand, i32, dev, (B, C), "cand")
    cur, goal = _in(cur, i32, dev, (B,), "cur"), _in(goal, i32, dev, (B,), "goal")
    targets = _in(targets, torch.int64, dev, (B,), "targets")
    no_vp_left, masks = _in(no_vp_left, u8, dev, (B,), "no_vp_left"), _in(masks, u8, dev, (B, C), "masks")
    if outs is not None:
        for k, dt in (("a_t", torch.int64), ("node", i32), ("just_ended", u8), ("stop_node", i32),
                      ("entropy", torch.float32), ("rand", torch.float32)):
            _inout(outs[k], dt, dev, (B,), k)
    else:
        outs = {"a_t": torch.empty(B, dtype=torch.int64, device=dev),
                "node": torch.empty(B, dtype=torch.int32, device=dev),
                "just_ended": torch.empty(B, dtype=torch.uint8, device=dev),
                "stop_node": torch.empty(B, dtype=torch.int32, device=dev),
                "entropy": torch.empty(B, dtype=torch.float32, device=dev),
                "rand": torch.empty(B, dtype=torch.float32, device=dev)}
    call("bevbert_nav_action", ptr(logits.contiguous()), lib.dtype_code(logits), B, C, FEEDBACK[feedback], int(t),
         int(max_action_len), ptr(targets), ptr(cand), ptr(cur), ptr(goal), ptr(ended), ptr(no_vp_left), ptr(masks),
         ptr(stop_scores), ptr(stop_order), ptr(n_stop), N, float(expl_max_ratio), int(seed) & 0xffffffff,
         ptr(outs["a_t"]), ptr(outs["node"]), ptr(outs["just_ended"]), ptr(outs["stop_node"]), ptr(outs["entropy"]),
         ptr(outs["rand"]), stream())
    return outs


class _NavCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        B, C = logits.shape
        logits = logits.contiguous()
        out = torch.empty(2 * B + 1, dtype=torch.float32, device=logits.device)     # [lse | row losses | sum]
        call("bevbert_nav_ce_fwd", ptr(logits), ptr(target.contiguous()), ptr(out), B, C, IGNOREID,
             lib.dtype_code(logits), stream())
        ctx.save_for_backward(logits, target, out)
        return out[2 * B]

    @staticmethod
    def backward(ctx, dloss):
        logits, target, out = ctx.saved_tensors
        B, C = logits.shape
        d = torch.empty_like(logits)
        call("bevbert_nav_ce_bwd", ptr(logits), ptr(target.contiguous()), ptr(out), ptr(dloss.contiguous().float()),
             ptr(d), B, C, IGNOREID, lib.dtype_code(logits), stream())
        return d, None


def il_loss(logits, targets):
    """nn.CrossEntropyLoss(ignore_index=-100, reduction='sum')(logits.float(), targets) (agent_base.py:148) as a 0-d
    fp32 tensor: rows summed in row order by one thread, no atomics."""
    if not (logits.is_cuda and logits.dtype in (torch.float32, torch.bfloat16)):
        raise lib.BevBertHipError("il_loss: fp32 / bf16 device logits only")
    return _NavCE.apply(logits, _in(targets, torch.int64, logits.device, (logits.shape[0],), "targets"))


def traj_append(point, node_scan, frm, to, live, traj, traj_len, n_seg, overflow):
    """traj[b] += FloydGraph.path(frm[b], to[b]) for live samples (agent.py's traj[i]['path'].append(gmap.graph.path(...)),
    the path DeviceGraphMap.path returns) in scan indices, on the device.  point (B,Nm,Nm) i32: the agent map's next-hop
    table (DeviceGraphMap.t['point']); node_scan (B,Nm) i32: scan index of each map node (registration order, gm.names
    through ScanGraphs.index); frm / to (B,) map nodes; live (B,) u8.  traj (B,Lt), traj_len (B,), n_seg (B,) (number of
    appended segments = len(pred_path) - 1 once the start is counted) and overflow (1,) i32 are updated in place;
    read overflow once per episode."""
    dev = _device(point, traj)
    point = torch.as_tensor(point, device=dev)
    B, Nm = point.shape[0], point.shape[1]
    i32 = torch.int32
    point = _in(point, i32, dev, (B, Nm, Nm), "point")
    node_scan = _in(node_scan, i32, dev, (B, Nm), "node_scan")
    frm, to, live = _in(frm, i32, dev, (B,), "from"), _in(to, i32, dev, (B,), "to"), _in(live, torch.uint8, dev, (B,), "live")
    Lt = traj.shape[1]
    for x, shp, n in ((traj, (B, Lt), "traj"), (traj_len, (B,), "traj_len"), (n_seg, (B,), "n_seg"),
                      (overflow, (1,), "overflow")):
        _inout(x, i32, dev, shp, n)
    call("bevbert_nav_traj_append", ptr(point), Nm, ptr(node_scan), ptr(frm), ptr(to), ptr(live), ptr(traj),
         ptr(traj_len), Lt, ptr(n_seg), ptr(overflow), B, stream())


def nav_metrics(graphs, scan, path, path_len, action_steps, gt, gt_len):
    """`_eval_item` of B finished trajectories + eval_metrics' averages, in fp64 on the device.

    scan (B,) i32, path (B,Lp) i32 the flattened trajectory (sum(pred_path, [])) in scan indices, path_len (B,) i32,
    action_steps (B,) i32 = len(pred_path) - 1, gt (B,Lg) i32, gt_len (B,) i32.
    Returns (items (B, 12) f64 in METRIC_FIELDS order, avg (11,) f64 in AVG_FIELDS order)."""
    dev = _device(scan, path, gt, path_len)
    dist, _ = graphs.to(dev)
    B = torch.as_tensor(scan).shape[0]
    Lp, Lg = torch.as_tensor(path).shape[1], torch.as_tensor(gt).shape[1]
    i32 = torch.int32
    scan, path_len, action_steps, gt_len = (_in(x, i32, dev, (B,), n) for x, n in (
        (scan, "scan"), (path_len, "path_len"), (action_steps, "action_steps"), (gt_len, "gt_len")))
    path, gt = _in(path, i32, dev, (B, Lp), "path"), _in(gt, i32, dev, (B, Lg), "gt")
    items = torch.empty(B, len(METRIC_FIELDS), dtype=torch.float64, device=dev)
    avg = torch.empty(len(AVG_FIELDS), dtype=torch.float64, device=dev)
    call("bevbert_nav_metrics", ptr(dist), graphs.n_max, len(graphs.scans), ptr(scan), ptr(path), ptr(path_len),
         Lp, ptr(action_steps), ptr(gt), ptr(gt_len), Lg, B, ERROR_MARGIN, ptr(items), ptr(avg), stream())
    return items, avg


def metrics_dicts(items, avg):
    """(per-item dict of lists, averaged dict) in the reference's eval_metrics format from nav_metrics' tensors."""
    it = items.cpu().numpy()
    per = {k: [int(v) if k in INT_FIELDS else float(v) for v in it[:, i]] for i, k in enumerate(METRIC_FIELDS)}
    av = avg.cpu().numpy()
    return {k: float(av[i]) for i, (k, _, _) in enumerate(AVG_FIELDS)}, per


# ---------------------------------------------------------------------- object grounding (REVERIE / SOON), csrc/nav_obj.hip
# per-item metric columns of bevbert_nav_metrics_obj, in the order reverie/env.py:_eval_item fills `scores`
METRIC_FIELDS_OBJ = ("action_steps", "trajectory_steps", "trajectory_lengths", "success", "oracle_success", "spl", "rgs",
                     "rgspl")
# reverie/env.py eval_metrics' averaged dict: key -> (per-item column, scale)
AVG_FIELDS_OBJ = (("action_steps", "action_steps", 1.0), ("steps", "trajectory_steps", 1.0),
                  ("lengths", "trajectory_lengths", 1.0), ("sr", "success", 100.0), ("oracle_sr", "oracle_success", 100.0),
                  ("spl", "spl", 100.0), ("rgs", "rgs", 100.0), ("rgspl", "rgspl", 100.0))


def object_step(obj_logits, obj_ids, obj_lens, gt_obj, cur, end_vps, n_end, ended, stop_og, outs=None):
    """`_teacher_object` and the 'og' record of one navigation step (reverie/agent_obj.py:384-400, 516-526) for B samples;
    call it BEFORE action_step of the same step (it reads the pre-action `ended`).

    obj_logits (B,O) fp32 / bf16 with -inf on masked slots; obj_ids (B,O) i32 the caller's integer object ids; obj_lens (B);
    gt_obj (B) i32; cur (B) i32 current node; end_vps (B,E) i32 + n_end (B) i32 the gt_end_vps set; ended (B) u8;
    stop_og (B,N) i32, indexed like stop_scores, is updated in place: a live sample records the id of its arg-max object
    (-1 = None: no objects) under its current node, a revisit overwrites.

    Returns a dict of device tensors: targets (B,) int64 for ``il_loss(obj_logits, targets)`` (IGNOREID when ended, off
    the goal set, or the target is not among the objects), og_slot (B,) i32 = torch.argmax of the valid slots (-1: none)."""
    B, O = obj_logits.shape
    dev = obj_logits.device
    if dev.type != "cuda" or obj_logits.dtype not in (torch.float32, torch.bfloat16):
        raise lib.BevBertHipError("object_step: fp32 / bf16 device logits only")
    i32, u8 = torch.int32, torch.uint8
    N = _inout(stop_og, i32, dev, (B, stop_og.shape[1]), "stop_og").shape[1]
    E = torch.as_tensor(end_vps).shape[1]
    obj_ids, end_vps = _in(obj_ids, i32, dev, (B, O), "obj_ids"), _in(end_vps, i32, dev, (B, E), "end_vps")
    obj_lens = _in(obj_lens, torch.int64, dev, (B,), "obj_lens")
    gt_obj, cur, n_end = (_in(x, i32, dev, (B,), n) for x, n in ((gt_obj, "gt_obj"), (cur, "cur"), (n_end, "n_end")))
    ended = _in(ended, u8, dev, (B,), "ended")
    if outs is not None:
        _inout(outs["targets"], torch.int64, dev, (B,), "targets")
        _inout(outs["og_slot"], i32, dev, (B,), "og_slot")
    else:
        outs = {"targets": torch.empty(B, dtype=torch.int64, device=dev), "og_slot": torch.empty(B, dtype=i32, device=dev)}
    call("bevbert_nav_obj_step", ptr(obj_logits.contiguous()), lib.dtype_code(obj_logits), B, O, ptr(obj_ids), ptr(obj_lens),
         ptr(gt_obj), ptr(cur), ptr(end_vps), ptr(n_end), E, ptr(ended), ptr(stop_og), N, ptr(outs["targets"]),
         ptr(outs["og_slot"]), stream())
    return outs


def object_pick(just_ended, stop_node, stop_og, pred_obj):
    """traj[i]['pred_objid'] of the samples that stop this step (reverie/agent_obj.py:597-604); call it AFTER action_step
    with its just_ended / stop_node (B,).  pred_obj (B,) i32 is persistent and updated in place: a just-ended sample gets
    the 'og' record of its stop node (-1 = None), the other rows keep their value.  Returns pred_obj."""
    dev = _device(pred_obj, stop_og)
    B = pred_obj.shape[0]
    N = _inout(stop_og, torch.int32, dev, (B, stop_og.shape[1]), "stop_og").shape[1]
    _inout(pred_obj, torch.int32, dev, (B,), "pred_obj")
    just_ended = _in(just_ended, torch.uint8, dev, (B,), "just_ended")
    stop_node = _in(stop_node, torch.int32, dev, (B,), "stop_node")
    call("bevbert_nav_obj_pick", ptr(just_ended), ptr(stop_node), ptr(stop_og), N, ptr(pred_obj), B, stream())
    return pred_obj


def nav_metrics_obj(graphs, scan, path, path_len, action_steps, gt, gt_len, goal_vps, n_goal, pred_obj, gt_obj):
    """reverie/env.py `_eval_item` of B finished trajectories + eval_metrics' averages, in fp64 on the device.

    scan, path (B,Lp), path_len, action_steps, gt (B,Lg), gt_len as in nav_metrics; goal_vps (B,E) i32 + n_goal (B) i32 the
    viewpoints the target object is visible from (scan indices); pred_obj / gt_obj (B) i32 (-1 = no prediction).
    Returns (items (B, 8) f64 in METRIC_FIELDS_OBJ order, avg (8,) f64 in AVG_FIELDS_OBJ order)."""
    dev = _device(scan, path, gt, path_len)
    dist, _ = graphs.to(dev)
    B = torch.as_tensor(scan).shape[0]
    Lp, Lg, E = (torch.as_tensor(x).shape[1] for x in (path, gt, goal_vps))
    i32 = torch.int32
    scan, path_len, action_steps, gt_len, n_goal, pred_obj, gt_obj = (_in(x, i32, dev, (B,), n) for x, n in (
        (scan, "scan"), (path_len, "path_len"), (action_steps, "action_steps"), (gt_len, "gt_len"), (n_goal, "n_goal"),
        (pred_obj, "pred_obj"), (gt_obj, "gt_obj")))
    path, gt, goal_vps = _in(path, i32, dev, (B, Lp), "path"), _in(gt, i32, dev, (B, Lg), "gt"), \
        _in(goal_vps, i32, dev, (B, E), "goal_vps")
    items = torch.empty(B, len(METRIC_FIELDS_OBJ), dtype=torch.float64, device=dev)
    avg = torch.empty(len(AVG_FIELDS_OBJ), dtype=torch.float64, device=dev)
    call("bevbert_nav_metrics_obj", ptr(dist), graphs.n_max, len(graphs.scans), ptr(scan), ptr(path), ptr(path_len), Lp,
         ptr(action_steps), ptr(gt), ptr(gt_len), Lg, ptr(goal_vps), ptr(n_goal), E, ptr(pred_obj), ptr(gt_obj), B,
         ptr(items), ptr(avg), stream())
    return items, avg


def metrics_dicts_obj(items, avg):
    """(averaged dict, per-item dict of lists) in reverie/env.py eval_metrics' format from nav_metrics_obj's tensors."""
    it = items.cpu().numpy()
    per = {k: [int(v) if k in INT_FIELDS else (bool(v) if k == "rgs" else float(v)) for v in it[:, i]]
           for i, k in enumerate(METRIC_FIELDS_OBJ)}
    av = avg.cpu().numpy()
    return {k: float(av[i]) for i, (k, _, _) in enumerate(AVG_FIELDS_OBJ)}, per
