"""Device-side ghost-node map of the continuous-environment (CE) agent (csrc/ce_map.hip).

Between ``waypoint.waypoint_step`` and ``GlocalTextPathNavCMT.forward_navigation_per_step`` the reference keeps one
``GraphMap`` per environment in Python (bevbert_ce/vlnce_baselines/models/graph_utils.py:142-372) and builds the step's
inputs in loops over the batch (ss_trainer_BEV.py:477-611,1035-1179): two networkx all-pairs Dijkstra runs per
environment and step, dictionaries of lists, a ``.item()`` per environment.  In the CE map node ids are plain integers
(``identify_node`` names the k-th node ``str(k)``, ghosts are ``g0, g1, ...``), so unlike the discrete agent's map
(graph_map_dev.py) no host dictionary is needed: ``CEGraphMap`` keeps B maps in dense device arrays of fixed capacity
and every per-step method is a fixed sequence of launches with fixed output shapes -- the step can be captured in one
hipGraph together with the waypoint stage and the navigation forward.

    update               identify_node + estimate_cand_pos + update_graph          -> bevbert_ce_update
    nav_gmap_variable    _nav_gmap_variable + get_pos_fts + front_to_ghost_dist    -> bevbert_ce_nav_vars
    remember_pano        update_node_pc (the inputs of lift, stored per node)      -> bevbert_ce_remember
    bev_inputs           gather_node_pc + lift + splat, get_neighbors,             -> bevbert_ce_bev_select, bev_lift_bin,
                         _discretize_polar_relpos (+ SAP fusion indices)              bev_splat_mean, bevbert_ce_bev_cands
    record_stop_scores / teacher_index / act                                       -> bevbert_ce_stop_scores / _teacher / _act
    to_reference         one D2H copy -> the reference's list of action dicts

Ids in every output: -1 = [stop] / none, k < N = node k (the reference's ``str(k)``), N + g = ghost g (``'g' + str(g)``).
The only host input of a step is one packed pinned transfer (``stage``): positions, headings, the live mask, the
step id and the matrices of lift / splat.  Turning Habitat's quaternion into a heading stays with the caller, and so do the Habitat calls of training
(``cand_real_pos``: ``update`` returns ``cand_slot`` so that a caller can keep them next to the simulator).
``remember_pano`` keeps every node's panorama grids, depths and camera matrices in a device store and ``bev_inputs``
lifts and splats the chosen nodes from it with the existing ``ops.bev_lift_bin`` / ``ops.bev_splat_mean(rows=...)``.
"""
import ctypes

import numpy as np
import torch

from . import lib
from . import ops
from .pretrain_cmt import bevpos_polar
from .synthetic import pose_matrix

_CeState = lib.struct("bevbert_ce_state")
_PTRS = tuple(n for n, ct in _CeState._fields_ if ct is ctypes.c_void_p)      # the device arrays, in the struct's order


class CEGraphMap:
    """B ghost-node maps on the device.  ``merge_ghost``: one flag or one per map (MODEL.merge_ghost); ``ghost_aug``:
    IL.ghost_aug in training, 0 otherwise; ``seed`` keys its draws.  Capacities are fixed: ``node_capacity`` N steps per
    episode (<= 64), ``ghost_capacity`` Gh ghost ids per episode (default 5 N: five candidates a step),
    ``front_capacity`` observations merged into one ghost, ``cand_capacity`` BEV candidates besides the current node.
    Exceeding one refuses the item and raises the flag ``check_overflow`` reads; nothing is truncated silently."""

    def __init__(self, batch_size, hidden_size, device, dtype=torch.float32, loc_noise=0.5, merge_ghost=True, ghost_aug=0.0,
                 seed=0, node_capacity=16, ghost_capacity=None, front_capacity=16, cand_capacity=15, bev_dim=11,
                 bev_res=1.0):
        device = torch.device(device)
        if device.type != "cuda":
            raise lib.BevBertHipError("CEGraphMap keeps the maps in device memory: it needs the MI355X")
        B, N, H = int(batch_size), int(node_capacity), int(hidden_size)
        Gh = 5 * N if ghost_capacity is None else int(ghost_capacity)
        if not (1 <= N <= 64 and Gh >= 1 and 1 + N + Gh <= 512):
            raise ValueError(f"CEGraphMap: node_capacity {N} (1..64), 1 + N + ghost_capacity = {1 + N + Gh} (<= 512)")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("CEGraphMap: embeddings are float32 or bfloat16")
        self.B, self.N, self.Gh, self.P, self.H, self.K = B, N, Gh, int(front_capacity), H, 1 + int(cand_capacity)
        self.G = 1 + N + Gh
        self.device, self.dtype = device, dtype
        self.loc_noise, self.ghost_aug, self.seed = float(loc_noise), float(ghost_aug), int(seed) & 0xFFFFFFFF
        self.bev_dim, self.bev_res = int(bev_dim), float(bev_res)
        mg = np.full(B, bool(merge_ghost), dtype=np.uint8) if np.ndim(merge_ghost) == 0 else \
            np.asarray(merge_ghost, dtype=bool).astype(np.uint8).reshape(B)

        def z(shape, dt):
            return torch.zeros(shape, dtype=dt, device=device)
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        self.t = {
            "node_pos": z((B, N, 3), f64), "edge_w": torch.full((B, N, N), -1.0, dtype=f64, device=device),
            "dist": torch.full((B, N, N), float("inf"), dtype=f64, device=device), "hops": z((B, N, N), i32),
            "pred": torch.full((B, N, N), -1, dtype=i32, device=device), "n_nodes": z((B,), i32),
            "node_step": z((B, N), i32), "stop_score": z((B, N), torch.float32), "node_embeds": z((B, N, H), dtype),
            "g_cnt": z((B,), i32), "g_alive": z((B, Gh), u8), "g_npos": z((B, Gh), i32), "g_pos": z((B, Gh, self.P, 3), f64),
            "g_mean": z((B, Gh, 3), f64), "g_aug": z((B, Gh, 3), f64), "g_sum": z((B, Gh, H), torch.float32),
            "g_fronts": z((B, Gh, self.P), i32), "prev_vp": torch.full((B,), -1, dtype=i32, device=device),
            "cur_vp": z((B,), i32), "merge": torch.from_numpy(mg).to(device), "overflow": z((1,), i32),
        }
        st = _CeState()
        for k in _PTRS:
            setattr(st, k, self.t[k].data_ptr())
        st.B, st.N, st.Gh, st.P, st.H, st.dtype = B, N, Gh, self.P, H, lib.dtype_code(dtype)
        self.state, self._st = st, ctypes.addressof(st)
        # the step's packed host input: [pose (B,4) f64 | step_id i32 (8 bytes) | live (B) u8 | T_c2w (B,V,16) f32 |
        # T_w2c (B,16) f32 | S (B,3) f32]; two pinned buffers take turns, so packing a step never waits for the last copy
        V = self.V = 12
        self._o_live = B * 32 + 8
        self._o_c2w = self._o_live + (B + 15) // 16 * 16
        self._o_w2c = self._o_c2w + B * V * 64
        self._o_S = self._o_w2c + B * 64
        self._nb = self._o_S + (B * 12 + 15) // 16 * 16
        self._pins = [torch.zeros(self._nb, dtype=u8).pin_memory() for _ in range(2)]
        self._hosts = [p.numpy() for p in self._pins]
        self._evs = [None, None]
        self._slot = 0
        self._feed = z((self._nb,), u8)
        base = self._feed.data_ptr()
        self._pose, self._step, self._live = base, base + B * 32, base + self._o_live
        self.T_c2w = self._feed[self._o_c2w:self._o_w2c].view(torch.float32).view(B, V, 4, 4)
        self.T_w2c = self._feed[self._o_w2c:self._o_S].view(torch.float32).view(B, 4, 4)
        self.S_w2c = self._feed[self._o_S:self._o_S + B * 12].view(torch.float32).view(B, 3)
        self.store = None                  # remember_pano allocates it on first use (per-episode, B * N slots)
        self._pix = None
        self._bev_pos = bevpos_polar(self.bev_dim, device)
        self._gmap_ids = None

    def reset(self):
        """Empty every map for the next batch of episodes (fills on the current stream; the overflow flag is kept)."""
        t = self.t
        for k in ("n_nodes", "g_cnt", "g_alive", "g_npos", "cur_vp", "hops", "stop_score"):
            t[k].zero_()
        t["edge_w"].fill_(-1.0)
        t["dist"].fill_(float("inf"))
        t["pred"].fill_(-1)
        t["prev_vp"].fill_(-1)
        self._gmap_ids = None

    live = property(lambda self: self._feed[self._o_live:self._o_live + self.B])

    # -- the one host input of a step ----------------------------------------------------------------------------------
    def stage(self, step_id, cur_pos, heading, live=None, copy=True):
        """Pack the step's host input into a pinned buffer and ship it with ONE non-blocking copy on the current
        stream: cur_pos (B,3), heading (B) (float64, the reference's Python floats), the live mask (B), step_id, and the
        matrices of lift / splat computed with the numpy twin of transfrom3D exactly as ss_trainer_BEV.py:391-400,420-429
        do: 12 camera-to-world matrices (x, y, z, heading - k * 30 deg, elevation pi), the world-to-ego matrix (heading
        -h) and the shift (the position in float32).
        Two pinned buffers alternate and each is guarded by an event recorded behind its copy, so a call waits only if
        the copy of the step BEFORE the last one is still pending -- in a rollout, never; it is an event wait on a
        copy, not a device synchronisation.  ``copy=False`` rewrites the buffer a captured step copies from, for a
        replay: that one address is fixed in the graph, so the call has to wait until the previous replay has read it
        (follow every replay with ``mark_replayed()``)."""
        B, V = self.B, self.V
        capturing = torch.cuda.is_current_stream_capturing()
        if copy:
            self._slot ^= 1
        k = self._slot
        if self._evs[k] is not None and not capturing:
            self._evs[k].synchronize()
        host = self._hosts[k]
        pos = np.asarray(cur_pos, dtype=np.float64).reshape(B, 3)
        hd = np.asarray(heading, dtype=np.float64).reshape(B)
        pose = host[:B * 32].view(np.float64).reshape(B, 4)
        pose[:, :3], pose[:, 3] = pos, hd
        host[B * 32:B * 32 + 4].view(np.int32)[0] = int(step_id)
        host[self._o_live:self._o_live + B] = 1 if live is None else np.asarray(live, dtype=bool).astype(np.uint8)
        xyzhe = np.zeros((B * (V + 1), 5))
        views = xyzhe[:B * V].reshape(B, V, 5)
        views[:, :, :3] = pos[:, None]
        views[:, :, 3] = -np.arange(V)[None] * np.radians(30) + hd[:, None]
        views[:, :, 4] = np.pi
        xyzhe[B * V:, 3] = -hd
        T = pose_matrix(xyzhe)
        host[self._o_c2w:self._o_w2c] = T[:B * V].reshape(-1).view(np.uint8)
        host[self._o_w2c:self._o_S] = T[B * V:].reshape(-1).view(np.uint8)
        host[self._o_S:self._o_S + B * 12] = pos.astype(np.float32).reshape(-1).view(np.uint8)
        if copy:
            self._feed.copy_(self._pins[k], non_blocking=True)
            if not capturing:
                self.mark_replayed()

    def mark_replayed(self):
        """Record, on the current stream, that everything queued so far has read the current pinned buffer."""
        if self._evs[self._slot] is None:
            self._evs[self._slot] = torch.cuda.Event()
        self._evs[self._slot].record(torch.cuda.current_stream(self.device))

    # -- per-step methods: launches only ------------------------------------------------------------------------------
    def update(self, step_id, cand_count, cand_angles, cand_distances, avg_pano_embeds, pano_embeds, nav_types,
               cur_pos=None, heading=None, live=None):
        """identify_node + estimate_cand_pos + update_graph for every live map (graph_utils.py:182-262).  The candidate
        tensors are waypoint_step's own device outputs (cand_count (B) i32, cand_angles / cand_distances (B,C) f32),
        avg_pano_embeds (B,H) and pano_embeds (B,L,H) the panorama encoder's, nav_types (B,L) i64 the encoder's input:
        candidate j takes the j-th row whose type is 1.  Embeddings enter as constants (``ce_train.CEMapTape`` wraps this
        call and ``nav_gmap_variable`` for training: it carries the gradient of ``gmap_img_fts`` back to them).  ``cur_pos`` / ``heading`` /
        ``live`` given: ``stage`` is called first with ``step_id``; otherwise the staged values are used as they are.  Returns cand_slot (B,C) i32: the id each candidate went to."""
        if cur_pos is not None:
            self.stage(step_id, cur_pos, heading, live)
        B, C = cand_angles.shape
        if B != self.B or pano_embeds.dim() != 3 or tuple(pano_embeds.shape[::2]) != (B, self.H) or \
                tuple(nav_types.shape) != tuple(pano_embeds.shape[:2]) or tuple(avg_pano_embeds.shape) != (B, self.H) or \
                tuple(cand_distances.shape) != (B, C) or tuple(cand_count.shape) != (B,):
            raise ValueError("CEGraphMap.update: cand_count (B), cand_angles / cand_distances (B,C), avg_pano_embeds (B,H), "
                             "pano_embeds (B,L,H), nav_types (B,L)")
        if cand_count.dtype != torch.int32 or cand_angles.dtype != torch.float32 or cand_distances.dtype != torch.float32 or \
                nav_types.dtype != torch.int64:
            raise ValueError("CEGraphMap.update: cand_count int32, cand_angles / cand_distances float32, nav_types int64")
        avg = avg_pano_embeds.detach().to(self.dtype).contiguous()
        pano = pano_embeds.detach().to(self.dtype).contiguous()
        slot = torch.empty(B, C, dtype=torch.int32, device=self.device)
        lib.call("bevbert_ce_update", self._st, self._pose, self._live, self._step, lib.ptr(cand_count.contiguous()),
                 lib.ptr(cand_angles.contiguous()), lib.ptr(cand_distances.contiguous()), C, lib.ptr(avg), lib.ptr(pano),
                 lib.ptr(nav_types.contiguous()), pano.shape[1], self.loc_noise, self.ghost_aug, self.seed, lib.ptr(slot),
                 lib.stream())
        return slot

    def nav_gmap_variable(self):
        """_nav_gmap_variable (ss_trainer_BEV.py:534-611) padded to G = 1 + N + Gh rows with a prefix mask: [stop], the
        nodes in creation order, the live ghosts in creation order.  gmap_ids (B,G) i64 replaces the id lists."""
        B, G, dev = self.B, self.G, self.device
        o = {"gmap_ids": torch.empty(B, G, dtype=torch.int64, device=dev),
             "gmap_step_ids": torch.empty(B, G, dtype=torch.int64, device=dev),
             "gmap_visited_masks": torch.empty(B, G, dtype=torch.bool, device=dev),
             "gmap_masks": torch.empty(B, G, dtype=torch.bool, device=dev),
             "gmap_img_fts": torch.empty(B, G, self.H, dtype=self.dtype, device=dev),
             "gmap_pos_fts": torch.empty(B, G, 7, dtype=torch.float32, device=dev),
             "gmap_pair_dists": torch.empty(B, G, G, dtype=torch.float32, device=dev),
             "no_vp_left": torch.empty(B, dtype=torch.bool, device=dev)}
        lib.call("bevbert_ce_nav_vars", self._st, self._pose, self._live, *(lib.ptr(o[k]) for k in (
            "gmap_ids", "gmap_step_ids", "gmap_visited_masks", "gmap_masks", "gmap_img_fts", "gmap_pos_fts",
            "gmap_pair_dists", "no_vp_left")), lib.stream())
        self._gmap_ids = o["gmap_ids"]
        return o

    def remember_pano(self, rgb_grid, depth_grid):
        """GraphMap.update_node_pc for every live map (ss_trainer_BEV.py:1047,1067), kept as the INPUTS of lift: the
        step's grid features rgb_grid (B,12,196,C), depths depth_grid (B,12,14,14) (metres / 10, as the depth sensor
        hands them over) and the staged camera-to-world matrices go into slot b * N + cur of a device-resident,
        per-episode store (allocated on first use; a slot is always rewritten before a new episode can select it).
        bev_inputs lifts from it."""
        B, V, N = self.B, self.V, self.N
        if rgb_grid.dim() != 4 or tuple(rgb_grid.shape[:2]) != (B, V) or depth_grid.numel() != B * V * rgb_grid.shape[2]:
            raise ValueError("remember_pano: rgb_grid (B,12,hw*hw,C), depth_grid (B,12,hw,hw)")
        if rgb_grid.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("remember_pano: grid features are float32, bfloat16 or float16")
        P0, C = V * rgb_grid.shape[2], rgb_grid.shape[3]
        hw = int(round(rgb_grid.shape[2] ** 0.5))
        if hw * hw != rgb_grid.shape[2] or (C * rgb_grid.element_size()) % 4:
            raise ValueError("remember_pano: a square grid and a channel row of whole 4-byte words expected")
        st = self.store
        if st is None or st["rgb"].shape[1:] != (P0, C) or st["rgb"].dtype != rgb_grid.dtype:
            dev = self.device
            st = self.store = {"rgb": torch.zeros(B * N, P0, C, dtype=rgb_grid.dtype, device=dev),
                               "depth": torch.zeros(B * N, V, hw, hw, dtype=torch.float32, device=dev),
                               "T": torch.zeros(B * N, V, 4, 4, dtype=torch.float32, device=dev)}
            self._pix = ops.pixel_scale(hw, dev)
        rgb = rgb_grid.detach().contiguous()
        dep = depth_grid.detach().reshape(B, V, hw, hw).float().contiguous()
        for src, dst in ((rgb, st["rgb"]), (dep, st["depth"]), (self.T_c2w, st["T"])):
            lib.call("bevbert_ce_remember", self._st, self._live, lib.ptr(src), lib.ptr(dst),
                     src[0].numel() * src.element_size(), lib.stream())

    def bev_inputs(self, order=1):
        """_nav_bev_variable (ss_trainer_BEV.py:477-532).
        bev_fts (after ``remember_pano``): the nodes are chosen as ``gather_node_pc(cur, order)`` is WRITTEN --
        ``len(shortest_path[cur][node]) <= order``, and a path counts both its end points, so the trainer's ``order=1``
        selects the current node only (its own panorama; the visited 1-hop neighbours need ``order=2``).  ``order`` is
        kept general: up to R = 1 (order <= 1) or min(N, 10) (the lift kernel takes 24 576 points) nodes in creation
        order, more raise the overflow flag.  Their stored depths and matrices are gathered, lifted and binned by
        ``ops.bev_lift_bin`` with the staged world-to-ego matrix and shift, and ``ops.bev_splat_mean(rows=...)`` reads the
        stored grid features in place.  bev_masks is all ones (ss_trainer_BEV.py:457-458).
        Candidates: get_neighbors (the current node, its 1-hop nodes, the ghosts it fronts), their cells by
        _discretize_polar_relpos, the navigable mask, bev_pos_fts (the start node's position features next to
        bevpos_polar) and -- from the integer ids, on the device -- the (src, vis_c) pair ``fuse_sap_logits`` takes.
        bev_cand_idxs / bev_cand_ids are (B, 1 + Cn), Cn = cand_capacity (padding 0 / -1, bev_cand_count real slots)."""
        B, K, dev, cells = self.B, self.K, self.device, self.bev_dim * self.bev_dim
        o = {"bev_nav_masks": torch.empty(B, cells, dtype=torch.bool, device=dev),
             "bev_cand_idxs": torch.empty(B, K, dtype=torch.int64, device=dev),
             "bev_cand_ids": torch.empty(B, K, dtype=torch.int64, device=dev),
             "bev_cand_count": torch.empty(B, dtype=torch.int32, device=dev),
             "bev_gpos_fts": torch.empty(B, 7, dtype=torch.float32, device=dev),
             "src": torch.empty(B, self.G, dtype=torch.int64, device=dev),
             "vis_c": torch.empty(B, K, dtype=torch.bool, device=dev)}
        lib.call("bevbert_ce_bev_cands", self._st, self._pose, self._live, self.bev_dim, self.bev_res, K, *(lib.ptr(o[k]) for k in (
            "bev_nav_masks", "bev_cand_idxs", "bev_cand_ids", "bev_cand_count", "bev_gpos_fts", "src", "vis_c")), lib.stream())
        o["bev_masks"] = torch.ones(B, cells, dtype=torch.bool, device=dev)
        o["bev_pos_fts"] = torch.cat([o["bev_gpos_fts"][:, None].expand(-1, cells, -1), self._bev_pos[None].expand(B, -1, -1)], 2)
        if self.store is not None:
            st, V = self.store, self.V
            R = 1 if order <= 1 else min(self.N, 10)
            rows = torch.empty(B, R, dtype=torch.int32, device=dev)
            row_live = torch.empty(B, R, dtype=torch.bool, device=dev)
            lib.call("bevbert_ce_bev_select", self._st, self._live, int(order), R, lib.ptr(rows), lib.ptr(row_live), lib.stream())
            hw = st["depth"].shape[-1]
            depths = torch.empty(B, R * V, hw, hw, dtype=torch.float32, device=dev)
            T_c2w = torch.empty(B, R * V, 4, 4, dtype=torch.float32, device=dev)
            for src, dst in ((st["depth"], depths), (st["T"], T_c2w)):          # padding slots: no depth
                lib.call("bevbert_gm_gather_views", lib.ptr(src), lib.ptr(rows), lib.ptr(row_live), lib.ptr(dst), B * R,
                         src[0].numel() * 4, lib.stream())
            _, order_, start = ops.bev_lift_bin(depths, T_c2w, self.T_w2c, self.S_w2c, self._pix, self.bev_dim, self.bev_res)
            o["bev_fts"], _, _ = ops.bev_splat_mean(st["rgb"], order_, start, cells, rows=rows)
            o["grid_rows"], o["grid_rows_live"] = rows, row_live
        return o

    def record_stop_scores(self, probs0):
        """gmap.node_stop_scores[cur_vp] = nav_probs[i, 0] (ss_trainer_BEV.py:1083-1084); probs0 (B) f32, any stride."""
        if probs0.dtype != torch.float32 or probs0.dim() != 1 or probs0.shape[0] != self.B:
            raise ValueError("record_stop_scores: (B) float32 expected")
        lib.call("bevbert_ce_stop_scores", self._st, self._live, lib.ptr(probs0), probs0.stride(0), lib.stream())

    def teacher_index(self, cur_dist_to_goal, ghost_goal_dist):
        """_teacher_action_new with the 'spl' expert (ss_trainer_BEV.py:317-334) from distances the caller measured:
        cur_dist_to_goal (B) f64, ghost_goal_dist (B,Gh) f64 indexed by ghost id.  (B) i64: 0 within 1.5 m of the goal,
        -100 when no ghost is left, else the gmap row of the first nearest live ghost."""
        if tuple(cur_dist_to_goal.shape) != (self.B,) or tuple(ghost_goal_dist.shape) != (self.B, self.Gh):
            raise ValueError("teacher_index: cur_dist_to_goal (B), ghost_goal_dist (B, ghost_capacity)")
        out = torch.empty(self.B, dtype=torch.int64, device=self.device)
        lib.call("bevbert_ce_teacher", self._st, self._live, lib.ptr(cur_dist_to_goal.double().contiguous()),
                 lib.ptr(ghost_goal_dist.double().contiguous()), lib.ptr(out), lib.stream())
        return out

    def act(self, a_t, last_step=False, consume_ghost=True, gmap_ids=None):
        """ss_trainer_BEV.py:1110-1179: the stop rule, the stop node, ghost and nearest front, back_path, prev_vp = front,
        ghost deletion.  a_t (B) i64 rows of the last nav_gmap_variable's listing.  Returns the device record (B, 11 + 4 N)
        f64 that ``to_reference`` reads."""
        ids = self._gmap_ids if gmap_ids is None else gmap_ids
        if ids is None:
            raise lib.BevBertHipError("CEGraphMap.act: call nav_gmap_variable first (a_t indexes its listing)")
        if a_t.dtype != torch.int64 or tuple(a_t.shape) != (self.B,) or tuple(ids.shape) != (self.B, self.G):
            raise ValueError("CEGraphMap.act: a_t (B) int64, gmap_ids (B,G) int64")
        rec = torch.empty(self.B, 11 + 4 * self.N, dtype=torch.float64, device=self.device)
        lib.call("bevbert_ce_act", self._st, self._live, lib.ptr(a_t.contiguous()), lib.ptr(ids), int(bool(last_step)),
                 int(bool(consume_ghost)), lib.ptr(rec), lib.stream())
        return rec

    # -- the places that synchronise -----------------------------------------------------------------------------------
    def to_reference(self, rec, back_algo="control", tryout=False):
        """The reference's list of 'action' dicts from an ``act`` record, with ONE device-to-host copy (ids as the
        reference's strings; None for a map that is not live).  ``vis_info`` is None: the reference fills it for stop
        actions (all node and ghost positions, ss_trainer_BEV.py:1122-1126) for its video option only, which is not
        built; the positions are in ``t["node_pos"]`` / ``t["g_aug"]`` for a caller that draws."""
        N = self.N
        out = []
        for r in rec.cpu().numpy():
            act, cur, tgt, ghost, n = (int(x) for x in r[:5])
            if act < 0:
                out.append(None)
                continue
            path = [int(v) for v in r[5:5 + n]]
            ppos = r[11 + N:11 + 4 * N].reshape(N, 3)
            back = [(str(v), ppos[i].copy()) for i, v in enumerate(path)] if back_algo == "control" else None
            a = {"act": act, "cur_vp": str(cur), "back_path": back, "tryout": tryout}
            if act == 0:
                a.update(stop_vp=str(tgt), stop_pos=r[5 + N:8 + N].copy())
            else:
                a.update(front_vp=str(tgt), front_pos=r[5 + N:8 + N].copy(), ghost_vp=f"g{ghost}", ghost_pos=r[8 + N:11 + N].copy())
            out.append({"action": a, "vis_info": None})
        return out

    def check_overflow(self):
        """Non-zero if a capacity was ever exceeded (1) or an action named no live ghost (2); one D2H sync: call it
        where the host reads the step's results back anyway and raise."""
        return int(self.t["overflow"].item())
