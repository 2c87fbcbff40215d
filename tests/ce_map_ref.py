"""Numpy restatement of the continuous-environment (CE) agent's ghost-node map: test infrastructure, not product code.

What it restates (bevbert_ce/vlnce_baselines): models/graph_utils.py:14-75,142-372 (GraphMap and its helpers) and
ss_trainer_BEV.py:317-345,465-611,1083-1179 (_teacher_action_new from given distances, _discretize_polar_relpos, the
candidate half of _nav_bev_variable, _nav_gmap_variable, the stop-score record and the action block).  Node ids are the
integers the reference spells as strings (node k is str(k), ghost g is 'g' + str(g)), everything is kept in the padded,
fixed-capacity layout of vln_bevbert_amd.ce_map.CEGraphMap so that a test compares array with array.
tests/test_ce_map_host.py pins this file to the reference's recorded outputs (tests/golden/ce_map.npz).
"""
import numpy as np

MAX_DIST, MAX_STEP = 30, 10
INF = np.inf


def estimate_cand_pos(pos, heading, ang, dis):
    """graph_utils.py:65-75 with the heading given; ang / dis are the float32 values waypoint_step hands over."""
    ang = (heading + np.asarray(ang, np.float64)) % (2 * np.pi)
    dis = np.asarray(dis, np.float64)
    out = np.zeros((len(ang), 3))
    out[:, 0] = pos[0] - dis * np.sin(ang)
    out[:, 1] = pos[1]
    out[:, 2] = pos[2] - dis * np.cos(ang)
    return out


def position_distance(a, b):
    d = np.asarray(b, np.float64) - np.asarray(a, np.float64)
    return float(np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2))


def rel_pos_fts(a, b, base_heading, xz=False):
    """graph_utils.py:22-48 with to_clock=True, base_elevation=0."""
    dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    xz_dist = max(np.sqrt(dx ** 2 + dz ** 2), 1e-8)
    xyz_dist = max(np.sqrt(dx ** 2 + dy ** 2 + dz ** 2), 1e-8)
    heading = np.arcsin(-dx / xz_dist)
    if b[2] > a[2]:
        heading = np.pi - heading
    heading = 2 * np.pi - (heading - base_heading)
    elevation = np.arcsin(dz / xyz_dist)
    return heading, elevation, (xz_dist if xz else xyz_dist)


def dijkstra_all(W, n):
    """All-pairs Dijkstra on the dense symmetric weight matrix W (n, n) (< 0: no edge): one pass per source, the minimum
    taken with strict < (first index), distances accumulated from the source as dist[u] + w.  Returns dist, hops (number
    of nodes on the path, both ends counted), pred (predecessor of v on the path from the source, -1 at the source)."""
    dist = np.full((n, n), INF)
    hops = np.zeros((n, n), np.int32)
    pred = np.full((n, n), -1, np.int32)
    for s in range(n):
        d, h, p, done = dist[s], hops[s], pred[s], np.zeros(n, bool)
        d[s], h[s] = 0.0, 1
        for _ in range(n):
            u, best = -1, INF
            for v in range(n):
                if not done[v] and d[v] < best:
                    u, best = v, d[v]
            if u < 0:
                break
            done[u] = True
            for v in range(n):
                if W[u, v] >= 0 and not done[v]:
                    nd = d[u] + W[u, v]
                    if nd < d[v]:
                        d[v], h[v], p[v] = nd, h[u] + 1, u
    return dist, hops, pred


class EnvMap:
    """One environment's GraphMap on integer ids."""

    def __init__(self, loc_noise, merge_ghost=True, ghost_aug=0.0, node_capacity=16):
        self.loc_noise, self.merge_ghost, self.ghost_aug, self.N = loc_noise, bool(merge_ghost), ghost_aug, node_capacity
        self.pos, self.step_ids, self.embeds, self.stop_scores = [], [], [], []
        self.W = np.full((node_capacity, node_capacity), -1.0)
        self.ghosts = {}            # ghost id -> dict(pos=[...], mean, sum, cnt, fronts=[...], aug): creation order
        self.ghost_cnt, self.prev_vp = 0, None
        self.dist = self.hops = self.pred = None

    @staticmethod
    def _localize(q, items, noise):
        min_dis, min_k = 10000, None
        for k, p in items:
            dis = ((q - p) ** 2).sum() ** 0.5
            if dis < min_dis:
                min_dis, min_k = dis, k
        return None if min_dis > noise else min_k

    def update(self, step_id, cur_pos, heading, ang, dis, cur_embed, cand_embeds, noise=None):
        """identify_node + estimate_cand_pos + update_graph.  noise: {ghost id: (3,)} the (already clipped) training
        noise of this update, None = zeros.  Returns (cur, cand_slot): the node k a candidate was localized to, or
        N + g for the ghost g it went to (the numbering of gmap_ids)."""
        cur_pos = np.asarray(cur_pos, np.float64)
        cur = len(self.pos)
        cand_pos = estimate_cand_pos(cur_pos, heading, ang, dis)
        if self.prev_vp is not None:
            w = position_distance(self.pos[self.prev_vp], cur_pos)
            self.W[self.prev_vp, cur] = self.W[cur, self.prev_vp] = w
        self.pos.append(cur_pos)
        self.embeds.append(np.asarray(cur_embed))
        self.step_ids.append(step_id)
        slots = []
        for cpos, cemb in zip(cand_pos, cand_embeds):
            nvp = self._localize(cpos, enumerate(self.pos), self.loc_noise)
            if nvp is not None:
                self.W[cur, nvp] = self.W[nvp, cur] = position_distance(cur_pos, self.pos[nvp])
                slots.append(nvp)
                continue
            gvp = self._localize(cpos, [(g, v["mean"]) for g, v in self.ghosts.items()], self.loc_noise) \
                if self.merge_ghost else None
            if gvp is None:
                gvp = self.ghost_cnt
                self.ghost_cnt += 1
                self.ghosts[gvp] = {"pos": [cpos], "mean": cpos, "sum": np.asarray(cemb).copy(), "cnt": 1, "fronts": [cur]}
            else:
                g = self.ghosts[gvp]
                g["pos"].append(cpos)
                g["mean"] = np.mean(g["pos"], axis=0)
                g["sum"] = g["sum"] + cemb
                g["cnt"] += 1
                g["fronts"].append(cur)
            slots.append(self.N + gvp)
        for g, v in self.ghosts.items():
            v["aug"] = v["mean"] + (0.0 if noise is None else np.asarray(noise[g], np.float64))
        self.dist, self.hops, self.pred = dijkstra_all(self.W[:cur + 1, :cur + 1], cur + 1)
        return cur, slots

    def path(self, x, y):
        out = [y]
        while out[-1] != x:
            out.append(int(self.pred[x, out[-1]]))
        return out[::-1]

    def front_to_ghost_dist(self, g):
        min_dis, min_front = 10000, None
        for f in self.ghosts[g]["fronts"]:
            dis = position_distance(self.pos[f], self.ghosts[g]["aug"])
            if dis < min_dis:
                min_dis, min_front = dis, f
        return min_dis, min_front

    def pos_fts(self, cur, cur_pos, heading, ids):
        """get_pos_fts: ids as in gmap_ids (-1 = [stop], k < N node, N + g ghost)."""
        ang, dst = [], []
        for i in ids:
            if i < 0:
                ang.append([0, 0]); dst.append([0, 0, 0])
                continue
            if i >= self.N:
                h, e, d = rel_pos_fts(cur_pos, self.ghosts[i - self.N]["aug"], heading)
                fd, f = self.front_to_ghost_dist(i - self.N)
                sd, ss = self.dist[cur, f] + fd, self.hops[cur, f] + 1
            else:
                h, e, d = rel_pos_fts(cur_pos, self.pos[i], heading)
                sd, ss = self.dist[cur, i], self.hops[cur, i]
            ang.append([h, e]); dst.append([d / MAX_DIST, sd / MAX_DIST, ss / MAX_STEP])
        ang, dst = np.array(ang).astype(np.float32), np.array(dst).astype(np.float32)
        fts = np.vstack([np.sin(ang[:, 0]), np.cos(ang[:, 0]), np.sin(ang[:, 1]), np.cos(ang[:, 1])]).transpose()
        return np.concatenate([fts.astype(np.float32), dst], 1)

    def gmap_ids(self):
        return [-1] + list(range(len(self.pos))) + [self.N + g for g in self.ghosts]

    def pair_dists(self, ids):
        n = len(ids)
        out = np.zeros((n, n), np.float32)
        for j in range(1, n):
            for k in range(j + 1, n):
                a, b = ids[j], ids[k]
                if b < self.N:
                    d = self.dist[a, b]
                elif a < self.N:
                    fd, f = self.front_to_ghost_dist(b - self.N)
                    d = self.dist[a, f] + fd
                else:
                    fd1, f1 = self.front_to_ghost_dist(a - self.N)
                    fd2, f2 = self.front_to_ghost_dist(b - self.N)
                    d = fd1 + self.dist[f1, f2] + fd2
                out[j, k] = out[k, j] = d / MAX_DIST
        return out

    def neighbors(self, cur, cur_pos, heading):
        """get_neighbors: ids ([-1] = the current node) and the (heading, xz distance) rows, float32 values in float64."""
        ids, rel = [-1], [np.zeros(2)]
        for k, p in enumerate(self.pos):
            if self.hops[cur, k] == 2:
                h, _, d = rel_pos_fts(cur_pos, p, heading, xz=True)
                ids.append(k); rel.append(np.array([h, d], dtype=np.float32))
        for g, v in self.ghosts.items():
            if cur in v["fronts"]:
                h, _, d = rel_pos_fts(cur_pos, v["aug"], heading, xz=True)
                ids.append(self.N + g); rel.append(np.array([h, d], dtype=np.float32))
        return ids, np.array(rel)


def discretize_polar_relpos(rel, bev_dim=11, bev_res=1):
    c = int((bev_dim - 1) // 2)
    x = c + (rel[:, 1] * np.sin(rel[:, 0]) / bev_res).round()
    y = c - (rel[:, 1] * np.cos(rel[:, 0]) / bev_res).round()
    xy = np.clip(np.stack([x, y], 1), 0, bev_dim - 1).astype(np.int64)
    return xy[:, 1] * bev_dim + xy[:, 0]


def sap_fusion(gmap_ids, n_nodes, cand_ids, G, K, N):
    """pretrain_cmt.sap_fusion_indices on integer ids: src (G,) into [local | backtrack | 0], vis_c (K,)."""
    src, vis_c, tmp = np.full(G, K + 1, np.int64), np.zeros(K, bool), {}
    src[0] = 0
    for j, i in enumerate(cand_ids):
        if j > 0:
            if i < N:
                vis_c[j] = True
            else:
                tmp[i] = j
    for j, i in enumerate(gmap_ids):
        if j > 0 and i >= N:
            src[j] = tmp.get(i, K)
    return src, vis_c


def snapshot(m):
    """The graph state of a CEMapRef in the padded layout of the golden file / of CEGraphMap's arrays."""
    B, N, Gh, P = m.B, m.N, m.Gh, 16
    s = {"n_nodes": np.zeros(B, np.int64), "node_pos": np.zeros((B, N, 3)), "dist": np.full((B, N, N), np.inf),
         "hops": np.zeros((B, N, N), np.int64), "ghost_alive": np.zeros((B, Gh), bool), "ghost_mean": np.zeros((B, Gh, 3)),
         "ghost_aug": np.zeros((B, Gh, 3)), "ghost_nfronts": np.zeros((B, Gh), np.int64),
         "ghost_fronts": np.full((B, Gh, P), -1, np.int64)}
    for b, e in enumerate(m.maps):
        if not m.live[b]:
            continue
        n = len(e.pos)
        s["n_nodes"][b] = n
        s["node_pos"][b, :n] = e.pos
        s["dist"][b, :n, :n], s["hops"][b, :n, :n] = e.dist, e.hops
        for g, v in e.ghosts.items():
            s["ghost_alive"][b, g], s["ghost_mean"][b, g], s["ghost_aug"][b, g] = True, v["mean"], v["aug"]
            s["ghost_nfronts"][b, g] = len(v["fronts"])
            s["ghost_fronts"][b, g, :len(v["fronts"])] = v["fronts"]
    return s


class CEMapRef:
    """B EnvMaps behind the interface (and the padded outputs) of CEGraphMap."""

    def __init__(self, B, hidden, loc_noise=0.5, merge_ghost=True, ghost_aug=0.0, node_capacity=16, ghost_capacity=None,
                 max_cands=5, cand_capacity=15, bev_dim=11, bev_res=1):
        mg = [merge_ghost] * B if isinstance(merge_ghost, (bool, int)) else list(merge_ghost)
        self.B, self.H, self.N, self.C = B, hidden, node_capacity, max_cands
        self.Gh = 5 * node_capacity if ghost_capacity is None else ghost_capacity
        self.G, self.bev_dim, self.bev_res = 1 + self.N + self.Gh, bev_dim, bev_res
        self.maps = [EnvMap(loc_noise, mg[b], ghost_aug, node_capacity) for b in range(B)]
        self.K = 1 + cand_capacity
        self.cur = [-1] * B

    def update(self, step_id, cur_pos, heading, live, cand_count, cand_angles, cand_distances, avg_pano, pano, nav_types,
               noise=None):
        self.cur_pos, self.heading, self.live = np.asarray(cur_pos, np.float64), np.asarray(heading, np.float64), live
        slot = np.full((self.B, self.C), -1, np.int64)
        for b, m in enumerate(self.maps):
            if not live[b]:
                continue
            k = int(cand_count[b])
            ce = pano[b][np.asarray(nav_types[b]) == 1]
            assert len(ce) == k
            self.cur[b], s = m.update(step_id, self.cur_pos[b], self.heading[b], cand_angles[b][:k], cand_distances[b][:k],
                                      avg_pano[b], ce, None if noise is None else noise[b])
            slot[b, :k] = s
        return slot

    def nav_gmap_variable(self):
        B, G, H = self.B, self.G, self.H
        o = {"gmap_ids": np.full((B, G), -1, np.int64), "gmap_step_ids": np.zeros((B, G), np.int64),
             "gmap_visited_masks": np.zeros((B, G), bool), "gmap_masks": np.zeros((B, G), bool),
             "gmap_img_fts": np.zeros((B, G, H), np.float32), "gmap_pos_fts": np.zeros((B, G, 7), np.float32),
             "gmap_pair_dists": np.zeros((B, G, G), np.float32), "no_vp_left": np.zeros(B, bool)}
        for b, m in enumerate(self.maps):
            if not self.live[b]:
                continue
            ids = m.gmap_ids()
            n, nn = len(ids), len(m.pos)
            o["gmap_ids"][b, :n] = ids
            o["gmap_step_ids"][b, 1:1 + nn] = m.step_ids
            o["gmap_visited_masks"][b, 1:1 + nn] = True
            o["gmap_masks"][b, :n] = True
            for j, i in enumerate(ids[1:], 1):
                o["gmap_img_fts"][b, j] = m.embeds[i] if i < self.N else m.ghosts[i - self.N]["sum"] / m.ghosts[i - self.N]["cnt"]
            o["gmap_pos_fts"][b, :n] = m.pos_fts(self.cur[b], self.cur_pos[b], self.heading[b], ids)
            o["gmap_pair_dists"][b, :n, :n] = m.pair_dists(ids)
            o["no_vp_left"][b] = len(m.ghosts) == 0
        return o

    def bev_inputs(self):
        B, K, D = self.B, self.K, self.bev_dim
        Cn = K - 1
        o = {"bev_nav_masks": np.zeros((B, D * D), bool), "bev_cand_idxs": np.zeros((B, 1 + Cn), np.int64),
             "bev_cand_ids": np.full((B, 1 + Cn), -1, np.int64), "bev_cand_count": np.zeros(B, np.int64),
             "bev_gpos_fts": np.zeros((B, 7), np.float32), "src": np.full((B, self.G), 1 + Cn + 1, np.int64),
             "vis_c": np.zeros((B, 1 + Cn), bool)}
        o["src"][:, 0] = 0
        for b, m in enumerate(self.maps):
            if not self.live[b]:
                continue
            ids, rel = m.neighbors(self.cur[b], self.cur_pos[b], self.heading[b])
            idx = discretize_polar_relpos(rel, D, self.bev_res)
            n = len(ids)
            o["bev_nav_masks"][b, idx] = True
            o["bev_cand_idxs"][b, :n], o["bev_cand_ids"][b, :n], o["bev_cand_count"][b] = idx, ids, n
            o["bev_gpos_fts"][b] = m.pos_fts(self.cur[b], self.cur_pos[b], self.heading[b], [0])[0]
            gi = m.gmap_ids()
            src, o["vis_c"][b] = sap_fusion(gi, len(m.pos), ids, self.G, 1 + Cn, self.N)
            src[len(gi):] = 1 + Cn + 1
            o["src"][b] = src
        return o

    def record_stop_scores(self, probs0):
        for b, m in enumerate(self.maps):
            if self.live[b]:
                m.stop_scores.append(np.float32(probs0[b]))

    def teacher_index(self, cur_dist_to_goal, ghost_goal_dist):
        out = np.full(self.B, -100, np.int64)
        for b, m in enumerate(self.maps):
            if not self.live[b]:
                continue
            if cur_dist_to_goal[b] < 1.5:
                out[b] = 0
            elif len(m.ghosts):
                gs = list(m.ghosts)
                out[b] = 1 + len(m.pos) + int(np.argmin([ghost_goal_dist[b][g] for g in gs]))
        return out

    def act(self, a_t, last_step, consume_ghost=True):
        """ss_trainer_BEV.py:1110-1179 -> list of the 'action' dicts with integer ids (None for an ended sample)."""
        out = []
        for b, m in enumerate(self.maps):
            if not self.live[b]:
                out.append(None)
                continue
            cur = self.cur[b]
            if a_t[b] == 0 or last_step or len(m.ghosts) == 0:
                stop = int(np.argmax(m.stop_scores))
                out.append({"act": 0, "cur_vp": cur, "stop_vp": stop, "stop_pos": m.pos[stop], "back_path": m.path(cur, stop)[1:]})
            else:
                g = m.gmap_ids()[int(a_t[b])] - self.N
                _, front = m.front_to_ghost_dist(g)
                out.append({"act": 4, "cur_vp": cur, "front_vp": front, "front_pos": m.pos[front], "ghost_vp": g,
                            "ghost_pos": m.ghosts[g]["aug"], "back_path": m.path(cur, front)[1:]})
                m.prev_vp = front
                if consume_ghost:
                    m.ghosts.pop(g)
        return out


def replay(gold, noise=None, **kw):
    """The restatement driven through the recorded episodes of tests/golden/ce_map.npz: one dict of outputs per step.
    noise[t][b] = {ghost id: (3,)}: the training noise of that update (None = none)."""
    T, B = gold["in_live"].shape
    m = CEMapRef(B, gold["in_avg_pano"].shape[-1], float(gold["loc_noise"]), gold["merge_ghost"].tolist(), **kw)
    steps = []
    for t in range(T):
        i = {k[3:]: gold[k][t] for k in gold.files if k.startswith("in_")}
        o = {"cand_slot": m.update(t + 1, i["cur_pos"], i["heading"], i["live"], i["cand_count"], i["cand_angles"],
                                   i["cand_distances"], i["avg_pano"], i["pano"], i["nav_types"],
                                   None if noise is None else noise[t])}
        o["state"] = snapshot(m)
        o.update(m.nav_gmap_variable())
        o.update(m.bev_inputs())
        m.record_stop_scores(i["probs0"])
        o["teacher"] = m.teacher_index(i["cur_dist"], i["ghost_dist"])
        o["actions"] = m.act(i["a_t"], t == T - 1)
        steps.append(o)
    return steps


def grids(t, B=3):
    """The recorded episodes' panorama of step t: (B,12,196,768) grid features (whole numbers: cell means are exact in
    float32) and (B,12,14,14) depths / 10 with a tenth of the pixels at 0 (no depth)."""
    from tests.waypoint_ref import synthetic
    rgb = synthetic(1000 + t, (B, 12, 196, 768), ints=True)
    dep = np.abs(synthetic(2000 + t, (B, 12, 14, 14))) * 0.5
    dep[synthetic(3000 + t, (B, 12, 14, 14)) < -0.9] = 0.0
    return rgb, dep.astype(np.float32)
