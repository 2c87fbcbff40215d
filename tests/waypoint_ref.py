"""CPU restatement of the CE agent's candidate waypoint stage, for the waypoint tests only.

Written from the behaviour the reference shows under the installed torch (mode 'waypoint' of the CE policy, its nms
helper and the trainer's panorama-input collation), not from its text; tests/test_waypoint_host.py pins it to the
reference's recorded outputs (tests/golden/waypoint.npz).  The four quirks it keeps are listed in
vln_bevbert_amd/csrc/waypoint.hip (Q1-Q4).

Conventions: `logits` is the predictor's output (120, 12), i.e. AFTER its roll by 5; `unroll` gives the classifier
layout (12, 120) the device stage takes.
"""
import math

import numpy as np
import torch

K_MAX, L_PAD, VIEWS, ANGLES, DISTS = 5, 17, 12, 120, 12


def synthetic(seed, shape, ints=False):
    """Deterministic pseudo-random fp32 array that needs no stored data and no library generator: an integer hash of
    the flat index.  ints: whole numbers in [-8, 8) (their 4 x 4 means are exact in fp32); else values in [-1, 1)."""
    n = int(np.prod(shape))
    x = np.arange(n, dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    if ints:
        return ((x >> np.uint64(40)) % np.uint64(16)).astype(np.float32).reshape(shape) - 8.0
    return ((x >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32).reshape(shape)


def unroll(logits):
    """Predictor output (..., 120, 12) -> classifier output (..., 12, 120): row r of the classifier's (120, 12) view is
    angle r - 5."""
    t = torch.as_tensor(logits)
    return torch.roll(t, 5, dims=-2).reshape(*t.shape[:-2], VIEWS, 120)


def heat_map(logits):
    t = torch.as_tensor(logits, dtype=torch.float32)
    return torch.softmax(t.reshape(-1), 0).reshape(ANGLES, DISTS)


def _suppressed(w, d, pr, pc):
    lo = pr - 5 if pc == 0 else pr - 4              # Q1: the centre is the fractional row pr + pc / 12
    dd = d - pc
    return lo <= w <= pr + 5 and min(abs(dd), abs(dd + DISTS)) <= 7     # Q2


def nms_picks(P, with_margin=False):
    """P (120, 12) probabilities -> ([(angle, dist)] in row-major order, min relative lead of a pick over the best other
    live cell, its exact wrap duplicate aside)."""
    P = np.asarray(P, dtype=np.float32)
    W = np.concatenate([P[-1:], P, P[:1]], 0)       # Q3
    S = W.copy()
    cells, margin = set(), math.inf
    ws, ds = np.divmod(np.arange(S.size), DISTS)
    for _ in range(K_MAX):
        ix = int(np.argmax(S.reshape(-1)))          # the first index wins ties
        pr, pc = divmod(ix, DISTS)
        if with_margin:
            flat = S.reshape(-1).astype(np.float64).copy()
            flat[ix] = -1.0
            dup = {0: ANGLES, ANGLES: 0, 1: ANGLES + 1, ANGLES + 1: 1}.get(pr)
            if dup is not None:
                flat[dup * DISTS + pc] = -1.0
            margin = min(margin, (float(S[pr, pc]) - flat.max()) / float(S[pr, pc]))
        if 1 <= pr <= ANGLES and W[pr, pc] != 0:
            cells.add((pr - 1) * DISTS + pc)
        kill = np.array([_suppressed(int(w), int(d), pr, pc) for w, d in zip(ws, ds)]).reshape(S.shape)
        S[kill] *= 0
    out = [divmod(c, DISTS) for c in sorted(cells)]
    return (out, margin) if with_margin else out


def region_probs(logits, angle):
    """The 120 probabilities the training draw of a candidate at `angle` is taken from: softmax over the cells of its
    (clockwise) image, angles 10 img - 5 .. 10 img + 4, distance fastest."""
    raw = unroll(torch.as_tensor(logits, dtype=torch.float32))
    img = ((angle + 5) // 10) % VIEWS
    return torch.softmax(raw[img], 0)


def draw_cell(angle, act):
    """(angle, dist) of region cell `act` for a candidate first found at `angle` (Q4: image 0 counts from angle 0)."""
    img = ((angle + 5) // 10) % VIEWS
    pointer = (img - 1) * 10 + 5 if img != 0 else 0
    return act // DISTS + pointer, act % DISTS


def inverse_cdf(probs, u):
    """First cell whose cumulative probability exceeds u; also the distance of u to the nearest CDF step."""
    c = np.cumsum(np.asarray(probs, dtype=np.float64))
    j = int(np.searchsorted(c, u, side="right"))
    return min(j, len(c) - 1), float(np.abs(c - u).min())


def cand_features(angles, dists):
    """img idx (counter-clockwise), angle features (K, 4), angles (counter-clockwise rad), distances -- fp32 arithmetic
    in the order the reference applies it."""
    a = torch.tensor(list(angles), dtype=torch.int64)
    d = torch.tensor(list(dists), dtype=torch.int64)
    rad_c = a.float() / 120 * 2 * math.pi
    rad_cc = 2 * math.pi - a.float() / 120 * 2 * math.pi
    fts = torch.stack([torch.sin(rad_c), torch.cos(rad_c), torch.zeros_like(rad_c), torch.ones_like(rad_c)], 1)
    img = 12 - (a + 5) // 10
    img[img == 12] = 0
    return img, fts, rad_cc, (d + 1) * 0.25


def pano_angle_fts():
    idx = np.arange(VIEWS, dtype=np.int64)
    rad = torch.from_numpy((1 - idx / 12) * 2 * math.pi)
    return torch.stack([torch.sin(rad), torch.cos(rad), torch.zeros_like(rad), torch.ones_like(rad)], 1).float()


def pano_features(rgb_embeds, depth_embeds):
    """(B*12, 512), (B*12, 128, 4, 4) clockwise -> counter-clockwise (B, 12, 512), (B, 12, 128) with the 4 x 4 mean."""
    rgb = torch.as_tensor(rgb_embeds).reshape(-1, VIEWS, 512)
    dep = torch.as_tensor(depth_embeds).reshape(-1, VIEWS, 128, 16).float().mean(-1)
    order = [0] + list(range(VIEWS - 1, 0, -1))
    return rgb[:, order], dep[:, order]


def vp_inputs(pano_rgb, pano_depth, img_idx, angle_fts):
    """One sample's panorama-encoder rows padded to 17: candidates, then the views no candidate points into."""
    k = len(img_idx)
    free = [v for v in range(VIEWS) if v not in set(int(i) for i in img_idx)]
    rows = [int(i) for i in img_idx] + free
    n = len(rows)
    rgb = torch.zeros(L_PAD, 512, dtype=pano_rgb.dtype)
    dep = torch.zeros(L_PAD, 128, dtype=pano_depth.dtype)
    loc = torch.zeros(L_PAD, 4)
    nav = torch.zeros(L_PAD, dtype=torch.int64)
    rgb[:n], dep[:n] = pano_rgb[rows], pano_depth[rows]
    if k:
        loc[:k] = angle_fts
    loc[k:n] = pano_angle_fts()[free]
    nav[:k] = 1
    return rgb, dep, loc, nav, n


def stage(logits, rgb_embeds=None, depth_embeds=None, acts=None):
    """The whole eval stage (acts = None) or the training stage with hand-set region cells `acts` (B, 5) for a batch of
    predictor outputs (B, 120, 12): dict of fixed-shape arrays in the device stage's layout."""
    logits = torch.as_tensor(logits, dtype=torch.float32)
    B = logits.shape[0]
    o = {"cand_count": np.zeros(B, np.int32), "cand_angle_idx": -np.ones((B, K_MAX), np.int32),
         "cand_dist_idx": -np.ones((B, K_MAX), np.int32), "cand_img_idx": -np.ones((B, K_MAX), np.int32),
         "cand_angle_fts": np.zeros((B, K_MAX, 4), np.float32), "cand_angles": np.zeros((B, K_MAX), np.float32),
         "cand_distances": np.zeros((B, K_MAX), np.float32), "heat": np.zeros((B, ANGLES, DISTS), np.float32),
         "region_probs": np.zeros((B, K_MAX, 120), np.float32), "margin": np.zeros(B)}
    if rgb_embeds is not None:
        prgb, pdep = pano_features(rgb_embeds, depth_embeds)
        o.update(pano_rgb=prgb.numpy(), pano_depth=pdep.numpy(), rgb_fts=np.zeros((B, L_PAD, 512), np.float32),
                 dep_fts=np.zeros((B, L_PAD, 128), np.float32), loc_fts=np.zeros((B, L_PAD, 4), np.float32),
                 nav_types=np.zeros((B, L_PAD), np.int64), view_lens=np.zeros(B, np.int64))
    for b in range(B):
        P = heat_map(logits[b])
        picks, o["margin"][b] = nms_picks(P.numpy(), with_margin=True)
        k = len(picks)
        o["heat"][b] = P.numpy()
        o["cand_count"][b] = k
        for j, (a, _) in enumerate(picks):
            o["region_probs"][b, j] = region_probs(logits[b], a).numpy()
        if acts is not None:
            picks = [draw_cell(a, int(acts[b][j])) for j, (a, _) in enumerate(picks)]
        img, fts, rad, dist = cand_features([p[0] for p in picks], [p[1] for p in picks])
        o["cand_angle_idx"][b, :k] = [p[0] for p in picks]
        o["cand_dist_idx"][b, :k] = [p[1] for p in picks]
        o["cand_img_idx"][b, :k] = img.numpy()
        o["cand_angle_fts"][b, :k] = fts.numpy()
        o["cand_angles"][b, :k] = rad.numpy()
        o["cand_distances"][b, :k] = dist.numpy()
        if rgb_embeds is not None:
            r, d, l, nv, n = vp_inputs(prgb[b], pdep[b], img, fts)
            o["rgb_fts"][b], o["dep_fts"][b], o["loc_fts"][b], o["nav_types"][b], o["view_lens"][b] = \
                r.numpy(), d.numpy(), l.numpy(), nv.numpy(), n
    return o


def ring_attention(qkv, nh, masked=False):
    """fp64 self-attention over the ring of 12 views from packed qkv (B, 12, 3 * nh * 64): the three-key softmax, or
    (masked) the reference's form: all 12 keys with -10000 added to the nine others."""
    x = torch.as_tensor(qkv).double()
    B = x.shape[0]
    q, k, v = (t.reshape(B, VIEWS, nh, 64).transpose(1, 2) for t in x.chunk(3, -1))
    s = q @ k.transpose(-1, -2) / 8.0
    i = torch.arange(VIEWS)
    near = ((i[:, None] - i[None, :]) % VIEWS)
    near = (near <= 1) | (near == VIEWS - 1)
    if masked:
        p = torch.softmax(s + (~near).double() * -10000.0, -1)
    else:
        p = torch.softmax(s.masked_fill(~near, -math.inf), -1)
    return (p @ v).transpose(1, 2).reshape(B, VIEWS, nh * 64)
