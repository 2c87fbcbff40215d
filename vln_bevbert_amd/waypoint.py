"""Device-side candidate waypoint prediction of the continuous-environment (CE) agent.

In the discrete task the simulator hands the agent its candidates; in CE the agent predicts them every step, before the
panorama encoder can run (bevbert_ce/vlnce_baselines/models/Policy_ViewSelection_BEV.py:166-321 mode 'waypoint', driven
from ss_trainer_BEV.py:1019-1031).  The reference does the part behind the predictor in Python loops over the batch with
nonzero() / .cpu() / .tolist() per sample; here the whole stage is a fixed sequence of launches with fixed output shapes
and no host synchronisation (csrc/waypoint.hip), so it can be captured in a hipGraph together with the navigation step:

    WaypointPredictor   BinaryDistPredictor_TRM (waypoint_pred/TRM_net.py), forward only, same state_dict
    waypoint_step       predictor -> candidates (+ training draw) -> panorama-encoder inputs, all on the device
    to_reference        one device-to-host copy -> the reference's list-shaped wp_outputs (the Habitat-side consumers)
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .lib import dtype_code, ptr, stream

NUM_ANGLES, NUM_IMGS, NUM_DISTS = 120, 12, 12
K_MAX = 5           # nms(max_predictions=5)
L_PAD = 17          # 5 candidates + 12 views


class _Holder(nn.Module):
    """Bare container: gives parameters the reference's dotted names."""


class _TFLayerNorm(nn.Module):
    """The reference's BertLayerNorm parameters (weight / bias; eps inside the square root, as the fused kernel)."""

    def __init__(self, hidden, eps=1e-12):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.bias = nn.Parameter(torch.zeros(hidden))
        self.variance_epsilon = eps


class _Layer(nn.Module):
    def __init__(self, H, inter, eps):
        super().__init__()
        self.attention = _Holder()
        self.attention.self = _Holder()
        for k in ("query", "key", "value"):
            setattr(self.attention.self, k, nn.Linear(H, H))
        self.attention.output = _Holder()
        self.attention.output.dense = nn.Linear(H, H)
        self.attention.output.LayerNorm = _TFLayerNorm(H, eps)
        self.intermediate = _Holder()
        self.intermediate.dense = nn.Linear(H, inter)
        self.output = _Holder()
        self.output.dense = nn.Linear(inter, H)
        self.output.LayerNorm = _TFLayerNorm(H, eps)


class WaypointPredictor(nn.Module):
    """BinaryDistPredictor_TRM: Linear(2048, 768) + ReLU on the 12 depth embeddings, a 2-layer post-norm BERT encoder in
    which a view attends to itself and its two ring neighbours, a 768 -> 768 -> 120 classifier; the (12, 120) rows are the
    (120, 12) angle x distance map, rolled by HEATMAP_OFFSET = 5.  Same constructor defaults, state_dict keys and shapes
    as the reference, including the parameters its forward never touches (visual_merge.*, mergefeats_LayerNorm.*), so the
    published checkpoint's ['predictor']['state_dict'] loads with strict=True.  Frozen and always eval there
    (ss_trainer_BEV.py:239-240,684,780,905): forward only, a call in training mode raises."""

    TRM_LAYER, TRM_NEIGHBOR, HEATMAP_OFFSET = 2, 1, 5
    NUM_HEADS, INTERMEDIATE, LN_EPS = 12, 3072, 1e-12

    def __init__(self, hidden_dim=768, n_classes=12, device=None):
        super().__init__()
        self.device = device
        self.num_angles, self.num_imgs, self.n_classes = NUM_ANGLES, NUM_IMGS, n_classes
        if hidden_dim != self.NUM_HEADS * 64:
            raise ValueError("the ring attention kernel is specialised for 64-wide heads (hidden_dim = 768)")
        self.visual_fc_depth = nn.Sequential(nn.Flatten(), nn.Linear(128 * 4 * 4, hidden_dim), nn.ReLU(True))
        self.visual_merge = nn.Sequential(nn.Linear(hidden_dim * 2, hidden_dim), nn.ReLU(True))     # unused, as there
        self.waypoint_TRM = _Holder()
        self.waypoint_TRM.bert = _Holder()
        self.waypoint_TRM.bert.encoder = _Holder()
        self.waypoint_TRM.bert.encoder.layer = nn.ModuleList(
            [_Layer(hidden_dim, self.INTERMEDIATE, self.LN_EPS) for _ in range(self.TRM_LAYER)])
        self.mergefeats_LayerNorm = _TFLayerNorm(hidden_dim, self.LN_EPS)                         # unused, as there
        self.vis_classifier = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                            nn.Linear(hidden_dim, int(n_classes * (self.num_angles / self.num_imgs))))
        for p in self.parameters():
            p.requires_grad_(False)
        self._c = None
        self.eval()

    def finalize(self, device, compute_dtype=torch.float32):
        """Move the parameters to ``device`` and build the compute-dtype GEMM operands (packed q|k|v per layer).  The
        predictor is frozen, so it needs no gradient arena; call again after loading other weights."""
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("compute dtype must be float32 or bfloat16")
        self.to(device)
        for p in self.parameters():
            p.requires_grad_(False)
        cd = compute_dtype

        def w(lin):
            return lin.weight.detach().to(cd).contiguous()
        c = {"dtype": cd, "fc": w(self.visual_fc_depth[1]), "cls0": w(self.vis_classifier[0]),
             "cls2": w(self.vis_classifier[2]), "cls2_b": self.vis_classifier[2].bias.detach().to(cd), "layers": []}
        for lyr in self.waypoint_TRM.bert.encoder.layer:
            s = lyr.attention.self
            c["layers"].append({
                "qkv": torch.cat([s.query.weight, s.key.weight, s.value.weight], 0).detach().to(cd).contiguous(),
                "qkv_b": torch.cat([s.query.bias, s.key.bias, s.value.bias], 0).detach().to(cd).contiguous(),
                "ao": w(lyr.attention.output.dense), "inter": w(lyr.intermediate.dense), "out": w(lyr.output.dense)})
        self._c = c
        self.eval()
        return self

    def classifier_output(self, depth_feats):
        """(B*12, 128, 4, 4) -> (B, 12, 120) fp32: the classifier rows before the roll (what the candidate kernel takes)."""
        if self.training:
            raise RuntimeError("WaypointPredictor is forward-only (the reference never trains it): call .eval()")
        if self._c is None:
            raise RuntimeError("WaypointPredictor: call finalize(device, compute_dtype) first -- there is no CPU path")
        c = self._c
        cd = c["dtype"]
        ops.RT.res32 = False
        with torch.no_grad():
            x = depth_feats.reshape(depth_feats.shape[0], -1).to(cd)
            B = x.shape[0] // NUM_IMGS
            fc = self.visual_fc_depth[1]
            h = ops.bias_relu(ops.linear(x, fc.weight, None, w_c=c["fc"]), fc.bias)
            for lyr, lc in zip(self.waypoint_TRM.bert.encoder.layer, c["layers"]):
                s, ao = lyr.attention.self, lyr.attention.output
                qkv = ops.linear(h, s.query.weight, s.query.bias, w_c=lc["qkv"], b_c=lc["qkv_b"])
                a = ring_attention(qkv.view(B, NUM_IMGS, -1), self.NUM_HEADS).view(B * NUM_IMGS, -1)
                a = ops.bias_dropout_residual_layernorm(ops.linear(a, ao.dense.weight, None, w_c=lc["ao"]), ao.dense.bias, h,
                                                        ao.LayerNorm.weight, ao.LayerNorm.bias, self.LN_EPS)
                i = ops.bias_gelu(ops.linear(a, lyr.intermediate.dense.weight, None, w_c=lc["inter"]),
                                  lyr.intermediate.dense.bias)
                h = ops.bias_dropout_residual_layernorm(ops.linear(i, lyr.output.dense.weight, None, w_c=lc["out"]),
                                                        lyr.output.dense.bias, a, lyr.output.LayerNorm.weight,
                                                        lyr.output.LayerNorm.bias, self.LN_EPS)
            c0, c2 = self.vis_classifier[0], self.vis_classifier[2]
            h = ops.bias_relu(ops.linear(h, c0.weight, None, w_c=c["cls0"]), c0.bias)
            y = ops.linear(h, c2.weight, c2.bias, w_c=c["cls2"], b_c=c["cls2_b"])
            return y.view(B, NUM_IMGS, -1).float()

    def forward(self, rgb_feats, depth_feats):
        """The reference's signature (rgb_feats is ignored there too): (B, 120, 12) logits, rolled by HEATMAP_OFFSET."""
        y = self.classifier_output(depth_feats)
        return torch.roll(y.view(y.shape[0], self.num_angles, self.n_classes), -self.HEATMAP_OFFSET, 1)


def ring_attention(qkv, nh):
    """Self-attention of packed qkv (B, 12, 3 * nh * 64) over the ring of 12 views (a view sees itself and its two
    neighbours); forward only."""
    if qkv.dim() != 3 or qkv.shape[1] != NUM_IMGS or qkv.shape[2] != 3 * nh * 64 or not qkv.is_contiguous():
        raise ValueError(f"ring_attention: contiguous (B, 12, {3 * nh * 64}) expected, got {tuple(qkv.shape)}")
    out = torch.empty(qkv.shape[0], NUM_IMGS, nh * 64, dtype=qkv.dtype, device=qkv.device)
    ops.call("bevbert_wp_ring_attn", ptr(qkv), ptr(out), qkv.shape[0], nh, 0.125, dtype_code(qkv), stream())
    return out


_PANO_FTS = {}


def pano_angle_fts(device):
    """(12, 4) angle features of the counter-clockwise views (Policy_ViewSelection_BEV.py:132-134): float64, then cast."""
    t = _PANO_FTS.get(device)
    if t is None:
        rad = torch.from_numpy((1 - np.arange(NUM_IMGS, dtype=np.int64) / 12) * 2 * math.pi)
        t = torch.stack([torch.sin(rad), torch.cos(rad), torch.zeros_like(rad), torch.ones_like(rad)], 1).float()
        t = _PANO_FTS[device] = t.to(device)
    return t


def waypoint_candidates(cls_logits, in_train=False, seed=0, t=0):
    """Candidates from classifier rows (B, 12, 120) (before the roll): dict of fixed-shape device tensors."""
    B, dev = cls_logits.shape[0], cls_logits.device
    if tuple(cls_logits.shape[1:]) != (NUM_IMGS, 120):
        raise ValueError(f"waypoint_candidates: (B, 12, 120) expected, got {tuple(cls_logits.shape)}")
    x = cls_logits.float().contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    o = {"cand_count": torch.empty(B, **i32), "cand_angle_idx": torch.empty(B, K_MAX, **i32),
         "cand_dist_idx": torch.empty(B, K_MAX, **i32), "cand_img_idx": torch.empty(B, K_MAX, **i32),
         "cand_angle_fts": torch.empty(B, K_MAX, 4, **f32), "cand_angles": torch.empty(B, K_MAX, **f32),
         "cand_distances": torch.empty(B, K_MAX, **f32), "heat": torch.empty(B, NUM_ANGLES, NUM_DISTS, **f32)}
    if in_train:
        o["region_probs"] = torch.empty(B, K_MAX, 120, **f32)
        o["rand"] = torch.empty(B, K_MAX, **f32)
    ops.call("bevbert_wp_candidates", ptr(x), B, int(bool(in_train)), int(seed) & 0xFFFFFFFF, int(t), ptr(o["cand_count"]),
             ptr(o["cand_angle_idx"]), ptr(o["cand_dist_idx"]), ptr(o["cand_img_idx"]), ptr(o["cand_angle_fts"]),
             ptr(o["cand_angles"]), ptr(o["cand_distances"]), ptr(o.get("region_probs")), ptr(o["heat"]),
             ptr(o.get("rand")), stream())
    return o


def waypoint_pano_inputs(rgb_embeds, depth_embeds, cand):
    """Pooled counter-clockwise panorama features and the panorama-encoder inputs padded to 17 rows."""
    dev = rgb_embeds.device
    B = rgb_embeds.shape[0] // NUM_IMGS
    if rgb_embeds.numel() != B * NUM_IMGS * 512 or depth_embeds.numel() != B * NUM_IMGS * 2048 or \
            rgb_embeds.dtype != depth_embeds.dtype or cand["cand_count"].shape[0] != B:
        raise ValueError("waypoint_pano_inputs: rgb (B*12, 512) and depth (B*12, 128, 4, 4) of one dtype expected")
    rgb, dep = rgb_embeds.contiguous(), depth_embeds.contiguous()
    dt = dict(dtype=rgb.dtype, device=dev)
    o = {"pano_rgb": torch.empty(B, NUM_IMGS, 512, **dt), "pano_depth": torch.empty(B, NUM_IMGS, 128, **dt)}
    vp = {"rgb_fts": torch.empty(B, L_PAD, 512, **dt), "dep_fts": torch.empty(B, L_PAD, 128, **dt),
          "loc_fts": torch.empty(B, L_PAD, 4, dtype=torch.float32, device=dev),
          "nav_types": torch.empty(B, L_PAD, dtype=torch.int64, device=dev),
          "view_lens": torch.empty(B, dtype=torch.int64, device=dev)}
    ops.call("bevbert_wp_pano_inputs", ptr(rgb), ptr(dep), dtype_code(rgb), B, ptr(cand["cand_count"]),
             ptr(cand["cand_img_idx"]), ptr(cand["cand_angle_fts"]), ptr(pano_angle_fts(dev)), ptr(o["pano_rgb"]),
             ptr(o["pano_depth"]), ptr(vp["rgb_fts"]), ptr(vp["dep_fts"]), ptr(vp["loc_fts"]), ptr(vp["nav_types"]),
             ptr(vp["view_lens"]), stream())
    o["vp_inputs"] = vp
    return o


def waypoint_step(predictor, rgb_embeds, depth_embeds, in_train=False, seed=0, t=0, cls_logits=None):
    """Mode 'waypoint' behind the image backbones: rgb_embeds (B*12, 512), depth_embeds (B*12, 128, 4, 4) in the
    predictor's clockwise view order -> dict of device tensors: cand_count, cand_angle_idx, cand_dist_idx, cand_img_idx,
    cand_angle_fts, cand_angles, cand_distances, heat, (in_train: region_probs, rand), pano_rgb, pano_depth, pano_angle_fts
    and vp_inputs = {rgb_fts, dep_fts, loc_fts, nav_types, view_lens}, which ImageEmbeddings.embed(...,
    view_dep_fts=...) takes as they are.  in_train: the waypoint_aug draw, hashed from (seed, t) and the step salt.
    ``cls_logits`` (B, 12, 120) replaces the predictor's output (tests, recorded maps).  Nothing here synchronises."""
    if cls_logits is None:
        cls_logits = predictor.classifier_output(depth_embeds)
    out = waypoint_candidates(cls_logits, in_train, seed, t)
    out.update(waypoint_pano_inputs(rgb_embeds, depth_embeds, out))
    out["pano_angle_fts"] = pano_angle_fts(rgb_embeds.device)
    return out


_SMALL = ("cand_count", "cand_angle_idx", "cand_dist_idx", "cand_img_idx", "cand_angle_fts", "cand_angles",
          "cand_distances")


def to_reference(out):
    """The reference's list-shaped wp_outputs from a waypoint_step result.  ONE device-to-host copy (the small integer /
    float tensors, packed into one float64 buffer: every value is exact in it); the feature entries stay on the device
    as per-sample slices.  The only place of this module that synchronises."""
    B = out["cand_count"].shape[0]
    packed = torch.cat([out[k].reshape(B, -1).double() for k in _SMALL], 1).cpu().numpy()
    cols = np.cumsum([0] + [out[k][0].numel() for k in _SMALL])
    host = {k: packed[:, cols[i]:cols[i + 1]] for i, k in enumerate(_SMALL)}
    n = host["cand_count"][:, 0].astype(np.int64)
    img = host["cand_img_idx"].astype(np.int64)
    fts = host["cand_angle_fts"].astype(np.float32).reshape(B, K_MAX, 4)
    ref = {"cand_rgb": [], "cand_depth": [], "cand_angle_fts": [], "cand_img_idxes": [], "cand_angles": [],
           "cand_distances": [], "pano_rgb": out["pano_rgb"], "pano_depth": out["pano_depth"],
           "pano_angle_fts": out["pano_angle_fts"], "pano_img_idxes": np.arange(NUM_IMGS, dtype=np.int64)}
    for b in range(B):
        k = int(n[b])
        ref["cand_rgb"].append(out["vp_inputs"]["rgb_fts"][b, :k])
        ref["cand_depth"].append(out["vp_inputs"]["dep_fts"][b, :k])
        ref["cand_angle_fts"].append(torch.from_numpy(fts[b, :k].copy()))
        ref["cand_img_idxes"].append(img[b, :k].copy())
        ref["cand_angles"].append(host["cand_angles"][b, :k].astype(np.float32).tolist())
        ref["cand_distances"].append(host["cand_distances"][b, :k].astype(np.float32).tolist())
    return ref
