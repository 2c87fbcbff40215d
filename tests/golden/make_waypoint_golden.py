"""Regenerate tests/golden/waypoint.npz and tests/golden/waypoint_keys.txt from the reference's own code.

Build machine only (the reference is read from REF, imported -- not copied):
  * vlnce_baselines/waypoint_pred/TRM_net.py BinaryDistPredictor_TRM, weights from weights.fill_state_dict over the
    module's own key / shape list (stored as waypoint_keys.txt), eval mode, B = 3 seeded depth embeddings;
  * vlnce_baselines/models/Policy_ViewSelection_BEV.py BEV.forward(mode='waypoint') on a stand-in `self` whose encoders
    hand back given embeddings and with a stand-in predictor that hands back GIVEN logits (network rounding cannot move a
    discrete decision); its nms is the reference's own (waypoint_pred/utils.py);
  * vlnce_baselines/ss_trainer_BEV.py RLTrainer._vp_feature_variable on a stand-in `self` (it reads envs.num_envs only).
Stand-ins: pytorch_transformers re-exports the BertConfig the reference vendors; vlnce_baselines is registered as a bare
package so that its __init__ (Habitat) never runs; every other module these files import at module level and do not use
on these paths (habitat, gym, lmdb, ...) is an empty stub; torch.Tensor.cuda is the identity; np.bool is aliased.

Maps (all as predictor outputs (120, 12), i.e. after the roll):
  (a) 64 random permutations of the arithmetic progression 0, 0.01, ... (spread 14.4);
  (b) hand-placed peaks over a low permuted background, one map per quirk of the stage (see _hand_maps);
  (c) the three network outputs as they are: with the rule-seeded weights every pick leads the best other live cell by
      a relative 6e-4 or more on the reference's own probabilities (asserted below: at most one of the three may miss
      1e-4), so no scaling of the logits was needed.
Training draw: torch.distributions.Categorical is replaced, for that one call, by a stand-in that records the
probabilities it is given and returns hand-set cells, so the reference's own loop maps them to angles / distances.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REAL = ("vlnce_baselines.waypoint_pred", "vlnce_baselines.models.utils", "vlnce_baselines.models.Policy_ViewSelection_BEV",
        "vlnce_baselines.ss_trainer_BEV", "vlnce_baselines.utils", "vlnce_baselines.common.ops",
        "vlnce_baselines.common.transformer")
STUBS = ("habitat", "habitat_baselines", "habitat_extensions", "gym", "lmdb", "msgpack_numpy", "jsonlines", "fastdtw",
         "boto3", "botocore", "requests", "tqdm", "six", "einops", "torch_scatter")      # (never apex: its absence is handled)
PKGS = ("vlnce_baselines", "vlnce_baselines.models", "vlnce_baselines.common")


class _Meta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub

    def __call__(cls, *a, **k):                      # decorator (with or without arguments), constructor: all inert
        if cls is not _Stub:
            return super().__call__(*a, **k)
        return a[0] if len(a) == 1 and not k and isinstance(a[0], type) else _Stub


class _Stub(metaclass=_Meta):
    pass


class _StubModule(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, only_unwanted):
        self.only_unwanted = only_unwanted

    def find_spec(self, name, path, target=None):
        if self.only_unwanted:                       # in front: vlnce_baselines modules off the used paths
            if not name.startswith("vlnce_baselines") or name in PKGS or any(name == r or name.startswith(r + ".") for r in REAL):
                return None
        elif name.split(".")[0] not in STUBS:
            return None
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _StubModule(spec.name)

    def exec_module(self, module):
        pass


def _stand_ins():
    base = os.path.join(REF, "bevbert_ce")
    for p in PKGS:
        m = types.ModuleType(p)
        m.__path__ = [os.path.join(base, *p.split("."))]
        sys.modules[p] = m
    for name in ("turtle", "tensorflow", "cv2"):
        sys.modules[name] = _StubModule(name)
    sys.meta_path.insert(0, _Finder(True))
    sys.meta_path.append(_Finder(False))             # last: those of STUBS that are not installed
    from vlnce_baselines.waypoint_pred.transformer.pytorch_transformer import modeling_bert
    pt = types.ModuleType("pytorch_transformers")
    pt.BertConfig = modeling_bert.BertConfig
    sys.modules["pytorch_transformers"] = pt
    torch.Tensor.cuda = lambda self, *a, **k: self
    if not hasattr(np, "bool"):
        np.bool = bool


def _hand_maps(rng):
    """One map per quirk; the background is a permutation of -10, -9.998, ... (all distinct, far below the peaks)."""
    def bg():
        return (rng.permutation(1440) * 0.002 - 10.0).reshape(120, 12).astype(np.float32)
    maps, want = [], []
    m = bg(); m[119, 3] = 5; m[60, 6] = 4; m[30, 6] = 3; m[90, 6] = 2; m[10, 6] = 1
    maps.append(m); want.append("max at angle 119 (col > 0): the wrap-row pick is cut off, its duplicate returns")
    m = bg(); m[0, 0] = 5; m[60, 6] = 4; m[30, 6] = 3; m[90, 6] = 2; m[100, 6] = 1
    maps.append(m); want.append("max at angle 0 (col = 0): the duplicate in the last wrap row is picked and cut off")
    m = bg(); m[50, 0] = 5; m[45, 0] = 4.5; m[55, 0] = 4.4; m[44, 0] = 4.3; m[56, 0] = 4.2
    maps.append(m); want.append("col = 0: rows -5 .. +5 suppressed, the peaks 6 rows away survive")
    m = bg(); m[50, 4] = 5; m[45, 4] = 4.5; m[55, 4] = 4.4; m[56, 4] = 4.3; m[44, 4] = 4.2
    maps.append(m); want.append("col > 0: rows -4 .. +5 suppressed: the peak 5 rows above survives, 5 below does not")
    m = bg(); m[30, 2] = 5; m[30, 10] = 4.5; m[30, 11] = 4.4; m[31, 1] = 4.3; m[80, 3] = 4.0
    maps.append(m); want.append("picked distance 2: cells with d >= 8 in the same rows survive")
    m = bg(); m[119, 0] = 5; m[0, 3] = 4.9; m[118, 11] = 4.8; m[1, 1] = 4.7; m[117, 9] = 4.6
    maps.append(m); want.append("peaks on both sides of the seam, max at angle 119 col 0: fewer than 5 candidates")
    m = bg(); m[4, 5] = 5; m[5, 5] = 4.9; m[114, 5] = 4.8; m[115, 5] = 4.7; m[64, 0] = 4.6
    maps.append(m); want.append("candidates on both sides of the image 0 / image 11 / image 1 borders (training pointer)")
    return np.stack(maps), want


def main():
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    _stand_ins()
    from tests import waypoint_ref as R
    from vln_bevbert_amd import weights
    from vlnce_baselines.waypoint_pred.TRM_net import BinaryDistPredictor_TRM
    from vlnce_baselines.models import Policy_ViewSelection_BEV as pol
    from vlnce_baselines import ss_trainer_BEV as trn
    from vlnce_baselines.models.utils import angle_feature_torch
    import math

    out = {}
    # ---------------- network
    net = BinaryDistPredictor_TRM(device="cpu")
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    with open(os.path.join(HERE, "waypoint_keys.txt"), "w") as f:
        for k, s in shapes.items():
            f.write(f"{k} {s}\n")
    net.load_state_dict(weights.fill_state_dict(shapes))
    net.eval()
    depth_net = torch.from_numpy(R.synthetic(7, (3 * 12, 128, 4, 4)))
    with torch.no_grad():
        net_logits = net(torch.zeros(3 * 12, 2048, 7, 7), depth_net)
    out["net_depth_seed"] = np.array(7)
    out["net_logits"] = net_logits.numpy()

    # ---------------- maps
    rng = np.random.default_rng(11)
    maps_a = np.stack([(rng.permutation(1440) * 0.01).reshape(120, 12) for _ in range(64)]).astype(np.float32)
    maps_b, want = _hand_maps(rng)
    maps_c = net_logits.numpy()
    logits = torch.from_numpy(np.concatenate([maps_a, maps_b, maps_c]))
    N = logits.shape[0]
    group = np.array([0] * 64 + [1] * len(maps_b) + [2] * 3)
    rgb = torch.from_numpy(R.synthetic(21, (N * 12, 512), ints=True))
    depth = torch.from_numpy(R.synthetic(22, (N * 12, 128, 4, 4), ints=True))

    idx = np.arange(12, dtype=np.int64)
    stand = types.SimpleNamespace(
        depth_encoder=lambda obs: depth, rgb_encoder=lambda obs: (rgb, torch.zeros(1).expand(N, 12, 196, 768)),
        grid_pool_depth=lambda x: torch.zeros(1).expand(N, 12, 196, 1),
        space_pool_rgb=torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((1, 1)), torch.nn.Flatten(start_dim=2)),
        space_pool_depth=torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((1, 1)), torch.nn.Flatten(start_dim=2)),
        pano_img_idxes=idx, pano_angle_fts=angle_feature_torch(torch.from_numpy((1 - idx / 12) * 2 * math.pi)))
    obs = {"rgb": torch.zeros(N, 2, 2, 3), "depth": torch.zeros(N, 2, 2, 1)}

    def run(in_train):
        with torch.no_grad():
            return pol.BEV.forward(stand, mode="waypoint", waypoint_predictor=lambda r, d: logits, observations=obs,
                                   in_train=in_train)

    # the reference keeps batch_output_map local: record it through its own nms
    seen = {}
    real_nms = pol.nms

    def spy(*a, **k):
        seen["map"] = real_nms(*a, **k)
        return seen["map"]
    pol.nms = spy
    wp = run(False)
    pol.nms = real_nms
    omap = seen["map"].squeeze(1)[:, 1:-1, :]
    out["logits"], out["group"] = logits.numpy(), group
    out["hand_notes"] = np.array(want)
    nz = omap.nonzero()
    out["output_map_nz"] = nz.numpy().astype(np.int32)            # (n, 3): sample, angle, dist -- the map is 5-sparse
    out["output_map_val"] = omap[nz[:, 0], nz[:, 1], nz[:, 2]].numpy()
    feat_idx = np.concatenate([np.arange(8), np.arange(64, N)])
    out["feat_idx"] = feat_idx
    out["heat"] = torch.softmax(logits.reshape(N, -1), 1).reshape(N, 120, 12).numpy()[feat_idx]

    def pack(wp, pre):
        cnt = np.array([len(a) for a in wp["cand_angles"]], dtype=np.int32)
        ang, dist = np.zeros((N, 5), np.float32), np.zeros((N, 5), np.float32)
        img, fts = -np.ones((N, 5), np.int32), np.zeros((N, 5, 4), np.float32)
        for b in range(N):
            k = cnt[b]
            ang[b, :k] = np.array(wp["cand_angles"][b], dtype=np.float32)
            dist[b, :k] = np.array(wp["cand_distances"][b], dtype=np.float32)
            img[b, :k] = wp["cand_img_idxes"][b]
            fts[b, :k] = wp["cand_angle_fts"][b].numpy()
        out[pre + "cand_count"], out[pre + "cand_angles"], out[pre + "cand_distances"] = cnt, ang, dist
        out[pre + "cand_img_idx"], out[pre + "cand_angle_fts"] = img, fts
        return cnt

    cnt = pack(wp, "eval_")
    assert cnt[64] == 4 and cnt[65] == 4 and cnt[69] < 5, cnt[64:]
    out["pano_angle_fts"] = wp["pano_angle_fts"].numpy()
    out["pano_rgb"], out["pano_depth"] = wp["pano_rgb"].numpy()[feat_idx], wp["pano_depth"].numpy()[feat_idx]
    vp = trn.RLTrainer._vp_feature_variable(types.SimpleNamespace(envs=types.SimpleNamespace(num_envs=N)), wp)
    out["vp_rgb_fts"], out["vp_dep_fts"] = vp["rgb_fts"].numpy()[feat_idx], vp["dep_fts"].numpy()[feat_idx]
    out["vp_loc_fts"], out["vp_nav_types"] = vp["loc_fts"].numpy(), vp["nav_types"].numpy()
    out["vp_view_lens"] = vp["view_lens"].numpy()

    # (c): the lead of every pick on the reference's own probabilities
    margins = np.array([R.nms_picks(out_p, with_margin=True)[1]
                        for out_p in torch.softmax(logits[-3:].reshape(3, -1), 1).reshape(3, 120, 12).numpy()])
    out["net_margins"] = margins
    assert (margins >= 1e-4).sum() >= 2, margins

    # ---------------- training draw with hand-set cells
    acts = np.array([[(37 * b + 29 * k + 11) % 120 for k in range(5)] for b in range(N)], dtype=np.int64)
    acts[64:, 0], acts[64:, 1] = 0, 119
    probs = np.zeros((N, 5, 120), np.float32)
    state = {"b": 0}

    class Fixed:
        def __init__(self, p):
            probs[state["b"], :p.shape[0]] = p.numpy()
            self.k = p.shape[0]

        def sample(self):
            b = state["b"]
            state["b"] += 1
            return torch.from_numpy(acts[b, :self.k])
    real_cat = torch.distributions.Categorical
    torch.distributions.Categorical = Fixed
    try:
        wpt = run(True)
    finally:
        torch.distributions.Categorical = real_cat
    pack(wpt, "train_")
    out["train_acts"], out["way_heats_probs"] = acts, probs[64:]

    np.savez_compressed(os.path.join(HERE, "waypoint.npz"), **out)
    print("waypoint.npz", os.path.getsize(os.path.join(HERE, "waypoint.npz")), "bytes; counts (b):", cnt[64:71],
          "(c):", cnt[71:], "margins (c):", margins)


if __name__ == "__main__":
    main()
