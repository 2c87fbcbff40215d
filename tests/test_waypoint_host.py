"""The CPU restatement of the CE waypoint stage (tests/waypoint_ref.py) against the reference's recorded behaviour
(tests/golden/waypoint.npz, made by tests/golden/make_waypoint_golden.py from the reference's own mode 'waypoint', nms
and _vp_feature_variable), and WaypointPredictor's state_dict against the reference module's key / shape list."""
import os

import numpy as np
import pytest

from tests import waypoint_ref as R
from tests.helpers import read_shapes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "waypoint.npz"))


@pytest.fixture(scope="module")
def inputs(gold):
    n = gold["logits"].shape[0]
    return R.synthetic(21, (n * 12, 512), ints=True), R.synthetic(22, (n * 12, 128, 4, 4), ints=True)


@pytest.fixture(scope="module")
def ours(gold, inputs):
    return R.stage(gold["logits"], *inputs)


def _close(a, b, tol=1e-6):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max(initial=0.0)) <= tol


def test_golden_covers_the_cases_the_stage_is_specified_on(gold):
    g = gold["group"]
    assert (g == 0).sum() >= 64 and (g == 1).sum() >= 6 and (g == 2).sum() == 3
    cnt = gold["eval_cand_count"]
    assert (cnt[g == 1] < 5).any() and (cnt == 5).any()
    assert (gold["net_margins"] >= 1e-4).sum() >= 2


def test_restatement_reproduces_the_recorded_eval_outputs(gold, ours):
    assert (ours["cand_count"] == gold["eval_cand_count"]).all()
    nz = gold["output_map_nz"]
    want = [[] for _ in range(len(ours["cand_count"]))]
    for b, a, d in nz:
        want[b].append((int(a), int(d)))
    for b, w in enumerate(want):
        k = ours["cand_count"][b]
        assert list(zip(ours["cand_angle_idx"][b, :k].tolist(), ours["cand_dist_idx"][b, :k].tolist())) == w, b
    vals = ours["heat"][nz[:, 0], nz[:, 1], nz[:, 2]]
    _close(vals, gold["output_map_val"])
    assert (ours["cand_img_idx"] == gold["eval_cand_img_idx"]).all()
    for k in ("cand_angle_fts", "cand_angles", "cand_distances"):
        _close(ours[k], gold["eval_" + k])
    _close(ours["heat"][gold["feat_idx"]], gold["heat"])


def test_restatement_reproduces_the_recorded_panorama_inputs(gold, ours):
    L = gold["vp_nav_types"].shape[1]
    assert (ours["view_lens"] == gold["vp_view_lens"]).all() and L == gold["vp_view_lens"].max() <= R.L_PAD
    assert (ours["nav_types"][:, :L] == gold["vp_nav_types"]).all() and not ours["nav_types"][:, L:].any()
    _close(ours["loc_fts"][:, :L], gold["vp_loc_fts"])
    f = gold["feat_idx"]
    _close(ours["pano_rgb"][f], gold["pano_rgb"])
    _close(ours["pano_depth"][f], gold["pano_depth"])
    _close(ours["rgb_fts"][f][:, :L], gold["vp_rgb_fts"])
    _close(ours["dep_fts"][f][:, :L], gold["vp_dep_fts"])
    _close(R.pano_angle_fts().numpy(), gold["pano_angle_fts"])


def test_restatement_reproduces_the_recorded_hand_set_draws(gold, inputs):
    got = R.stage(gold["logits"], acts=gold["train_acts"])
    assert (got["cand_count"] == gold["train_cand_count"]).all()
    assert (got["cand_img_idx"] == gold["train_cand_img_idx"]).all()
    for k in ("cand_angle_fts", "cand_angles", "cand_distances"):
        _close(got[k], gold["train_" + k])
    _close(got["region_probs"][64:], gold["way_heats_probs"])
    # Q4 is in the recording: some candidate of image 0 first found at an angle >= 115 was drawn at an angle < 10
    a0, a1 = R.stage(gold["logits"])["cand_angle_idx"], got["cand_angle_idx"]
    assert ((a0 >= 115) & (a1 >= 0) & (a1 < 10)).any()


def test_inverse_cdf_picks_the_first_cell_above_the_draw():
    p = np.array([0.25, 0.0, 0.5, 0.25])
    assert [R.inverse_cdf(p, u)[0] for u in (0.0, 0.2499, 0.25, 0.7499, 0.75, 0.9999)] == [0, 0, 2, 2, 3, 3]


def test_waypoint_predictor_has_the_reference_state_dict():
    from vln_bevbert_amd import WaypointPredictor
    want = read_shapes("waypoint_keys.txt")
    m = WaypointPredictor()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert list(got) == list(want)                      # same order too
    assert not any(p.requires_grad for p in m.parameters()) and not m.training
    m.train()
    with pytest.raises(RuntimeError):
        m(None, None)
