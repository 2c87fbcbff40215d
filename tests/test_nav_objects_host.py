"""Object-grounding navigation steps without a GPU: the goldens of tests/golden/make_nav_obj_golden.py, the feed builders of
the two navigation runners with object tokens (padded shapes, bucket keys) and without (exactly what they built before),
the host half of ``nav_obj_variable``, the synthetic REVERIE episodes and the C ABI's new declarations."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, load_golden
from vln_bevbert_amd import lib, synthetic
from vln_bevbert_amd.nav_static import NavGraphRunner, NavTrainRunner, _slice_outputs, nav_obj_variable

NEW_ENTRIES = ("bevbert_obj_rows_fwd", "bevbert_obj_rows_bwd", "bevbert_nav_obj_step", "bevbert_nav_obj_pick",
               "bevbert_nav_metrics_obj")


# ------------------------------------------------------------------------------------------------------ goldens
def test_goldens_load_and_hold_the_cases_the_kernels_are_checked_on():
    g = load_golden("nav_obj")
    tgt, ol, ended = g["sup_target"], g["sup_obj_len"], g["sup_ended"].astype(bool)
    cur_on_goal = np.array([c in e[:n] for c, e, n in zip(g["sup_cur"], g["sup_end_vps"], g["sup_n_end"])])
    has_target = np.array([t in ids[:n] for t, ids, n in zip(g["sup_gt_obj"], g["sup_obj_ids"], ol)])
    assert ended.any() and (tgt[ended] == -100).all()                                   # an ended sample
    assert (~ended & ~cur_on_goal).any() and (tgt[~cur_on_goal] == -100).all()          # off the goal set
    lost = ~ended & cur_on_goal & ~has_target & (ol > 0)
    assert lost.any() and (tgt[lost] == -100).all()                                     # on it, target not among its objects
    assert (ol == 0).any() and (tgt[ol == 0] == -100).all()                             # no objects
    assert (tgt >= 0).any() and all(g["sup_obj_ids"][b, t] == g["sup_gt_obj"][b] for b, t in enumerate(tgt) if t >= 0)
    lg = g["sup_obj_logits"]
    assert any(n > 1 and (lg[b, :n] == lg[b, :n].max()).sum() > 1 for b, n in enumerate(ol))     # duplicate arg-max
    assert all(np.isneginf(lg[b, n:]).all() and np.isfinite(lg[b, :n]).all() for b, n in enumerate(ol))
    # _nav_obj_variable: one row ends exactly at L, one has no objects
    vl, vo = g["var_view_lens"], g["var_obj_lens"]
    assert (vl + vo).max() == g["var_pano"].shape[1] and (vo == 0).any() and g["var_obj_embeds"].shape[1] == vo.max()
    assert 0 < g["met_item_success"].mean() < 1 and 0 < g["met_item_rgs"].mean() < 1
    assert (g["met_item_oracle_success"] > g["met_item_success"]).any() and (g["met_pred_obj"] == -1).any()
    assert list(g["met_avg_keys"]) == ["action_steps", "steps", "lengths", "sr", "oracle_sr", "spl", "rgs", "rgspl"]

    m = load_golden("nav_tiny_rvr")
    assert (m["obj_lens"] == 0).any() and m["obj_lens"].max() == m["nav_obj"].shape[1] == m["obj_masks"].shape[1]
    assert np.array_equal(np.isfinite(m["nav_obj"]), m["obj_masks"]) and np.isneginf(m["nav_obj"][~m["obj_masks"]]).all()
    grads = [k[6:] for k in m.files if k.startswith("grad::")]
    assert any(k.startswith("og_head.") for k in grads) and any(".obj_linear." in k for k in grads)
    assert all(float(np.abs(m["grad::" + k]).max()) > 0 for k in grads)
    for f in ("nav_obj.npz", "nav_tiny_rvr.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 512 * 1024, f


def test_the_generator_reproduces_the_committed_goldens(tmp_path):
    """Where the reference is mounted: a fresh run of make_nav_obj_golden.py (its own process: it stubs modules and patches
    torch.Tensor.cuda) gives the committed files -- integers, masks and the reference's fp64 metrics exactly, the fp32
    model outputs up to the rounding of another machine's CPU GEMMs."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_nav_expert_golden as E
    finally:
        sys.path.remove(GOLDEN)
    if not os.path.isdir(E.REF):
        pytest.skip("the reference is not mounted")
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_nav_obj_golden.py"), str(tmp_path)], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("nav_obj", "nav_tiny_rvr"):
        want, got = load_golden(name), np.load(tmp_path / f"{name}.npz")
        assert want.files == got.files, name
        for k in want.files:
            if name == "nav_tiny_rvr" and want[k].dtype == np.float32:
                scale = max(1e-6, float(np.abs(want[k][np.isfinite(want[k])]).max()))
                assert np.array_equal(np.isfinite(want[k]), np.isfinite(got[k])), k
                fin = np.isfinite(want[k])
                assert float(np.abs(want[k][fin] - got[k][fin]).max()) <= 1e-4 * scale, k
            else:
                assert want[k].dtype == got[k].dtype and np.array_equal(want[k], got[k]), (name, k)


# ------------------------------------------------------------------------------------------------------ feed builders
def _pano_batch(B, V, O, D=6, Do=5, objects=True):
    g = torch.Generator().manual_seed(V + O)
    view_lens = torch.tensor([V, V - 1][:B])
    obj_lens = torch.tensor([O, max(0, O - 1)][:B])
    L = int((view_lens + obj_lens).max()) if objects else V
    b = {"view_img_fts": torch.randn(B, V, D, generator=g), "loc_fts": torch.randn(B, L, 7, generator=g),
         "nav_types": torch.ones(B, L, dtype=torch.long), "view_lens": view_lens, "obj_img_fts": None, "obj_lens": None}
    if objects:
        b.update(obj_img_fts=torch.randn(B, O, Do, generator=g), obj_lens=obj_lens)
    return b, L


def _nav_inputs(B=2, G=5, C=3, L=4, H=8, O=None):
    g = torch.Generator().manual_seed(3)
    visited = torch.tensor([[True, True, False, False, True], [True, False, False, True, False]])
    nav = {"txt_embeds": torch.randn(B, L, H, generator=g), "txt_masks": torch.ones(B, L, dtype=torch.bool),
           "gmap_img_embeds": torch.randn(B, G, H, generator=g), "gmap_step_ids": torch.randint(0, 9, (B, G), generator=g),
           "gmap_pos_fts": torch.randn(B, G, 7, generator=g), "gmap_masks": torch.ones(B, G, dtype=torch.bool),
           "gmap_pair_dists": torch.rand(B, G, G, generator=g), "gmap_visited_masks": visited,
           "gmap_visited_masks_cpu": visited.clone(), "bev_fts": torch.randn(B, 9, H, generator=g),
           "bev_pos_fts": torch.randn(B, 9, 3, generator=g), "bev_nav_masks": torch.ones(B, 9, dtype=torch.bool),
           "bev_cand_idxs": torch.randint(0, 9, (B, C), generator=g),
           "gmap_vpids": [[None, "a", "b", "c", "d"], [None, "p", "q", "r", "s"]],
           "bev_cand_vpids": [[None, "b", "d"], [None, "r", "q"]], "obj_embeds": None, "obj_masks": None}
    if O is not None:
        nav.update(obj_embeds=torch.randn(B, O, H, generator=g), obj_masks=torch.ones(B, O, dtype=torch.bool))
    return nav


NAV_NAMES = ["gmap_img_embeds", "gmap_step_ids", "gmap_pos_fts", "gmap_masks", "gmap_pair_dists", "gmap_visited_masks",
             "bev_fts", "bev_pos_fts", "bev_nav_masks", "bev_cand_idxs", "src", "vis_c"]
NAV_SHAPES = {"gmap_img_embeds": (2, 8, 8), "gmap_step_ids": (2, 8), "gmap_pos_fts": (2, 8, 7), "gmap_masks": (2, 8),
              "gmap_pair_dists": (2, 8, 8), "gmap_visited_masks": (2, 8), "bev_cand_idxs": (2, 8)}


@pytest.mark.parametrize("O,Op", [(0, 4), (1, 4), (5, 8)])
def test_object_batches_are_padded_into_buckets_keyed_by_the_object_axis(O, Op):
    """pad 4: 0 objects become one pad step, 1 -> 4, 5 -> 8.  Panorama: obj_img_fts (B, Op, D), loc_fts / nav_types padded
    to V + Op tokens, the key gains Op, the caller's token axis is what the outputs are sliced back to.  Navigation:
    obj_embeds (B, Op, H) / obj_masks (B, Op) join the feeds, the key gains Op, obj_logits is sliced to the caller's O."""
    B, V = 2, 6
    runner = NavGraphRunner(SimpleNamespace(training=False, vln_bert=None), o_step=4)
    batch, L = _pano_batch(B, V, O)
    feeds, shapes, key, L_out = runner._panorama_call(batch)
    assert list(feeds) == ["view_img_fts", "loc_fts", "nav_types", "view_lens", "obj_img_fts", "obj_lens"]
    assert all(feeds[k] is batch[k] for k in feeds)
    assert shapes == {"obj_img_fts": (B, Op, 5), "loc_fts": (B, V + Op, 7), "nav_types": (B, V + Op)}
    assert key == (B, V, 6, Op) and L_out == L
    # both runners hand the padded step to their plumbing under that key and slice what comes back
    pe, pm = torch.zeros(B, V + Op, 8), torch.zeros(B, V + Op, dtype=torch.bool)
    seen = []
    runner._run = lambda key, feeds, fn, shapes=None, static=None: seen.append((key, list(feeds), shapes)) or (pe, pm)
    got = runner.panorama(batch)
    assert seen == [(("panorama", B, V, 6, Op), list(feeds), shapes)] and got[0].shape == (B, L, 8) and got[1].shape == (B, L)
    trainer = NavTrainRunner(SimpleNamespace(training=True, vln_bert=None), None, o_step=4)
    trainer._segment = lambda mode, key, feeds, diff, fn, shapes, names: \
        seen.append((mode, key, list(feeds), diff, shapes, names)) or {"pano_embeds": pe, "pano_masks": pm}
    got = trainer.panorama(batch)
    assert seen[1] == ("panorama", (B, V, 6, Op), list(feeds), (), shapes, ("pano_embeds", "pano_masks"))
    assert got[0].shape == (B, L, 8) and got[1].shape == (B, L)

    nav = _nav_inputs(O=O)
    for with_text in (False, True):
        feeds, shapes, key, sizes = runner._navigation_call(nav, with_text=with_text)
        assert list(feeds) == (["txt_embeds", "txt_masks"] if with_text else []) + NAV_NAMES + ["obj_embeds", "obj_masks"]
        assert feeds["obj_embeds"] is nav["obj_embeds"] and feeds["obj_masks"] is nav["obj_masks"]
        assert shapes == dict(NAV_SHAPES, obj_embeds=(2, Op, 8), obj_masks=(2, Op))
        assert key == (2, 8, 8, 4, 9, Op) and sizes == (5, 3)
    out = {"gmap_embeds": torch.zeros(2, 8, 8), "global_logits": torch.zeros(2, 8), "local_logits": torch.zeros(2, 8),
           "fused_logits": torch.zeros(2, 8), "obj_logits": torch.zeros(2, Op)}
    seen.clear()
    runner._text_inputs = lambda *a: {}
    runner._run = lambda key, feeds, *a: seen.append(key) or out
    got = runner.navigation(nav)
    assert seen == [("navigation", 2, 8, 8, 4, 9, Op)] and got["obj_logits"].shape == (2, O)
    nav["txt_embeds"].requires_grad_(True)
    nav["obj_embeds"].requires_grad_(True)
    trainer._segment = lambda mode, key, feeds, diff, fn, shapes, names: seen.append((mode, key, diff, names)) or out
    got = trainer.navigation(nav)
    assert seen[1] == ("navigation", (2, 8, 8, 4, 9, Op, ("txt_embeds", "obj_embeds")), ("txt_embeds", "obj_embeds"),
                       ("gmap_embeds", "global_logits", "local_logits", "fused_logits", "obj_logits"))
    assert got["obj_logits"].shape == (2, O) and got["fused_logits"].shape == (2, 5)


def test_batches_without_objects_build_the_feeds_and_keys_they_always_built():
    runner = NavGraphRunner(SimpleNamespace(training=False, vln_bert=None))
    batch, _ = _pano_batch(2, 6, 0, objects=False)
    feeds, shapes, key, L = runner._panorama_call(batch)
    assert list(feeds) == ["view_img_fts", "loc_fts", "nav_types", "view_lens"] and all(feeds[k] is batch[k] for k in feeds)
    assert shapes == {} and key == (2, 6, 6) and L is None
    seen = []
    pe, pm = torch.zeros(2, 6, 8), torch.zeros(2, 6, dtype=torch.bool)
    runner._run = lambda key, feeds, fn, shapes=None, static=None: seen.append((key, list(feeds), shapes)) or (pe, pm)
    got = runner.panorama(batch)
    assert seen == [(("panorama", 2, 6, 6), list(feeds), {})] and got[0] is pe and got[1] is pm
    nav = _nav_inputs()
    for with_text in (False, True):
        feeds, shapes, key, sizes = runner._navigation_call(nav, with_text=with_text)
        assert list(feeds) == (["txt_embeds", "txt_masks"] if with_text else []) + NAV_NAMES
        assert shapes == NAV_SHAPES and key == (2, 8, 8, 4, 9) and sizes == (5, 3)
    out = {"gmap_embeds": torch.zeros(2, 8, 8), "global_logits": torch.zeros(2, 8), "local_logits": torch.zeros(2, 8),
           "fused_logits": torch.zeros(2, 8)}
    got = _slice_outputs(out, 5, 3)
    assert list(got) == ["gmap_embeds", "global_logits", "local_logits", "fused_logits", "obj_logits"]
    assert got["obj_logits"] is None
    trainer = NavTrainRunner(SimpleNamespace(training=True, vln_bert=None), None)
    nav["txt_embeds"].requires_grad_(True)
    trainer._segment = lambda mode, key, feeds, diff, fn, shapes, names: seen.append((mode, key, list(feeds), names)) or out
    trainer.navigation(nav)
    assert seen[-1] == ("navigation", (2, 8, 8, 4, 9, ("txt_embeds",)), ["txt_embeds", "txt_masks"] + NAV_NAMES,
                        ("gmap_embeds", "global_logits", "local_logits", "fused_logits"))


def test_nav_obj_variable_refuses_lengths_that_do_not_fit_before_any_launch():
    pano = torch.zeros(2, 6, 8)
    for vl, ol in (([4, 5], [2, 2]), ([4, -1], [1, 1]), ([4, 4], [1])):
        with pytest.raises(lib.BevBertHipError, match="do not fit"):
            nav_obj_variable(pano, torch.tensor(vl), torch.tensor(ol))
    with pytest.raises(lib.BevBertHipError, match="multiple of 4"):
        nav_obj_variable(torch.zeros(2, 6, 6), torch.tensor([4, 4]), torch.tensor([1, 1]))
    with pytest.raises(lib.BevBertHipError, match="device memory only"):          # fits: the launch is what refuses the CPU
        nav_obj_variable(pano, torch.tensor([4, 4]), torch.tensor([2, 1]))


def test_synthetic_episodes_gain_object_fields_and_keep_their_walks():
    plain, ended = synthetic.make_nav_episodes(3, 5, seed=4)
    objs, ended2 = synthetic.make_nav_episodes(3, 5, seed=4, objects=5)
    assert all(np.array_equal(a, b) for a, b in zip(ended, ended2))
    extra = {"obj_ids", "gt_obj_id", "gt_end_vps"}
    for step, step2 in zip(plain, objs):
        for ob, ob2 in zip(step, step2):
            assert set(ob2) - set(ob) == extra and all(ob[k] == ob2[k] for k in ob)
            assert len(ob2["obj_ids"]) <= 5 and len(set(ob2["obj_ids"])) == len(ob2["obj_ids"])
            assert (ob2["gt_obj_id"] in ob2["obj_ids"]) == (ob2["viewpoint"] in ob2["gt_end_vps"])
    assert all(ob["viewpoint"] in ob["gt_end_vps"] for ob in objs[0])          # the start viewpoint shows the target
    seen = {}
    for step in objs:
        for ob in step:
            assert seen.setdefault(ob["viewpoint"], ob["obj_ids"]) == ob["obj_ids"]


def test_the_header_declares_the_object_grounding_entries_and_the_library_exports_them():
    protos = lib.prototypes()
    assert all(n in protos for n in NEW_ENTRIES)
    assert len(protos["bevbert_obj_rows_fwd"][1]) == 11 and len(protos["bevbert_nav_obj_step"][1]) == 17
    if os.path.exists(lib.LIB_PATH):
        l = lib.load()
        assert l.bevbert_version() >= 400
        N = None
        # argument checks answer before any launch
        assert l.bevbert_obj_rows_fwd(N, N, N, N, N, 1, 4, 4, 6, 0, N) == -1 and b"multiple of 4" in l.bevbert_last_error()
        assert l.bevbert_obj_rows_bwd(N, N, N, N, 1, 4, 4, 8, 0, N) == -1 and b"null pointer" in l.bevbert_last_error()
        assert l.bevbert_nav_obj_step(N, 2, 1, 4, N, N, N, N, N, N, 1, N, N, 4, N, N, N) == -1
        assert b"dtype 2 unsupported" in l.bevbert_last_error()
        assert l.bevbert_nav_obj_pick(N, N, N, 0, N, 1, N) == -1 and l.bevbert_nav_metrics_obj(
            N, 4, 1, N, N, N, 4, N, N, N, 4, N, N, 0, N, N, 1, N, N, N) == -1
