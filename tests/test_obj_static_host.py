"""CPU tests of the static object-token batches (static_step.StaticBatch with ``obj_static=True``; ``plan`` needs no
device) and of the C-ABI surface of the kernels that go with them (no compute calls).

The object-token index math of vilmodel.GlocalTextPathCMT._obj_tokens is restated here from traj_step_lens and the two
length vectors and evaluated on the UNPADDED batch; the loader-built tables must select the same rows of the padded one."""
import numpy as np
import pytest
import torch

from tests.obj_static_cases import CFG, SEED_A, SEED_B, SEED_OTHER_WIDTH, SHAPES_A, SHAPES_B, make
from vln_bevbert_amd import lib, static_step, synthetic
from vln_bevbert_amd.config import BevBertConfig
from vln_bevbert_amd.static_step import StaticBatch

def obj_tokens_today(traj, batch):
    """_obj_tokens' index math on the unpadded (T, L, H) states: (B, O, H) zero-padded tokens and the (B, O) mask."""
    ends = torch.from_numpy(np.cumsum(batch["traj_step_lens"]) - 1)
    ol_host = batch["traj_vp_obj_lens"].tolist()
    O = max(1, max(ol_host[e] for e in ends.tolist()))
    vl, ol = batch["traj_vp_view_lens"][ends], batch["traj_vp_obj_lens"][ends]
    j = torch.arange(O)[None, :]
    valid = j < ol[:, None]
    idx = torch.where(valid, vl[:, None] + j, torch.zeros_like(j))
    rows = traj[ends]
    obj = torch.gather(rows, 1, idx[..., None].expand(-1, -1, rows.shape[2]))
    return obj * valid[..., None].to(obj.dtype), valid


@pytest.mark.parametrize("seed,shapes", [(SEED_A, SHAPES_A), (SEED_B, SHAPES_B), (SEED_OTHER_WIDTH, SHAPES_B)])
@pytest.mark.parametrize("task", ["mrc", "og", "sap", "mlm"])
def test_object_tables_select_the_rows_of_todays_index_math(task, seed, shapes):
    batch = make(seed, task, shapes)
    host = StaticBatch.plan(CFG, task, batch, obj_static=True)
    st, padded = host["static"], host["padded"]
    T0, L0 = batch["traj_loc_fts"].shape[:2]
    Tp, Lp = padded["traj_loc_fts"].shape[:2]
    assert Tp % static_step.PANO_PAD == 0 and Lp % static_step.VIEW_PAD == 0 and Tp >= T0 and Lp >= L0
    assert padded["traj_nav_types"].shape == (Tp, Lp)
    assert padded["traj_obj_img_fts"].shape[0] == Tp and padded["traj_obj_img_fts"].shape[1] % static_step.OBJ_PAD == 0
    assert padded["traj_view_img_fts"].shape[0] == Tp and padded["traj_view_img_fts"].shape[1] % static_step.VIEW_PAD == 0
    # dummy panoramas: one view, no object, and no CSR segment refers to them
    assert padded["traj_vp_view_lens"][T0:].tolist() == [1] * (Tp - T0)
    assert padded["traj_vp_obj_lens"][T0:].tolist() == [0] * (Tp - T0)
    rowptr, idx, w, n_src = host["csr"]
    assert n_src == Tp * Lp and (not idx or max(idx) < T0 * Lp)
    # the panorama masks cover the joint axis
    lens = padded["traj_vp_view_lens"] + padded["traj_vp_obj_lens"]
    assert torch.equal(st["pano_masks"], torch.arange(Lp)[None, :] < lens[:, None])
    assert torch.equal(st["pano_km_inf"] == 0, st["pano_masks"]) and torch.equal(st["pano_km"] == 0, st["pano_masks"])
    # random states on the unpadded layout, copied into the padded one
    H = 8
    g = torch.Generator().manual_seed(seed)
    traj = torch.randn(T0, L0, H, generator=g)
    full = torch.randn(Tp, Lp, H, generator=g)
    full[:T0, :L0] = traj
    want, want_valid = obj_tokens_today(traj, batch)
    B, Op = st["obj_valid"].shape
    assert Op % static_step.OBJ_PAD == 0 and Op >= want.shape[1] and st["obj_rows"].shape == (B * Op,)
    assert st["obj_rows"].dtype == torch.int64 and st["obj_valid"].dtype == torch.bool
    got = full.reshape(-1, H).index_select(0, st["obj_rows"]).view(B, Op, H) * st["obj_valid"][..., None].to(full.dtype)
    O0 = want.shape[1]
    assert torch.equal(got[:, :O0], want) and torch.equal(st["obj_valid"][:, :O0], want_valid)
    assert not bool(st["obj_valid"][:, O0:].any()) and float(got[:, O0:].abs().sum()) == 0.0
    assert bool((st["obj_rows"].view(B, Op)[~st["obj_valid"]] == 0).all())
    assert float(want.abs().sum()) > 0


@pytest.mark.parametrize("seed,shapes", [(SEED_A, SHAPES_A), (SEED_B, SHAPES_B)])
def test_mrc_rows_are_the_masked_objects_in_order(seed, shapes):
    batch = make(seed, "mrc", shapes)
    host = StaticBatch.plan(CFG, "mrc", batch, obj_static=True)
    st, padded = host["static"], host["padded"]
    mask, probs = batch["vp_obj_mrc_masks"], batch["vp_obj_probs"]
    B, O0 = mask.shape
    pm, pp = padded.get("vp_obj_mrc_masks", mask), padded.get("vp_obj_probs", probs)
    Op = st["obj_valid"].shape[1]
    assert pm.shape == (B, Op) and pp.shape == (B, Op, CFG.obj_prob_size)
    assert torch.equal(pm[:, :O0], mask) and not bool(pm[:, O0:].any()) and torch.equal(pp[:, :O0], probs)
    n = int(mask.sum())
    assert st["mrc_n"] == n and n > 0
    npad = st["mrc_pos"].numel()
    assert npad % static_step.MRC_ROW_PAD == 0 and npad >= n and st["mrc_tpos"].numel() == npad == st["mrc_valid"].numel()
    assert st["mrc_valid"].dtype == torch.float32
    assert st["mrc_valid"].tolist() == [1.0] * n + [0.0] * (npad - n)
    assert st["mrc_pos"][n:].tolist() == [0] * (npad - n) and st["mrc_tpos"][n:].tolist() == [0] * (npad - n)
    # the selected rows, in the order of the boolean index of the reference (row-major over the unpadded mask)
    H = 6
    obj = torch.randn(B, Op, H, generator=torch.Generator().manual_seed(3))
    assert torch.equal(obj.reshape(-1, H).index_select(0, st["mrc_pos"][:n]), obj[:, :O0][mask])
    assert torch.equal(pp.reshape(-1, pp.shape[-1]).index_select(0, st["mrc_tpos"][:n]), probs[mask])
    assert bool(st["obj_valid"].reshape(-1)[st["mrc_pos"][:n]].all())          # a masked object is a real object


@pytest.mark.parametrize("task", ["mlm", "mrc", "sap", "og"])
def test_batches_with_other_step_and_object_counts_share_a_bucket(task):
    a, b, wide = make(SEED_A, task, SHAPES_A), make(SEED_B, task, SHAPES_B), make(SEED_OTHER_WIDTH, task, SHAPES_B)
    assert a["traj_step_lens"] != b["traj_step_lens"]
    assert a["traj_vp_obj_lens"].tolist() != b["traj_vp_obj_lens"].tolist()
    sa, sb, sw = (StaticBatch.plan(CFG, task, x, obj_static=True)["signature"] for x in (a, b, wide))
    assert sa == sb
    assert sw != sa and sw[5][2] != sa[5][2]                    # the padded joint width differs
    many = StaticBatch.plan(CFG, task, make(SEED_A, task, SHAPES_A, max_objects=12), obj_static=True)["signature"]
    assert many != sa and many[5][2] > sa[5][2]                 # more objects per panorama: a wider joint axis, another bucket
    # task, B, padded text shape, (Tp, Vp, feature width), G, ("obj", object axis, joint width, O_p, classes) [, rows / K]
    assert sa[0] == task and sa[1] == 3 and sa[2] == (3, 80) and sa[3] == (32, 40, 768) and sa[5][0] == "obj"
    assert sa[5][1] % static_step.OBJ_PAD == 0 and sa[5][3] % static_step.OBJ_PAD == 0 and sa[5][4] == CFG.obj_prob_size
    assert tuple(a["traj_step_lens"]) not in sa[5] and all(isinstance(x, (int, str)) for x in sa[5])      # no step counts
    assert len(sa) == (6 if task == "og" else 7)
    if task == "mrc":
        assert sa[6] == static_step.MRC_ROW_PAD
    if task == "mlm":
        assert sa[6] % static_step.MLM_ROW_PAD == 0


def test_without_the_keyword_the_layout_is_todays():
    a = make(SEED_A, "sap")
    host = StaticBatch.plan(CFG, "sap", a)
    assert host["signature"] == ("sap", 3, (3, 80), tuple(a["traj_view_img_fts"].shape), 20,
                                 ("obj", tuple(a["traj_obj_img_fts"].shape), (5, 2, 4), a["traj_loc_fts"].shape[1]), 5)
    assert not any(k.startswith("traj_") for k in host["padded"])
    assert "obj_rows" not in host["static"] and "pano_masks" not in host["static"]
    assert host["signature"] == StaticBatch.plan(CFG, "sap", a, obj_static=False)["signature"]
    assert StaticBatch(CFG, "sap", a, "cpu").capturable is False
    assert StaticBatch(CFG, "sap", a, "cpu", obj_static=True).capturable is True
    # a batch without objects does not change with the keyword
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    r2r = synthetic.make_batch(cfg, "sap", 3, seed=60, ragged=True, sems_as="ids")
    h0, h1 = StaticBatch.plan(cfg, "sap", r2r), StaticBatch.plan(cfg, "sap", r2r, obj_static=True)
    assert h0["signature"] == h1["signature"] and h0["padded"].keys() == h1["padded"].keys()
    assert all(torch.equal(h0["static"][k], h1["static"][k]) for k in h0["static"] if torch.is_tensor(h0["static"][k]))


def test_bucket_manager_passes_the_keyword_through():
    from vln_bevbert_amd.loader import BucketManager
    mgr = BucketManager(CFG, "cpu", obj_static=True)
    sb = mgr.acquire("mrc", make(SEED_A, "mrc"))
    assert sb.capturable and sb.obj_static and "mrc_pos" in sb.tensors["_static"]
    mgr.release(sb)
    sb2 = mgr.acquire("mrc", make(SEED_B, "mrc", SHAPES_B))
    assert mgr.stats["buckets_created"] == 1 and sb2.signature == sb.signature
    assert BucketManager(CFG, "cpu").acquire("mrc", make(SEED_A, "mrc")).capturable is False


def test_max_objects_is_default_preserving():
    def sample(**kw):
        return synthetic.make_sample(np.random.default_rng(5), 0, CFG, 3, 40, ragged_views=True, **kw)
    a, b = sample(), sample(max_objects=None)
    assert a["traj_vp_obj_lens"] == b["traj_vp_obj_lens"] and np.array_equal(a["vp_obj_probs"], b["vp_obj_probs"])
    lens = [n for s in range(8) for n in synthetic.make_sample(np.random.default_rng(s), 0, CFG, 5, 40, ragged_views=True,
                                                              max_objects=20)["traj_vp_obj_lens"]]
    assert max(lens) > 4 and max(lens) <= 20


# ----------------------------------------------------------------------------- the C-ABI surface of the new kernels
NEW_ENTRIES = ("bevbert_soft_ce_fwd", "bevbert_soft_ce_bwd", "bevbert_val_kl_rows")


def test_new_entries_are_declared_and_answer_without_a_launch():
    assert set(NEW_ENTRIES) <= set(lib.prototypes()) and "sap_loss.hip" in lib.SOURCES and "val_metrics.hip" in lib.SOURCES
    lib.build()
    l = lib.load()
    N = None
    rows = [("soft_ce: dtype %d unsupported", lambda dt, r=1: l.bevbert_soft_ce_fwd(N, N, N, N, N, r, 4, dt, N)),
            ("soft_ce: dtype %d unsupported", lambda dt, r=1: l.bevbert_soft_ce_bwd(N, N, N, N, N, N, r, 4, dt, N)),
            ("val_kl_rows: dtype %d unsupported", lambda dt, r=1: l.bevbert_val_kl_rows(N, 4, N, N, N, r, 4, dt, N, N, N))]
    for msg, f in rows:
        for dt in (2, 3, -1):
            rc = f(dt)
            assert rc == -3 and msg % dt in l.bevbert_last_error().decode(), (msg, dt, rc, l.bevbert_last_error())
        assert f(2, 0) == 0 and f(0, 0) == 0                       # no rows: 0, before the dtype is looked at
    # C < 1 and a misaligned base are argument errors
    assert l.bevbert_soft_ce_fwd(N, N, N, N, N, 1, 0, 0, N) == -1 and b"soft_ce: C=0" in l.bevbert_last_error()
    assert l.bevbert_soft_ce_bwd(N, N, N, N, N, N, 1, 0, 0, N) == -1 and b"soft_ce: C=0" in l.bevbert_last_error()
    assert l.bevbert_soft_ce_fwd(8, N, N, N, N, 1, 4, 0, N) == -1 and b"16-byte aligned" in l.bevbert_last_error()
    assert l.bevbert_soft_ce_bwd(16, N, N, N, N, 8, 1, 4, 0, N) == -1 and b"16-byte aligned" in l.bevbert_last_error()
    # a NULL tensor with rows to do and a dtype that has a kernel never reaches a launch
    for dt in (0, 1):
        assert l.bevbert_soft_ce_fwd(N, N, N, N, N, 1, 4, dt, N) == -1 and b"soft_ce_fwd: null tensor" in l.bevbert_last_error()
        assert l.bevbert_soft_ce_bwd(N, N, N, N, N, N, 1, 4, dt, N) == -1 and b"soft_ce_bwd: null tensor" in l.bevbert_last_error()
        assert l.bevbert_val_kl_rows(N, 4, N, N, N, 1, 4, dt, N, N, N) == -1 and b"val_kl_rows: null tensor" in l.bevbert_last_error()
    assert l.bevbert_val_kl_rows(N, 3, N, N, N, 1, 4, 0, N, N, N) == -1 and b"val_kl_rows: R=1 C=4 ld=3" in l.bevbert_last_error()
