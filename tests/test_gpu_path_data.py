"""R2R pre-training from device-resident tables on the MI355X: the panorama gather (csrc/path_data.hip) against a numpy
gather, StaticBatch by reference against the host-collated route, training steps on both routes, and PathBatchSource
through the streaming loader.  The fixture is the one of test_path_data_host.py (golden path_data.npz); its view features
encode (store row, view) in channels 0 and 1, so a gathered tensor says where every row came from."""
import numpy as np
import pytest
import torch

from vln_bevbert_amd import path_data as pd
from vln_bevbert_amd.config import BevBertConfig

from . import path_data_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOCAB = 400


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib
    lib.load()
    return True


# ----------------------------------------------------------------------------- the kernel
def small_table(Vmax_rows):
    """A 5-row PanoTable cut from the fixture's: row 0 is the 37-token panorama, row 4 a single-candidate viewpoint."""
    full, g = C.tables().pano, C.gold()
    first, last = full.row[str(g["shared_view_key"])], full.row[str(g["single_cand_key"])]
    pick = [first] + [r for r in range(len(full.keys)) if r not in (first, last)][:Vmax_rows - 2] + [last]
    return pd.PanoTable([full.keys[r] for r in pick], full.view_order[pick], full.n_tokens[pick], full.loc_fts[pick],
                        full.nav_types[pick], full.cand_ids[pick])


def numpy_gather(fts, table, rows, Vp, D):
    Tp, L = len(rows), table.loc_fts.shape[2]
    img, loc = np.zeros((Tp, Vp, D), np.float32), np.zeros((Tp, Vp, L), np.float32)
    nav, lens = np.zeros((Tp, Vp), np.int64), np.ones(Tp, np.int64)
    for t, r in enumerate(rows):
        if r < 0:
            continue
        n = int(table.n_tokens[r])
        img[t, :n] = fts[r, table.view_order[r, :n], :D].astype(np.float32)
        loc[t, :n], nav[t, :n], lens[t] = table.loc_fts[r, :n], table.nav_types[r, :n], n
    return img, loc, nav, lens


def run_gather(store, table, rows, Vp, D, fill=None):
    from vln_bevbert_amd.feature_store import pano_rows
    Tp, L = len(rows), table.loc_fts.shape[2]
    mk = lambda shape, dt: torch.full(shape, -7 if fill is None else fill, dtype=dt, device=DEV)
    out = mk((Tp, Vp, D), torch.float32), mk((Tp, Vp, L), torch.float32), mk((Tp, Vp), torch.int64), mk((Tp,), torch.int64)
    rows = np.asarray(rows, dtype=np.int32)
    pano_rows(store, table, rows, torch.from_numpy(rows).to(DEV), *out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D,Ds", [(512, 512), (512, 1512), (24, 28), (20, 24)])
def test_pano_gather_equals_a_numpy_gather(env, D, Ds):
    """N = 5 viewpoints, Tp = 3 with one dummy row, the 37-token panorama at Vp = 40.  D = 512 takes the 16-byte path on
    both strides; D = 24 of Ds = 28 has view rows that do not start on 16 bytes (vector path off, every element through
    the scalar tail); D = 20 of Ds = 24 mixes two 16-byte pieces with a 4-element tail.  fp16 -> fp32 is exact."""
    from vln_bevbert_amd.feature_store import ViewFeatureStore
    table = small_table(5)
    fts = C.view_features(Ds, n_keys=5, seed=11)
    store = ViewFeatureStore(table.keys, fts, DEV)
    rows = [0, -1, 4]
    assert table.n_tokens[0] == 37 and len(store) == 5
    got = run_gather(store, table, rows, 40, D)
    want = numpy_gather(fts, table, rows, 40, D)
    for name, a, b in zip(("img", "loc", "nav", "lens"), got, want):
        assert torch.equal(a.cpu(), torch.from_numpy(b)), (name, D, Ds)
    assert got[3].tolist() == [37, 1, int(table.n_tokens[4])]
    assert np.array_equal(want[0][0, :37, 1], table.view_order[0, :37])          # the rows are the table's view order
    # an exact fit of the view axis, every row real, more than one block of work
    rows = [3, 2, 1, 0, 4, 0]
    got = run_gather(store, table, rows, 37, D)
    for a, b in zip(got, numpy_gather(fts, table, rows, 37, D)):
        assert torch.equal(a.cpu(), torch.from_numpy(b))


def test_pano_gather_refuses_bad_rows_and_a_narrow_view_axis_before_any_launch(env):
    from vln_bevbert_amd.feature_store import ViewFeatureStore
    table = small_table(5)
    store = ViewFeatureStore(table.keys, C.view_features(16, n_keys=5, seed=11), DEV)
    for rows, Vp, err in (([0, 5], 40, IndexError), ([-2, 1], 40, IndexError), ([0, 1], 36, ValueError)):
        from vln_bevbert_amd.feature_store import pano_rows
        outs = [torch.full(s, -7, dtype=dt, device=DEV) for s, dt in
                (((2, Vp, 16), torch.float32), ((2, Vp, 7), torch.float32), ((2, Vp), torch.int64), ((2,), torch.int64))]
        r = np.asarray(rows, dtype=np.int32)
        with pytest.raises(err):
            pano_rows(store, table, r, torch.from_numpy(r).to(DEV), *outs)
        torch.cuda.synchronize()
        assert all(bool((o == -7).all()) for o in outs)            # nothing was launched
    other = pd.PanoTable(table.keys[::-1], table.view_order, table.n_tokens, table.loc_fts, table.nav_types)
    with pytest.raises(ValueError, match="same viewpoints"):
        run_gather(store, other, [0], 40, 16)
    run_gather(store, table, [1, -1], 36, 16)                       # 36 views are enough for these


# ----------------------------------------------------------------------------- StaticBatch by reference
@pytest.fixture(scope="module")
def world(env):
    """cfg, twin (tokens folded into the tiny vocabulary), tables, view store (Ds > image_feat_size) and a grid store
    over the viewpoints the fixture's paths visit."""
    from vln_bevbert_amd.feature_store import GridFeatureStore, ViewFeatureStore
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=VOCAB)
    data = C.data(cfg.image_feat_size, cfg.image_feat_size + 8, VOCAB)
    tab = C.tables()
    keys = [str(k) for k in C.gold()["keys"]]
    view_store = ViewFeatureStore(keys, C.view_features(cfg.image_feat_size + 8), DEV)
    gkeys = sorted({f"{it['scan']}_{vp}" for it in data.items for vp in it["path"]})
    g = torch.Generator(device=DEV).manual_seed(5)
    N, P = len(gkeys), cfg.grid_views * cfg.grid_hw ** 2
    depths = torch.rand(N, cfg.grid_views, cfg.grid_hw, cfg.grid_hw, generator=g, device=DEV) * 0.5
    grid = GridFeatureStore(gkeys, torch.randn(N, P, cfg.grid_feat_size, generator=g, device=DEV).half(), depths,
                            torch.randint(0, cfg.sem_classes, (N, P), generator=g, device=DEV).to(torch.uint8), DEV)
    return dict(cfg=cfg, data=data, tab=tab, view_store=view_store, grid=grid)


def both_routes(w, task, idxs, ends, seed):
    """(host-collated batch, by-reference batch, grid keys) of the same prefixes with the same mask draws."""
    data, tab = w["data"], w["tab"]
    rng = np.random.default_rng(seed)
    full = [data.get_input(int(i), int(e)) for i, e in zip(idxs, ends)]
    ref = [tab.sample(data, int(i), int(e), panos=False) for i, e in zip(idxs, ends)]
    labels = masks = None
    if task == "mlm":
        labels = []
        for a, b in zip(full, ref):
            ids = a["instr_encoding"]
            toks, lab = pd.mask_tokens(rng.random(len(ids)), rng.integers(104, VOCAB, size=len(ids)), ids)
            a["instr_encoding"] = b["instr_encoding"] = toks
            labels.append(lab)
    elif task == "masksem":
        masks = [pd.bev_mrc_masks(rng.random(441), 0.15, rng.integers(441)) for _ in full]
    return (pd.collate(task, full, 21, txt_labels=labels, mrc_masks=masks),
            pd.collate(task, ref, 21, txt_labels=labels, mrc_masks=masks), [s["grid_key"] for s in full])


def assert_same_batch(a, b, where):
    """Every tensor, every list and every _static entry of two StaticBatches (a: host route, b: by reference)."""
    assert a.signature == b.signature, where
    ta, tb = a.tensors, b.tensors
    assert set(tb) - set(ta) == {"pano_rows"} and set(ta) <= set(tb), (where, set(ta) ^ set(tb))
    for k, v in ta.items():
        if torch.is_tensor(v):
            assert v.dtype == tb[k].dtype and torch.equal(v.cpu(), tb[k].cpu()), (where, k)
        elif k == "_static":
            assert set(v) == set(tb[k]), where
            for n, x in v.items():
                y = tb[k][n]
                assert (torch.equal(x.cpu(), y.cpu()) and x.dtype == y.dtype) if torch.is_tensor(x) else x == y, (where, n)
        elif k == "gmap_csr":
            for n in ("rowptr", "idx", "w"):
                x, y = getattr(v[0], n, None), getattr(tb[k][0], n, None)
                if torch.is_tensor(x):
                    assert torch.equal(x.cpu(), y.cpu()), (where, n)
            assert v[1] == tb[k][1]
        elif k != "grid_store":
            assert v == tb[k], (where, k)


IDXS = np.array([6, 7, 0, 9])            # the 37-token start, the single-candidate end, a 2-node path, the 24-node walk
ENDS = np.array([2, 4, 0, 22])           # ... cut at 23 nodes: truncated to 20 + 1 panoramas


@pytest.mark.parametrize("task", ["mlm", "sap", "masksem"])
def test_static_batch_by_reference_equals_the_host_route(world, task):
    from vln_bevbert_amd.static_step import StaticBatch
    w = world
    host, ref, keys = both_routes(w, task, IDXS, ENDS, seed=1)
    assert "traj_view_img_fts" in host and "traj_view_img_fts" not in ref and ref["pano_rows"].dtype == torch.int32
    a = StaticBatch(w["cfg"], task, host, DEV, grid_store=w["grid"], grid_keys=keys)
    b = StaticBatch(w["cfg"], task, ref, DEV, grid_store=w["grid"], grid_keys=keys, view_store=w["view_store"],
                    pano_table=w["tab"].pano)
    assert b.tensors["traj_view_img_fts"].shape[1] == 40 and int(b.tensors["traj_vp_view_lens"].max()) == 37
    assert int((b.tensors["pano_rows"] < 0).sum()) > 0          # the panorama axis is padded with dummy rows
    assert_same_batch(a, b, (task, "built"))
    # the gathered rows are the store's: channel 0 is the store row, channel 1 the view, on every real token
    img, rows = b.tensors["traj_view_img_fts"].cpu(), b.tensors["pano_rows"].cpu().clone()
    lens = b.tensors["traj_vp_view_lens"].cpu()
    for t in range(len(rows)):
        n = int(lens[t]) if rows[t] >= 0 else 0
        assert bool((img[t, :n, 0] == rows[t]).all()) and not img[t, n:].any()
    # a second batch of the same bucket, written in place on both
    perm = np.array([3, 0, 2, 1])
    host2, ref2, keys2 = both_routes(w, task, IDXS[perm], ENDS[perm], seed=2)
    a.load(host2, grid_keys=keys2)
    b.load(ref2, grid_keys=keys2)
    assert_same_batch(a, b, (task, "refilled"))
    assert not torch.equal(b.tensors["pano_rows"].cpu(), rows)
    with pytest.raises(ValueError, match="pano_rows"):
        b.load(host2, grid_keys=keys2)


# ----------------------------------------------------------------------------- training steps
def _fresh(cfg):
    from vln_bevbert_amd import weights
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    model = GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    arena = model.finalize(DEV, torch.bfloat16)
    model.train()
    model.set_dropout(0.1)
    return model, arena


@pytest.mark.parametrize("task", ["mlm", "sap", "masksem"])
def test_four_training_steps_are_bit_equal_on_both_routes(world, task):
    """Two eager steps, the capture, one replay -- on the host-collated StaticBatch and on the by-reference one, same
    weights, same seed, dropout on: the step reads the same bits from the same shapes, so losses and parameters agree
    bit for bit."""
    from vln_bevbert_amd.static_step import StaticBatch
    from vln_bevbert_amd.train import PretrainTrainer
    w = world
    # The walk is taken whole here (24 nodes, truncated to 20 + 1 panoramas).  Cut at node 23 its next viewpoint is one it
    # has visited: the global SAP label then names a node whose logit is masked to -inf (the reference masks visited nodes
    # the same way, pretrain_cmt.py), the loss is inf on either route and comparing it says nothing.
    ends = np.array([2, 4, 0, 23])
    host, ref, keys = both_routes(w, task, IDXS, ends, seed=3)
    if task == "sap":
        labels, visited = host["global_act_labels"], host["gmap_visited_masks"]
        assert not visited[torch.arange(len(labels)), labels.clamp(min=0)].any()
    out = {}
    for route, batch, kw in (("host", host, {}), ("ref", ref, dict(view_store=w["view_store"], pano_table=w["tab"].pano))):
        model, arena = _fresh(w["cfg"])
        tr = PretrainTrainer(model, arena, learning_rate=1e-4, warmup_steps=2, num_train_steps=20)
        sb = StaticBatch(w["cfg"], task, batch, DEV, grid_store=w["grid"], grid_keys=keys, **kw)
        losses = [float(tr.step(task, sb)) for _ in range(tr.GRAPH_WARMUP + 2)]
        torch.cuda.synchronize()
        assert (sb.graph is not None) == tr.use_graphs and tr.graph_error is None
        out[route] = (losses, arena.params[::997].clone(), arena.params[-4096:].clone())
    assert np.isfinite(out["host"][0]).all() and len(set(out["host"][0])) == 4
    assert out["host"][0] == out["ref"][0], out
    assert torch.equal(out["host"][1], out["ref"][1]) and torch.equal(out["host"][2], out["ref"][2])


# ----------------------------------------------------------------------------- the loader
def test_path_batch_source_through_the_streaming_loader(world):
    """Twelve batches of PathBatchSource through StreamingLoader / BucketManager with the gather on the copy stream: every
    batch arrives with ITS panoramas in the buffers, a buffer set runs eagerly only for its own warm-up and replays its
    captured step from then on, and every set has been released at the end."""
    from vln_bevbert_amd.loader import BucketManager, StreamingLoader
    from vln_bevbert_amd.train import PretrainTrainer
    w = world
    data = w["data"]
    few = pd.R2RPathData(data.items[:4], data.graphs, data.scanvp_cands, data.image_feat_size, max_txt_len=data.max_txt_len)
    tab = pd.PrefixTables(few)
    # end_vp_pos_ratio = 1: every prefix is a whole path, so the four items always land in one bucket per task
    src = pd.PathBatchSource(few, tab, ["sap"] * 5 + ["mlm"], 4, seed=9, end_vp_pos_ratio=1.0, n_batches=12,
                             vocab_range=(104, VOCAB))
    items = list(src)
    assert [len(it) for it in items] == [4] * 12 and all("traj_view_img_fts" not in it[1] for it in items)
    model, arena = _fresh(w["cfg"])
    tr = PretrainTrainer(model, arena, learning_rate=1e-4, warmup_steps=2, num_train_steps=40)
    mgr = BucketManager(w["cfg"], DEV, depth=2, max_buckets=4, grid_store=w["grid"], view_store=w["view_store"],
                        pano_table=tab.pano)
    loader = StreamingLoader(iter(items), mgr, prefetch=1)
    steps, eager_after_warmup, losses = {}, 0, []
    for k, (task, sb) in enumerate(loader):
        rows = items[k][3]
        got = sb.tensors["traj_view_img_fts"][:len(rows), 0, 0].cpu()
        assert task == items[k][0] and torch.equal(got, rows.to(torch.float32)), k
        before, had_graph = sb.eager_runs, sb.graph is not None
        losses.append(float(tr.step(task, sb)))
        n = steps[id(sb)] = steps.get(id(sb), 0) + 1
        if n > tr.GRAPH_WARMUP + 1:
            eager_after_warmup += int(not had_graph or sb.eager_runs != before)
        loader.release(sb)
    torch.cuda.synchronize()
    sets = [sb for b in mgr.buckets.values() for sb in b["sets"]]
    assert len(losses) == 12 and np.isfinite(losses).all() and tr.graph_error is None
    assert len(mgr.buckets) == 2 and len(sets) == 4 and mgr.stats["refills"] == 8
    assert eager_after_warmup == 0
    assert all(sb.eager_runs == min(steps[id(sb)], tr.GRAPH_WARMUP) for sb in sets)
    assert mgr.captured_graphs() == sum(steps[id(sb)] > tr.GRAPH_WARMUP for sb in sets) >= 2
    assert not any(sb.in_use for sb in sets)
