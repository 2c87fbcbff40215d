"""vln_bevbert_amd/path_data.py against the reference's data layer (golden path_data.npz, recorded by
tests/golden/make_path_data_golden.py from R2RTextPathData / MlmDataset / SapDataset / MaskSemDataset and their collates).
Everything is compared exactly: the twin calls the same numpy functions on the same dtypes and shapes."""
import math

import numpy as np
import pytest
import torch

from vln_bevbert_amd import path_data as pd
from vln_bevbert_amd.path_data import PrefixTables, R2RPathData

from . import path_data_cases as C

FLOAT_FIELDS = ("traj_loc_fts", "gmap_pos_fts", "gmap_pair_dists", "T_c2w", "T_w2c", "S_w2c", "bev_gpos_fts")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_sample(s, p, G, data, where):
    """One get_input dict against prefix p of the golden."""
    scan = data.items[int(G["idx"][p])]["scan"]
    assert s["instr_id"] == str(G["instr_id"][p]), where
    assert list(s["instr_encoding"]) == G["instr_encoding"][p].tolist(), where
    assert [len(x) for x in s["traj_view_idxs"]] == G["view_lens"][p].tolist(), where
    assert np.array_equal(np.concatenate(s["traj_view_idxs"]), G["pano_view"][p]), where
    assert np.array_equal(np.repeat(C.rows_of(data, scan, s["traj_vpids"]), G["view_lens"][p]), G["pano_node"][p]), where
    assert np.array_equal(np.concatenate([np.asarray(x, dtype=np.int64) for x in s["traj_nav_types"]]),
                          G["traj_nav_types"][p]), where
    assert [len(c) for c in s["traj_cand_vpids"]] == G["cand_counts"][p].tolist(), where
    assert np.array_equal(C.rows_of(data, scan, [v for c in s["traj_cand_vpids"] for v in c]), G["traj_cand_vpids"][p]), where
    assert np.array_equal(C.rows_of(data, scan, s["traj_vpids"]), G["traj_vpids"][p]), where
    assert np.array_equal(C.rows_of(data, scan, s["gmap_vpids"]), G["gmap_vpids"][p]), where
    assert list(s["gmap_step_ids"]) == G["gmap_step_ids"][p].tolist(), where
    assert [int(x) for x in s["gmap_visited_masks"]] == G["gmap_visited_masks"][p].tolist(), where
    assert same_bits(np.asarray(s["bev_cand_idxs"]), G["bev_cand_idxs"][p]), where
    assert int(s["global_act_labels"]) == int(G["global_act_labels"][p]), where
    assert int(s["local_act_labels"]) == int(G["local_act_labels"][p]), where
    for k in FLOAT_FIELDS:
        got = np.concatenate(s[k], 0) if k == "traj_loc_fts" else s[k]
        assert same_bits(got, G[k][p]), (where, k, np.abs(np.asarray(got, np.float64) - G[k][p]).max())


@pytest.fixture(scope="module")
def G():
    names = ("idx", "end_idx", "instr_id", "instr_encoding", "view_lens", "pano_node", "pano_view", "traj_loc_fts",
             "traj_nav_types", "cand_counts", "traj_cand_vpids", "traj_vpids", "gmap_vpids", "gmap_step_ids",
             "gmap_visited_masks", "gmap_pos_fts", "gmap_pair_dists", "T_c2w", "T_w2c", "S_w2c", "bev_cand_idxs",
             "bev_gpos_fts", "global_act_labels", "local_act_labels")
    return {k: C.ragged(k) for k in names}


def test_the_fixture_covers_the_cases_the_tables_must_get_right(G):
    data = C.data()
    lens = [len(it["path"]) for it in data.items]
    assert 1 in lens and max(lens) > pd.TRAIN_MAX_STEP and set(range(2, 8)) <= set(lens)
    walk = data.items[lens.index(max(lens))]["path"]
    assert len(set(walk)) < len(walk)                                        # re-visits
    assert max(int(v.max()) for v in G["view_lens"]) == 37                   # two candidates on one view index
    assert min(int(c.min()) for c in G["cand_counts"]) == 1                  # a viewpoint with one candidate
    txt = [len(it["instr_encoding"]) for it in data.items]
    assert min(txt) < data.max_txt_len < max(txt)
    assert len(G["idx"]) == sum(lens)


def test_get_input_equals_the_reference_for_every_prefix(G):
    data = C.data()
    p = 0
    for idx, item in enumerate(data.items):
        for e in range(len(item["path"])):
            assert (int(G["idx"][p]), int(G["end_idx"][p])) == (idx, e)
            s = data.get_input(idx, e)
            check_sample(s, p, G, data, (idx, e))
            # the features themselves: rows of the identity store, cut to image_feat_size, fp32
            f = np.concatenate(s["traj_view_img_fts"], 0)
            assert f.dtype == np.float32 and f.shape[1] == data.image_feat_size
            assert np.array_equal(f[:, 0], G["pano_node"][p]) and np.array_equal(f[:, 1], G["pano_view"][p])
            assert s["grid_key"] == f"{item['scan']}_{item['path'][e]}"
            p += 1


def test_prefix_and_pano_tables_reproduce_get_input_for_every_prefix(G):
    data, tab = C.data(), C.tables()
    assert len(tab) == len(G["idx"])
    for p in range(len(tab)):
        idx, e = int(G["idx"][p]), int(G["end_idx"][p])
        s = tab.sample(data, idx, e)
        check_sample(s, p, G, data, (idx, e))
        n_pano, n_gmap, n_cand, widest = tab.counts(p)
        assert (n_pano, n_gmap, n_cand, widest) == (len(G["view_lens"][p]), len(G["gmap_vpids"][p]),
                                                    len(G["bev_cand_idxs"][p]), int(G["view_lens"][p].max()))
        assert s["traj_vp_view_lens"] == G["view_lens"][p].tolist()
    pano = tab.pano
    assert pano.keys == [str(k) for k in C.gold()["keys"]]
    assert pano.n_tokens.max() == 37 and pano.view_order.shape[1] == 37
    for r in range(len(pano.keys)):                 # everything beyond a panorama's tokens is zero
        n = int(pano.n_tokens[r])
        assert not pano.loc_fts[r, n:].any() and not pano.nav_types[r, n:].any() and not pano.view_order[r, n:].any()


def test_save_load_round_trips_bit_for_bit(tmp_path):
    tab = C.tables()
    path = str(tmp_path / "tables.npz")
    tab.save(path)
    back = PrefixTables.load(path)
    for k in PrefixTables.ARRAYS:
        assert same_bits(getattr(tab, k), getattr(back, k)), k
    for k in pd.PanoTable.FIELDS:
        assert same_bits(getattr(tab.pano, k), getattr(back.pano, k)), k
    assert back.pano.keys == tab.pano.keys and same_bits(back.pano.cand_ids, tab.pano.cand_ids)
    s0, s1 = tab.sample(C.data(), 9, 21), back.sample(C.data(), 9, 21)
    assert same_bits(s0["gmap_pos_fts"], s1["gmap_pos_fts"]) and s0["gmap_vpids"] == s1["gmap_vpids"]


def _recorded(task):
    g = C.gold()
    out = {}
    for name in ("random", "choice", "rand", "randint"):
        flat, n = g[f"{task}/draw.{name}"], g[f"{task}/draw.{name}.n"]
        out[name] = np.split(flat, np.cumsum(n)[:-1])
    return out


@pytest.mark.parametrize("task", ["mlm", "sap", "masksem"])
def test_collated_batch_equals_the_reference_given_its_draws(task):
    g, data = C.gold(), C.data()
    idxs, ends = g[f"{task}/idx"], g[f"{task}/end_idx"]
    draws = _recorded(task)
    samples = [data.get_input(int(i), int(e)) for i, e in zip(idxs, ends)]
    labels = masks = None
    n_cells = data.bev_dim ** 2
    for b, s in enumerate(samples):
        # the end index follows from the recorded uniform the way the Dataset decides it
        r = draws["rand"][b][0]
        n = len(data.items[int(idxs[b])]["path"])
        assert int(ends[b]) == (n - 1 if r < float(g["pos_ratio"]) else int(draws["randint"][b][0]))
    if task == "mlm":
        labels = []
        for b, s in enumerate(samples):
            u = draws["random"][b]
            ids = s["instr_encoding"]
            assert len(u) == len(ids)
            repl = np.zeros(len(ids), dtype=np.int64)
            takes = [k for k in range(len(ids)) if u[k] < 0.15 and 0.8 <= u[k] / 0.15 < 0.9]
            assert len(takes) == len(draws["choice"][b])
            repl[takes] = draws["choice"][b]
            s["instr_encoding"], lab = pd.mask_tokens(u, repl, ids)
            labels.append(lab)
    elif task == "masksem":
        masks = []
        for b in range(len(samples)):
            u = draws["rand"][b][1:1 + n_cells]
            pos = int(ends[b]) == len(data.items[int(idxs[b])]["path"]) - 1
            extra = draws["randint"][b][0 if pos else 1:]
            assert len(extra) == (0 if (u < float(g["mask_prob"])).any() else 1)
            masks.append(pd.bev_mrc_masks(u, float(g["mask_prob"]), int(extra[0]) if len(extra) else 0))
    batch = pd.collate(task, samples, data.bev_dim, txt_labels=labels, mrc_masks=masks)
    want = {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(task + "/")}
    img = batch.pop("traj_view_img_fts")
    assert img.dtype == torch.float32 and img.shape[-1] == data.image_feat_size
    assert np.array_equal(img[..., 0].numpy(), want["pano_node"]) and np.array_equal(img[..., 1].numpy(), want["pano_view"])
    seen = set()
    for k, v in batch.items():
        if torch.is_tensor(v):
            assert same_bits(v.numpy(), want[k]), (task, k)
            seen.add(k)
    assert list(batch["traj_step_lens"]) == want["traj_step_lens"].tolist()
    recorded = {k for k in want if "." not in k and k not in ("idx", "end_idx", "pano_node", "pano_view", "traj_step_lens")}
    assert recorded == seen, recorded ^ seen          # no field of the reference's batch is missing, none is extra
    for b, i in enumerate(idxs):
        scan = data.items[int(i)]["scan"]
        assert np.array_equal(C.rows_of(data, scan, batch["traj_vpids"][b]), want[f"traj_vpids.{b}"])
        assert np.array_equal(C.rows_of(data, scan, batch["gmap_vpids"][b]), want[f"gmap_vpids.{b}"])
        assert [len(c) for c in batch["traj_cand_vpids"][b]] == want[f"cand_counts.{b}"].tolist()
        assert np.array_equal(C.rows_of(data, scan, [v for c in batch["traj_cand_vpids"][b] for v in c]),
                              want[f"traj_cand_vpids.{b}"])


def test_from_files_equals_the_in_memory_construction(tmp_path, G):
    data = C.data()
    anno, conn, cands = C.write_files(str(tmp_path))
    d2 = R2RPathData.from_files(anno, conn, cands, data.image_feat_size, max_txt_len=data.max_txt_len)
    assert d2.items == data.items and d2.scanvp_cands == data.scanvp_cands
    assert [list(c) for c in d2.scanvp_cands.values()] == [list(c) for c in data.scanvp_cands.values()]     # dict order too
    assert d2.graphs.scans == data.graphs.scans and d2.graphs.ids == data.graphs.ids
    assert same_bits(d2.graphs.dist, data.graphs.dist) and same_bits(d2.graphs.hops, data.graphs.hops)
    for p in (0, 7, 30, len(G["idx"]) - 1):
        check_sample(d2.get_input(int(G["idx"][p]), int(G["end_idx"][p])), p, G, d2, p)


def test_hops_are_the_edge_counts_of_the_networkx_paths():
    g = C.graphs()
    for si in range(len(g.scans)):
        n = len(g.ids[si])
        for u in range(0, n, 7):
            for v in range(n):
                assert g.hops[si, u, v] == len(g.path(si, u, v)) - 1
        assert (g.hops[si, n:] == -1).all() and (g.hops[si, :, n:] == -1).all()


@pytest.mark.parametrize("task,ratio", [("mlm", 0.2), ("sap", 0.2), ("masksem", 0.5)])
def test_draw_branch_frequencies_match_the_reference(task, ratio):
    """tasks.py:74-78 / :319-325 / :630-634 with dataset.py:499-507: P(last node) = ratio; otherwise uniform over
    path[:-1] (SAP's 'neg_others' included).  Each observed frequency within 4 standard deviations over 20 000 draws."""
    data = C.data()
    n_draws = 20000
    idx = next(i for i, it in enumerate(data.items) if len(it["path"]) == 5)
    n = 5
    ends = data.draw(task, np.full(n_draws, idx), np.random.default_rng(7), ratio)
    probs = [(1 - ratio) / (n - 1)] * (n - 1) + [ratio]
    for e, p in enumerate(probs):
        sd = math.sqrt(p * (1 - p) / n_draws)
        assert abs((ends == e).mean() - p) < 4 * sd, (task, e, (ends == e).mean(), p)
    single = next(i for i, it in enumerate(data.items) if len(it["path"]) == 1)
    assert (data.draw(task, np.full(50, single), np.random.default_rng(1), ratio) == 0).all()


def test_mask_rules_at_least_one():
    ids = [101, 5000, 6000, 102]
    out, lab = pd.mask_tokens(np.full(4, 0.5), np.zeros(4, np.int64), ids)           # nothing drawn: token 0 is masked
    assert out == [103, 5000, 6000, 102] and lab == [101, -1, -1, -1]
    u = np.array([0.5, 0.15 * 0.5, 0.15 * 0.85, 0.15 * 0.95])                         # mask / random token / keep
    out, lab = pd.mask_tokens(u, np.array([0, 0, 7777, 0]), ids)
    assert out == [101, 103, 7777, 102] and lab == [-1, 5000, 6000, 102]
    m = pd.bev_mrc_masks(np.full(441, 0.9), 0.15, pick=17)                            # none below: the drawn cell, not cell 0
    assert m.sum() == 1 and m[17]
    u = np.full(441, 0.9)
    u[[3, 400]] = 0.1
    m = pd.bev_mrc_masks(u, 0.15, pick=17)
    assert m.sum() == 2 and m[3] and m[400]


def test_source_batches_match_their_cached_counts_and_the_full_collate():
    """PathBatchSource's by-reference host batch: the shape counts come from the tables, the small tensors equal those of
    the full collate of the same prefixes, and the panorama tensors are replaced by rows."""
    data, tab = C.data(), C.tables()
    src = pd.PathBatchSource(data, tab, ["sap"], 4, seed=3)
    idxs, ends = np.array([0, 9, 6, 7]), np.array([1, 22, 0, 4])
    task, batch, keys, rows = src.batch("sap", idxs, ends)
    full = pd.collate("sap", [data.get_input(int(i), int(e)) for i, e in zip(idxs, ends)], data.bev_dim)
    n_pano, widest, g_max, k_max, l_max = src.signature_counts(idxs, ends)
    assert (n_pano, widest) == tuple(full["traj_view_img_fts"].shape[:2]) and rows.shape == (n_pano,)
    assert (g_max, k_max, l_max) == (full["gmap_pos_fts"].shape[1], full["bev_cand_idxs"].shape[1], full["txt_ids"].shape[1])
    assert not {"traj_view_img_fts", "traj_loc_fts", "traj_nav_types", "pano_rows"} & set(batch)
    for k, v in batch.items():
        if torch.is_tensor(v):
            assert torch.equal(v, full[k]), k
        else:
            assert v == full[k], k
    assert keys == [f"{data.items[i]['scan']}_{data.items[i]['path'][e]}" for i, e in zip(idxs, ends)]
    assert np.array_equal(tab.pano.n_tokens[rows.numpy()], full["traj_vp_view_lens"].numpy())
    assert np.array_equal(rows.numpy(), np.asarray(full["traj_view_img_fts"][:, 0, 0].numpy(), dtype=np.int32))


def test_view_store_reads_an_hdf5_file_through_the_package_reader(golden_dir):
    """ViewFeatureStore.from_hdf5 on a real file (tests/golden/hdf5/rgb.hdf5, written by h5py): opened by the reader
    feature_cache.convert_hdf5 uses, rows in the order asked for, fp16 as on disk.  The fixture's datasets are
    (12, 196, 6); they are read as (36, 392) panoramas through a reshaping view of the same file object."""
    import os

    from vln_bevbert_amd import hdf5_reader
    from vln_bevbert_amd.feature_store import ViewFeatureStore
    path = os.path.join(golden_dir, "hdf5", "rgb.hdf5")
    back = np.load(os.path.join(golden_dir, "hdf5", "readback.npz"))

    class AsPanoramas:
        def __init__(self, p):
            self.f = hdf5_reader.open_file(p)

        def __enter__(self):
            self.f.__enter__()
            return self

        def __exit__(self, *a):
            return self.f.__exit__(*a)

        def keys(self):
            return self.f.keys()

        def __getitem__(self, k):
            return {Ellipsis: np.asarray(self.f[k][...]).reshape(36, -1)}

    keys = [str(k) for k in back["rgb/keys"]]
    store = ViewFeatureStore.from_hdf5(path, "cpu", reader=AsPanoramas)
    assert store.keys == keys and (store.n_views, store.Ds) == (36, 392) and store.fts.dtype == torch.float16
    pick = keys[::-1][:3]
    some = ViewFeatureStore.from_hdf5(path, "cpu", keys=pick, reader=AsPanoramas)
    assert some.keys == pick and some.rows(pick).tolist() == [0, 1, 2]
    for i, k in enumerate(pick):
        assert back[f"rgb/{k}"].dtype == np.float16
        assert np.array_equal(some.fts[i].numpy(), back[f"rgb/{k}"].reshape(36, -1))
    with pytest.raises(KeyError, match="not in the view-feature store"):
        some.rows(["nowhere_0"])


def test_a_refill_with_another_candidate_count_fits_the_bucket_of_a_task_that_does_not_read_it():
    """On real paths the width of bev_cand_idxs (the batch maximum of the last panoramas' candidate counts) moves from
    batch to batch.  Only SAP reads it and only SAP's signature carries it: for MLM a refill of another width lands in the
    same buffers, for SAP it is another bucket."""
    from vln_bevbert_amd.config import BevBertConfig
    from vln_bevbert_amd.static_step import StaticBatch
    data = C.data()
    cfg = BevBertConfig.tiny(image_feat_size=data.image_feat_size, vocab_size=30522)
    mk = lambda task, ends: pd.collate(task, [data.get_input(i, e) for i, e in zip((1, 2), ends)], data.bev_dim,
                                       txt_labels=[[-1] * 32, [-1] * 24] if task == "mlm" else None)
    for ends in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (2, 1)):
        a, b = mk("mlm", (0, 0)), mk("mlm", ends)
        if a["bev_cand_idxs"].shape != b["bev_cand_idxs"].shape and \
                StaticBatch.plan(cfg, "mlm", a)["signature"] == StaticBatch.plan(cfg, "mlm", b)["signature"]:
            break
    else:
        pytest.fail("no two fixture batches of one MLM bucket differ in their candidate count")
    sb = StaticBatch(cfg, "mlm", a, "cpu")
    sb.load(b)
    assert torch.equal(sb.tensors["bev_cand_idxs"], b["bev_cand_idxs"])
    assert StaticBatch.plan(cfg, "sap", mk("sap", (0, 0)))["signature"] != StaticBatch.plan(cfg, "sap", mk("sap", ends))["signature"]
