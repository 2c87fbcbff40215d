"""ScanGraphs (vln_bevbert_amd/nav_expert.py) against the reference's networkx tables (golden nav_expert.npz, made by
tests/golden/make_nav_expert_golden.py from load_nav_graphs + nx.all_pairs_dijkstra_path{,_length})."""
import json
import os

import numpy as np
import pytest

from vln_bevbert_amd.nav_expert import ScanGraphs

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "nav_expert.npz"))


@pytest.fixture(scope="module")
def graphs(gold, tmp_path_factory):
    """The fixture scans written back as <scan>_connectivity.json and loaded the way load_nav_graphs loads them."""
    raw = np.load(os.path.join(GOLDEN, "nav_scans.npz"))
    d = tmp_path_factory.mktemp("connectivity")
    paths = {}
    for s in gold["scans"]:
        s = str(s)
        ids, inc, un, pose = (raw[f"{s}/{k}"] for k in ("ids", "included", "unobstructed", "pose"))
        paths[s] = str(d / f"{s}_connectivity.json")
        with open(paths[s], "w") as f:
            json.dump([{"image_id": str(i), "included": bool(a), "unobstructed": [bool(x) for x in u],
                        "pose": [float(p) for p in po]} for i, a, u, po in zip(ids, inc, un, pose)], f)
    return ScanGraphs.from_connectivity(paths)


def test_node_order_and_distances_equal_networkx_bit_for_bit(gold, graphs):
    assert graphs.scans == [str(s) for s in gold["scans"]]
    assert graphs.n_max == gold["dist_0"].shape[0]
    for si in range(len(graphs.scans)):
        assert graphs.ids[si] == [str(x) for x in gold[f"ids_{si}"]]
        want = gold[f"dist_{si}"]
        got = graphs.dist[si]
        assert got.dtype == np.float64
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), si   # bit for bit, inf padding included


def test_every_shortest_path_equals_the_networkx_path(gold, graphs):
    for si in range(len(graphs.scans)):
        n = len(graphs.ids[si])
        flat, start = gold[f"paths_{si}"], gold[f"path_start_{si}"]
        for u in range(n):
            for v in range(n):
                want = flat[start[u * n + v]:start[u * n + v + 1]].tolist()
                assert graphs.path(si, u, v) == want, (si, u, v)
    assert any(len(l) >= 150 for l in graphs.ids)


def test_pred_table_is_int16_and_padded(graphs):
    S, N = len(graphs.scans), graphs.n_max
    assert graphs.pred.shape == (S, N, N) and graphs.pred.dtype == np.int16
    for si, ids in enumerate(graphs.ids):
        n = len(ids)
        assert (graphs.pred[si, :, n:] == -1).all() and (graphs.pred[si, n:, :] == -1).all()
        assert (np.diagonal(graphs.pred[si])[:n] == -1).all()
        assert np.isinf(graphs.dist[si, n:, :]).all()


def test_from_edges_builds_the_same_tables_as_from_connectivity(gold, graphs):
    """The edges of a scan in load_nav_graphs' order (item i, then its unobstructed j), as index pairs."""
    raw = np.load(os.path.join(GOLDEN, "nav_scans.npz"))
    si = 2
    s = graphs.scans[si]
    ids, inc, un, pose = (raw[f"{s}/{k}"] for k in ("ids", "included", "unobstructed", "pose"))
    edges = [(i, j) for i in range(len(ids)) if inc[i] for j in range(len(ids)) if un[i, j] and inc[j]]
    g2 = ScanGraphs.from_edges({"x": ([str(x) for x in ids], pose[:, [3, 7, 11]], edges)})
    n = len(graphs.ids[si])
    assert g2.ids[0] == graphs.ids[si] and g2.index[("x", graphs.ids[si][3])] == 3
    assert np.array_equal(g2.dist[0], graphs.dist[si, :n, :n])
    assert np.array_equal(g2.pred[0], graphs.pred[si, :n, :n])


def test_ties_follow_the_networkx_heap_order():
    # a square with unit sides: 0 -> 2 has two shortest paths; networkx takes the one through the neighbour that
    # entered the heap first (adjacency insertion order of 0: 1 before 3)
    ids = ["a", "b", "c", "d"]
    pos = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
    g = ScanGraphs.from_edges({"sq": (ids, pos, [(0, 1), (1, 2), (2, 3), (3, 0)])})
    assert g.path(0, 0, 2) == [0, 1, 2]
    g = ScanGraphs.from_edges({"sq": (ids, pos, [(0, 3), (3, 2), (2, 1), (1, 0)])})
    assert g.ids[0] == ["a", "d", "c", "b"]
    assert g.path(0, 0, 2) == [0, 1, 2]          # a -> d -> c
