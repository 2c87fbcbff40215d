"""The R2R path-data fixture of tests/golden/path_data.npz (made by tests/golden/make_path_data_golden.py from the
reference's own dataset classes), rebuilt for the host twin: shared by test_path_data_host.py and test_gpu_path_data.py."""
import functools
import json
import os

import numpy as np

from vln_bevbert_amd.nav_expert import ScanGraphs
from vln_bevbert_amd.path_data import PrefixTables, R2RPathData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(None)
def gold():
    with np.load(os.path.join(GOLDEN, "path_data.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def connectivity():
    """[(scan, connectivity json as a list of dicts)] of the three fixture scans, in the generator's order."""
    raw = np.load(os.path.join(GOLDEN, "nav_scans.npz"))
    out = []
    for s in sorted({k.split("/")[0] for k in raw.files}):
        ids, inc, un, pose = (raw[f"{s}/{k}"] for k in ("ids", "included", "unobstructed", "pose"))
        out.append((s, [{"image_id": str(i), "included": bool(a), "unobstructed": [bool(x) for x in u],
                         "pose": [float(p) for p in po]} for i, a, u, po in zip(ids, inc, un, pose)]))
    return out


def write_files(d):
    """The fixture as the files ``R2RPathData.from_files`` reads; returns its arguments."""
    g = gold()
    for s, conn in connectivity():
        with open(os.path.join(d, f"{s}_connectivity.json"), "w") as f:
            json.dump(conn, f)
    with open(os.path.join(d, "scans.txt"), "w") as f:
        f.write("\n".join(s for s, _ in connectivity()) + "\n")
    with open(os.path.join(d, "cands.json"), "w") as f:
        f.write(str(g["cands"]))
    with open(os.path.join(d, "anno.jsonl"), "w") as f:
        for it in json.loads(str(g["items"])):
            f.write(json.dumps(it) + "\n")
    return [os.path.join(d, "anno.jsonl")], d, os.path.join(d, "cands.json")


@functools.lru_cache(None)
def graphs():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for s, conn in connectivity():
            paths[s] = os.path.join(d, f"{s}_connectivity.json")
            with open(paths[s], "w") as f:
                json.dump(conn, f)
        return ScanGraphs.from_connectivity(paths)


def view_features(feat_size, n_keys=None, seed=None):
    """(N, 36, feat_size) fp16 identity-encoding view features: channel 0 the viewpoint's row in ``keys``, channel 1 the
    view (both exact in fp16), the rest seeded noise."""
    g = gold()
    n = len(g["keys"]) if n_keys is None else n_keys
    fts = np.random.default_rng(int(g["seed"]) if seed is None else seed).standard_normal((n, 36, feat_size)).astype(np.float16)
    fts[:, :, 0] = np.arange(n)[:, None]
    fts[:, :, 1] = np.arange(36)[None, :]
    return fts


@functools.lru_cache(None)
def data(image_feat_size=None, store_feat_size=None, vocab=None):
    """The twin over the fixture, with identity view features of ``store_feat_size`` channels (default: the golden's).
    ``vocab``: fold the instruction tokens into a vocabulary of that size (tiny models), keeping [CLS] 101 / [SEP] 102."""
    g = gold()
    D = int(g["image_feat_size"]) if image_feat_size is None else image_feat_size
    Ds = int(g["store_feat_size"]) if store_feat_size is None else store_feat_size
    keys = [str(k) for k in g["keys"]]
    fts = view_features(Ds)
    items = json.loads(str(g["items"]))
    if vocab is not None:
        for it in items:
            it["instr_encoding"] = [t if t in (101, 102) else 104 + t % (vocab - 104) for t in it["instr_encoding"]]
    return R2RPathData(items, graphs(), json.loads(str(g["cands"])), D,
                       max_txt_len=int(g["max_txt_len"]), view_fts={k: fts[i] for i, k in enumerate(keys)})


@functools.lru_cache(None)
def tables():
    return PrefixTables(data())


def ragged(name, group="prefix"):
    """The per-prefix arrays of a recorded field, reshaped."""
    g = gold()
    flat = g[f"{group}/{name}"]
    if flat.dtype.kind == "U":
        return list(flat)
    shapes = g[f"{group}/{name}.shape"]
    out, pos = [], 0
    for sh in shapes:
        n = int(np.prod(sh)) if len(sh) else 1
        out.append(flat[pos:pos + n].reshape(tuple(int(x) for x in sh)))
        pos += n
    assert pos == len(flat)
    return out


def rows_of(d, scan, vpids):
    """Viewpoint ids -> rows of the golden's ``keys`` (-1 for None)."""
    row = {str(k): i for i, k in enumerate(gold()["keys"])}
    return np.asarray([-1 if v is None else row[f"{scan}_{v}"] for v in vpids], dtype=np.int32)
