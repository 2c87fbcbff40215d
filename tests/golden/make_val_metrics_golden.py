"""Golden vectors of the validation metrics: tests/golden/val_metrics.npz.

Runs only in the build container (needs /root/reference and scikit-learn; never on the GPU box).  The AUC is the
reference's own utils/mlabel_utils.AUC(average='micro', task_type='binary') -- sklearn's roc_auc_score on
``logits.sigmoid()`` -- and the probabilities it saw are stored with it; losses and accuracies are the expressions of
the reference's validate_* loops (pretrain_src/train_r2r.py:372-510) evaluated by torch on the CPU.  Inputs are seeded
and stored.

    python tests/golden/make_val_metrics_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REF, "pretrain_src"))
from utils.mlabel_utils import AUC  # noqa: E402


def ref_auc(logits, labels):
    m = AUC(average="micro", task_type="binary")
    m(logits=torch.from_numpy(logits), target=torch.from_numpy(labels.astype(np.float32)))
    return float(m.value()), np.asarray(m.y_prob)


def main():
    rng = np.random.default_rng(20240611)
    out = {}
    # ---- SEM: a tie-rich grid (97 distinct logits, multiples of 1/8 in [-6, 6]) and a continuous input in [-8, 8];
    # element counts that are no multiple of the CPU vector width and span more than one parallel chunk / stay inside one
    for name, rows in (("grid", 1025), ("cont", 601)):
        if name == "grid":
            x = (rng.integers(-48, 49, size=(rows, 40)) / 8.0).astype(np.float32)
        else:
            x = rng.uniform(-8.0, 8.0, size=(rows, 40)).astype(np.float32)
        # labels that follow the logits loosely, about a tenth positive (the semantic classes are sparse)
        y = (rng.uniform(size=x.shape) < 1.0 / (1.0 + np.exp(-(x * 0.5 - 2.5)))).astype(np.uint8)
        auc, prob = ref_auc(x, y)
        loss = F.binary_cross_entropy_with_logits(torch.from_numpy(x).double(), torch.from_numpy(y).double(), reduction="sum")
        out.update({f"sem_{name}_logits": x, f"sem_{name}_labels": y, f"sem_{name}_prob": prob,
                    f"sem_{name}_auc": np.float64(auc), f"sem_{name}_loss": np.float64(loss.item() / rows)})
        print(name, "auc", auc, "loss", out[f"sem_{name}_loss"], "P", int(y.sum()), "N", int((1 - y).sum()),
              "distinct logits", len(np.unique(x)), "distinct probabilities", len(np.unique(prob)))
    # ---- MLM: two batches of (n, V) scores
    loss = hits = n = 0
    for i, (rows, V) in enumerate(((37, 211), (12, 211))):
        x = rng.normal(0, 2.0, size=(rows, V)).astype(np.float32)
        t = rng.integers(0, V, size=rows)
        t[::3] = x[::3].argmax(1)                                         # a third of the rows are hits
        xs, ts = torch.from_numpy(x).double(), torch.from_numpy(t)
        loss += F.cross_entropy(xs, ts, reduction="sum").item()
        hits += (xs.max(dim=-1)[1] == ts).sum().item()
        n += ts.numel()
        out.update({f"mlm_scores_{i}": x, f"mlm_labels_{i}": t})
    out.update({"mlm_loss": np.float64(loss / n), "mlm_acc": np.float64(hits / n), "mlm_hits": np.int64(hits), "mlm_n": np.int64(n)})
    # ---- SAP: two batches of global / local / fused logits with -inf on masked slots and one ignored label
    s, h, n = [0.0] * 3, [0] * 3, 0
    for i, B in enumerate((5, 3)):
        g = rng.normal(0, 1.5, size=(B, 9)).astype(np.float32)
        l = rng.normal(0, 1.5, size=(B, 7)).astype(np.float32)
        g[:, 6:][rng.uniform(size=(B, 3)) < 0.5] = -np.inf
        l[:, 4:][rng.uniform(size=(B, 3)) < 0.5] = -np.inf
        f = g.copy()
        f[:, :7] += np.where(np.isfinite(l), l, 0)
        gl, ll = rng.integers(0, 6, size=B), rng.integers(0, 4, size=B)
        gl[1::2] = g[1::2].argmax(1)
        if i == 0:
            gl[0], ll[0] = -100, -100
        for k, (x, t) in enumerate(((g, gl), (l, ll), (f, gl))):
            xs, ts = torch.from_numpy(x).double(), torch.from_numpy(t)
            s[k] += F.cross_entropy(xs, ts, reduction="sum").item()
            h[k] += torch.sum(torch.argmax(xs, 1) == ts).item()
        n += len(gl)
        out.update({f"sap_g_{i}": g, f"sap_l_{i}": l, f"sap_f_{i}": f, f"sap_gl_{i}": gl, f"sap_ll_{i}": ll})
    out.update({"sap_losses": np.asarray(s, np.float64) / n, "sap_hits": np.asarray(h, np.int64), "sap_n": np.int64(n)})
    path = os.path.join(HERE, "val_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
