"""The fp64 / integer restatement of the validation metrics (tests/val_metrics_ref.py) against the reference's own numbers
(tests/golden/val_metrics.npz, written by tests/golden/make_val_metrics_golden.py), and the bound between the reference's
AUC -- sklearn on torch's CPU sigmoid -- and the exact AUC of the logits that the device computes."""
import os

import numpy as np
import pytest

from tests import val_metrics_ref as R
from vln_bevbert_amd import lib


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "val_metrics.npz"))


def test_restatement_reproduces_the_reference_losses_and_counts(gold):
    rel = lambda a, b: abs(a - b) / abs(b)
    mlm = [(gold[f"mlm_scores_{i}"], gold[f"mlm_labels_{i}"]) for i in range(2)]
    got = R.validate_mlm(mlm)
    hits = sum(R.ce_rows(x, t)[1] for x, t in mlm)
    assert hits == int(gold["mlm_hits"]) and sum(len(t) for _, t in mlm) == int(gold["mlm_n"])
    assert got["acc"] == float(gold["mlm_acc"])
    assert rel(got["loss"], float(gold["mlm_loss"])) <= 1e-12
    sap = [tuple(gold[f"sap_{k}_{i}"] for k in ("g", "l", "f", "gl", "ll")) for i in range(2)]
    got = R.validate_sap(sap)
    n = int(gold["sap_n"])
    assert sum(len(b[3]) for b in sap) == n
    assert any((b[3] < 0).any() for b in sap) and any(np.isinf(b[0]).any() for b in sap)       # the cases are in the input
    for k, (lk, ak) in enumerate((("gloss", "gacc"), ("lloss", "lacc"), ("floss", "facc"))):
        assert got[ak] * n == int(gold["sap_hits"][k]), ak
        assert rel(got[lk], float(gold["sap_losses"][k])) <= 1e-12, lk
    for name in ("grid", "cont"):
        got = R.validate_sem([(gold[f"sem_{name}_logits"], gold[f"sem_{name}_labels"])])
        assert rel(got["loss"], float(gold[f"sem_{name}_loss"])) <= 1e-12, name
    # the header and the loader agree on the new entries
    names = {"bevbert_val_ce_rows", "bevbert_val_bce_keys", "bevbert_val_auc"}
    assert names <= set(lib.prototypes()) and "val_metrics.hip" in lib.SOURCES


def test_reference_auc_is_within_the_discordant_pair_bound_of_the_exact_auc(gold):
    """|auc_reference - auc_exact| <= D / (P N): both are (pairs won + half the pairs tied) / (P N) over the same P N
    (positive, negative) pairs, one on the stored probabilities, one on the logits; a pair contributes 0, 1/2 or 1, so a
    pair whose order is the same under both contributes equally and every other pair moves the sum by at most 1.
    D is counted by brute force.  Printed: D, the bound and the distance."""
    for name in ("grid", "cont"):
        x, p, y = gold[f"sem_{name}_logits"], gold[f"sem_{name}_prob"], gold[f"sem_{name}_labels"]
        u2, P, N = R.auc_counts(x, y)
        exact = u2 / (2 * P * N)
        ref = float(gold[f"sem_{name}_auc"])
        D = R.discordant_pairs(x, p, y)
        print(f"{name}: P {P} N {N} distinct logits {len(np.unique(x))} probabilities {len(np.unique(p))} "
              f"D {D} bound {D / (P * N):.3e} |ref - exact| {abs(ref - exact):.3e}")
        assert 0.5 < exact < 1.0
        assert D > 0 and abs(ref - exact) <= D / (P * N)
        # the restatement on the probabilities the reference saw IS the reference's number
        assert abs(R.auc_exact(p, y) - ref) <= 1e-12, name
    # the grid is tie-rich on purpose, and the integer AUC treats -0.0 and +0.0 as one value
    assert len(np.unique(gold["sem_grid_logits"])) == 97
    assert R.auc_counts(np.array([-0.0, 0.0], np.float32), np.array([1, 0])) == (1, 1, 1)
    assert np.isnan(R.auc_exact(np.array([1.0, 2.0]), np.array([0, 0])))
