"""numpy / fp64 restatement of the reference's validation loops (pretrain_src/train_r2r.py:372-510 validate_mlm,
validate_sap, validate_sem, validate_masksem; train_reverie_obj.py:483-507 validate_og) and the exact AUC in Python
integers.  What the device metrics (vln_bevbert_amd/validate.py, csrc/val_metrics.hip) are checked against.

Inputs are numpy arrays; logits of any float type are widened to fp64 (exact for fp32 and bf16 values)."""
import numpy as np


def ce_rows(logits, targets, valid=None):
    """(loss sum fp64, arg-max hits, rows) of F.cross_entropy(reduction='sum') / argmax == target / len(target) with
    ignore_index = any negative target (no loss, no hit, counted); rows with valid == 0 are left out altogether."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targets, dtype=np.int64)
    keep = np.ones(len(t), bool) if valid is None else np.asarray(valid) != 0
    loss, hits = 0.0, 0
    for r in np.nonzero(keep)[0]:
        if t[r] < 0:
            continue
        row = x[r]
        m = row.max()
        with np.errstate(divide="ignore"):
            lse = m + np.log(np.exp(row - m).sum()) if np.isfinite(m) else m
        loss += lse - row[t[r]]
        hits += int(np.argmax(row) == t[r])            # first occurrence of the maximum, as torch.argmax documents
    return loss, hits, int(keep.sum())


def bce_sum(logits, labels, valid=None):
    """(sum of binary_cross_entropy_with_logits over the valid rows' elements in fp64, valid rows)."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels) != 0
    keep = np.ones(len(x), bool) if valid is None else np.asarray(valid) != 0
    x, y = x[keep], y[keep]
    # max(x, 0) - x y + log1p(exp(-|x|)), the product written out so that an infinite logit on its label's side costs 0
    per = np.maximum(np.where(y, -x, x), 0.0) + np.log1p(np.exp(-np.abs(x)))
    return float(per.sum()), int(keep.sum())


def auc_counts(scores, labels):
    """(2U, P, N) as Python integers: group the elements by score value; a positive beats every negative below its group
    and ties with the negatives inside it: 2U = sum_k pos_k (2 neg_below_k + neg_k)."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    y = (np.asarray(labels).reshape(-1) != 0)
    s = np.where(s == 0, 0.0, s)                        # -0.0 and +0.0 are one value
    _, inv = np.unique(s, return_inverse=True)
    inv = inv.reshape(-1)
    pos = np.bincount(inv, weights=y).astype(np.int64)
    neg = np.bincount(inv, weights=~y).astype(np.int64)
    below, u2 = 0, 0
    for p, n in zip(pos.tolist(), neg.tolist()):
        u2 += p * (2 * below + n)
        below += n
    return u2, int(pos.sum()), int(neg.sum())


def auc_exact(scores, labels):
    u2, P, N = auc_counts(scores, labels)
    return u2 / (2 * P * N) if P and N else float("nan")


# ---- the five loops: lists of per-batch arrays in, the reference's val_log (without tok_per_s) out ---------------------
def validate_mlm(batches):
    """batches: [(scores (n, V), labels (n,))]"""
    loss = hits = n = 0
    for scores, labels in batches:
        l, h, k = ce_rows(scores, labels)
        loss, hits, n = loss + l, hits + h, n + k
    return {"loss": loss / n, "acc": hits / n}


validate_og = validate_mlm


def validate_sap(batches):
    """batches: [(global (B, G), local (B, K), fused (B, G), global labels (B,), local labels (B,))]"""
    s, h, n = [0.0] * 3, [0] * 3, 0
    for g, l, f, gl, ll in batches:
        for i, (x, t) in enumerate(((g, gl), (l, ll), (f, gl))):
            a, b, _ = ce_rows(x, t)
            s[i] += a
            h[i] += b
        n += len(gl)
    return {"gloss": s[0] / n, "lloss": s[1] / n, "floss": s[2] / n, "gacc": h[0] / n, "lacc": h[1] / n, "facc": h[2] / n}


def validate_sem(batches):
    """batches: [(logits (n, C), labels (n, C))]; loss over ROWS as the reference divides, AUC micro-averaged."""
    loss = rows = 0
    for x, y in batches:
        l, k = bce_sum(x, y)
        loss, rows = loss + l, rows + k
    return {"loss": loss / rows, "auc": auc_exact(np.concatenate([np.asarray(x, np.float64) for x, _ in batches]),
                                                  np.concatenate([np.asarray(y) for _, y in batches]))}


validate_masksem = validate_sem


def discordant_pairs(logits, probs, labels, chunk=256):
    """Number of (positive, negative) pairs whose order under ``probs`` differs from their order under ``logits``
    (brute force over all P N pairs)."""
    x, p = np.asarray(logits, np.float64).reshape(-1), np.asarray(probs, np.float64).reshape(-1)
    y = np.asarray(labels).reshape(-1) != 0
    xn, pn, xpos, ppos = x[~y][None, :], p[~y][None, :], x[y], p[y]
    d = 0
    for i in range(0, len(xpos), chunk):
        xp, pp = xpos[i:i + chunk, None], ppos[i:i + chunk, None]
        d += int((np.sign(xp - xn) != np.sign(pp - pn)).sum())
    return d
