"""Pre-training validation on the device: the counterpart of pretrain_src/train_r2r.py:351-510 (validate, validate_mlm,
validate_sap, validate_sem, validate_masksem) and train_reverie_obj.py's validate_og.

The reference reads 2 to 6 scalars back per batch and ships every SEM logit to the host for sklearn.  Here the sums, the
counts and the sort keys of the AUC stay in device memory (csrc/val_metrics.hip) and a task reads back ONCE: sixteen
8-byte words (three accumulators, the AUC statistic, the key-overflow flag) in one device-to-host copy.

Metric definitions ("Validation metrics"):
  * mlm, og:        loss = sum of cross-entropies / rows, acc = arg-max hits / rows (lowest index on a tie).
  * mrc:            loss = sum over the masked objects of KL(detector probabilities || softmax(logits)) / objects, acc =
                    objects whose arg-max class equals the arg-max of their probabilities / objects (lowest index on a tie).
  * sap:            gloss / lloss / floss and gacc / lacc / facc over the global, local and fused logits, all divided by
                    the number of samples; a label of -100 adds no loss and no hit but counts as a sample.
  * sem, masksem:   loss = sum of BCE-with-logits over all elements / ROWS (the reference's divisor), auc = the exact
                    Mann-Whitney AUC of the fp32 logits over all (row, class) elements (micro average), ties at
                    mid-rank, computed in integers: auc = 2U / (2 P N).  NaN when P == 0 or N == 0 (sklearn raises there).
The reference's AUC is sklearn's on ``logits.sigmoid()``; torch's CPU sigmoid is not a function of the value alone
(vectorised body and tail round differently), so that number is not reproducible to the last digits; how far the two can
be apart is bounded in tests/test_val_metrics_host.py.

``static_step.StaticBatch`` inputs run without any host synchronisation (the tails of the training step: loader-built
masked-token rows, SAP fusion table, ops.sem_select); collate dicts go through ``model(batch, task,
compute_loss=False)``, which synchronises where the reference does, and then through the same kernels.
"""
import time

import torch

from . import ops
from .lib import call, dtype_code, ptr, stream
from .static_step import StaticBatch
from .vilmodel import ensure_arena

_AUC_SCRATCH_BYTES = 1024 * 3 * 8
# accumulator block of a task, int64 words: [0:3] [3:6] [6:9] three {sum f64, a, b} accumulators, [9:12] 2U P N, [12] overflow
_WORDS = 16
_ACC, _AUC, _OVF = (0, 3, 6), 9, 12

TAP = None          # test hook: set to a list and every kernel call appends (entry, dict of the tensors it consumed)


_SCRATCH = {}


def _scratch(dev, nbytes):
    """Record space of the kernels (8 bytes per row); launches of one stream follow each other, so one buffer serves."""
    buf = _SCRATCH.get(dev)
    if buf is None or buf.numel() * 8 < nbytes:
        buf = _SCRATCH[dev] = torch.empty(max(_AUC_SCRATCH_BYTES, nbytes + nbytes // 2) // 8 + 1, dtype=torch.int64, device=dev)
    return buf


def val_ce_rows(logits, targets, valid, acc):
    """acc (3 int64 words: fp64 loss sum, hits, rows) += the rows of ``logits`` (R, C) fp32 / bf16, unit column stride, any
    row stride; see include/bevbert_hip.h bevbert_val_ce_rows."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and targets.dtype == torch.int64 and targets.is_contiguous()
    assert valid is None or (valid.dtype == torch.float32 and valid.is_contiguous() and valid.numel() == logits.shape[0])
    assert acc.dtype == torch.int64 and acc.numel() == 3 and acc.is_contiguous() and targets.numel() == logits.shape[0]
    R, C = logits.shape
    if TAP is not None:
        TAP.append(("val_ce_rows", {"logits": logits.clone(), "targets": targets.clone(),
                                    "valid": None if valid is None else valid.clone()}))
    call("bevbert_val_ce_rows", ptr(logits), logits.stride(0) if R > 1 else C, ptr(targets), ptr(valid), R, C,
         dtype_code(logits), ptr(acc), ptr(_scratch(logits.device, 8 * R)), stream())


def val_kl_rows(logits, targets, idx, valid, acc):
    """acc (fp64 KL sum, arg-max agreements, rows) += the rows of ``logits`` (R, C) fp32 / bf16 against the fp32 rows
    ``targets[idx]`` (idx None: row r); see include/bevbert_hip.h bevbert_val_kl_rows."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and targets.dim() == 2 and targets.shape[1] == logits.shape[1]
    assert targets.dtype == torch.float32 and targets.is_contiguous()
    R, C = logits.shape
    assert (idx is None and targets.shape[0] == R) or (idx is not None and idx.dtype == torch.int64 and idx.is_contiguous()
                                                       and idx.numel() == R)
    assert valid is None or (valid.dtype == torch.float32 and valid.is_contiguous() and valid.numel() == R)
    assert acc.dtype == torch.int64 and acc.numel() == 3 and acc.is_contiguous()
    if TAP is not None:
        TAP.append(("val_kl_rows", {"logits": logits.clone(), "targets": targets.clone(), "idx": None if idx is None else idx.clone(),
                                    "valid": None if valid is None else valid.clone()}))
    call("bevbert_val_kl_rows", ptr(logits), logits.stride(0) if R > 1 else C, ptr(targets), ptr(idx), ptr(valid), R, C,
         dtype_code(logits), ptr(acc), ptr(_scratch(logits.device, 8 * R)), stream())


def val_bce_keys(logits, labels, idx, valid, acc, keys, cursor, capacity, overflow):
    """acc += (BCE sum, valid rows); keys[cursor : cursor + R C] = the packed sort keys (INT64_MAX for invalid rows);
    returns the advanced cursor.  ``labels`` uint8 (n, C) read through ``idx`` (None: row r)."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and labels.dtype == torch.uint8 and labels.is_contiguous()
    assert labels.shape[-1] == logits.shape[1] and (idx is not None or labels.numel() == logits.numel())
    assert keys.dtype == torch.int64 and keys.is_contiguous() and capacity <= keys.numel()
    assert acc.dtype == torch.int64 and acc.numel() == 3 and overflow.dtype == torch.int64
    R, C = logits.shape
    if TAP is not None:
        TAP.append(("val_bce_keys", {"logits": logits.clone(), "labels": labels.clone(), "idx": None if idx is None else idx.clone(),
                                     "valid": None if valid is None else valid.clone()}))
    call("bevbert_val_bce_keys", ptr(logits), logits.stride(0) if R > 1 else C, ptr(labels), ptr(idx), ptr(valid), R, C,
         dtype_code(logits), ptr(acc), ptr(_scratch(logits.device, 8 * R)), ptr(keys), cursor, capacity, ptr(overflow), stream())
    return cursor + R * C


def val_auc(sorted_keys, out):
    """out (3 int64 words) = 2U, P, N of ascending keys (INT64_MAX entries skipped)."""
    assert sorted_keys.dtype == torch.int64 and sorted_keys.is_contiguous() and out.dtype == torch.int64 and out.numel() == 3
    call("bevbert_val_auc", ptr(sorted_keys), sorted_keys.numel(), ptr(out), ptr(_scratch(out.device, _AUC_SCRATCH_BYTES)), stream())


def _read_back(t):
    """THE device-to-host copy of a task (tests wrap it to tell it from any other synchronisation)."""
    return t.cpu()


class ValAccumulator:
    """Device state of one task's validation pass: the 16-word block and the key buffer of the AUC.

    ``key_capacity=None``: the key buffer grows on the host's knowledge of the cursor (an allocation and a device copy,
    no synchronisation).  A number fixes it: keys beyond it are dropped on the device, the overflow flag comes back with
    the read-back and ``finish`` raises."""

    def __init__(self, device, key_capacity=None):
        self.device = torch.device(device)
        self.words = torch.zeros(_WORDS, dtype=torch.int64, device=self.device)
        self.fixed = key_capacity is not None
        self.capacity = int(key_capacity) if self.fixed else 0
        self.keys = torch.empty(self.capacity, dtype=torch.int64, device=self.device) if self.fixed else None
        self.cursor = 0

    def reset(self):
        call("bevbert_zero", ptr(self.words), _WORDS * 8, stream())
        self.cursor = 0

    def acc(self, i=0):
        return self.words[_ACC[i]:_ACC[i] + 3]

    def add_ce(self, logits, targets, valid=None, which=0):
        val_ce_rows(logits, targets, valid, self.acc(which))

    def add_kl(self, logits, targets, idx=None, valid=None):
        val_kl_rows(logits, targets, idx, valid, self.acc(0))

    def add_bce(self, logits, labels, idx=None, valid=None):
        need = self.cursor + logits.numel()
        if not self.fixed and need > self.capacity:
            cap = max(need, 2 * self.capacity)
            keys = torch.empty(cap, dtype=torch.int64, device=self.device)
            if self.cursor:
                keys[:self.cursor].copy_(self.keys[:self.cursor])
            self.keys, self.capacity = keys, cap
        self.cursor = val_bce_keys(logits, labels, idx, valid, self.acc(0), self.keys, self.cursor, self.capacity,
                                   self.words[_OVF:_OVF + 1])

    def finish(self, auc=False):
        """Sort + AUC statistic if asked, then the one read-back: a dict of Python numbers."""
        if auc:
            n = min(self.cursor, self.capacity)
            if n:
                sorted_keys, _ = torch.sort(self.keys[:n])              # plumbing: once per task
            else:
                sorted_keys = torch.empty(0, dtype=torch.int64, device=self.device)
            val_auc(sorted_keys, self.words[_AUC:_AUC + 3])
        host = _read_back(self.words)
        if int(host[_OVF]):
            raise RuntimeError(f"validation: {self.cursor} AUC keys do not fit the key buffer of {self.capacity}")
        out = {"sums": [float(host[i:i + 1].view(torch.float64)) for i in _ACC],
               "a": [int(host[i + 1]) for i in _ACC], "b": [int(host[i + 2]) for i in _ACC]}
        out["U2"], out["P"], out["N"] = (int(x) for x in host[_AUC:_AUC + 3])
        return out


def auc_of(U2, P, N):
    return U2 / (2 * P * N) if P and N else float("nan")


# ---- one batch of one task -> accumulator ---------------------------------------------------------------------------
def _static_inputs(model, sb):
    ensure_arena(model)
    b = dict(sb.tensors)
    model.lift_splat(b)
    model.drop_feats(b)
    return b


def _sem_static(model, b, acc, masked):
    if masked:
        b["bev_fts"] = b["bev_fts"].detach().masked_fill(b["bev_mrc_masks"].unsqueeze(-1), 0)
    bev = model.bert.forward_sem(*model._cmt_args(b), sem_pred_token=model.sem_pred_token, **model._host_kw(b))
    st = b["_static"]
    sems = b["bev_sems"].reshape(-1, b["bev_sems"].shape[-1])
    if sems.dtype != torch.uint8:
        sems = (sems != 0).to(torch.uint8)
    idx, valid, _ = ops.sem_select(b["bev_sem_masks"], b["bev_mrc_masks"] if masked else None, st["sem_cap"], sems.shape[-1])
    rows = ops.take_rows(bev.reshape(-1, bev.shape[-1]), idx)
    acc.add_bce(model.local_sem_head(rows), sems.contiguous(), idx, valid)


def add_batch(model, task, batch, acc):
    """Run one validation batch of ``task`` and add its metrics to ``acc``."""
    if isinstance(batch, StaticBatch) and task.startswith("mlm"):
        b = _static_inputs(model, batch)
        st = b["_static"]
        txt = model.bert.forward_mlm(*model._cmt_args(b), **model._host_kw(b))
        rows = ops.take_rows(txt.reshape(-1, txt.shape[-1]), st["mlm_pos"])
        acc.add_ce(model.mlm_head(rows), st["mlm_targets"], st["mlm_valid"])       # logits in the compute dtype
    elif isinstance(batch, StaticBatch) and task.startswith(("sem", "masksem")):
        _sem_static(model, _static_inputs(model, batch), acc, task.startswith("masksem"))
    elif task.startswith("mlm"):
        scores = model(batch, task, compute_loss=False)
        labels = batch["txt_labels"]
        acc.add_ce(scores, labels[labels != -1].contiguous())                       # one sync, as the reference
    elif task.startswith("sap"):
        # a static batch carries the fusion table and the masks: the non-fused tail has no synchronisation with it
        g, l, f, gl, ll = model(batch.tensors if isinstance(batch, StaticBatch) else batch, task, compute_loss=False)
        gl, ll = gl.contiguous(), ll.contiguous()
        acc.add_ce(g, gl, which=0)
        acc.add_ce(l, ll, which=1)
        acc.add_ce(f, gl, which=2)
    elif task.startswith("og"):
        b = batch.tensors if isinstance(batch, StaticBatch) else batch
        acc.add_ce(model(b, task, compute_loss=False), b["obj_labels"].contiguous())
    elif task.startswith("mrc") and isinstance(batch, StaticBatch) and "mrc_pos" in batch.tensors["_static"]:
        # an obj_static batch: loader-built rows of the masked objects, zero-weight padding, no synchronisation
        b = _static_inputs(model, batch)
        st = b["_static"]
        _, _, obj, _ = model.bert(*model._cmt_args(b), return_gmap_embeds=False, **model._host_kw(b))
        rows = ops.take_rows(obj.reshape(-1, obj.shape[-1]), st["mrc_pos"])
        probs = b["vp_obj_probs"].reshape(-1, b["vp_obj_probs"].shape[-1])
        acc.add_kl(model.obj_classifier(rows), probs, st["mrc_tpos"], st["mrc_valid"])      # logits in the compute dtype
    elif task.startswith("mrc"):
        pred, targets = model(batch.tensors if isinstance(batch, StaticBatch) else batch, task, compute_loss=False)
        acc.add_kl(pred, targets.contiguous())                                          # one sync, as the reference
    elif task.startswith(("sem", "masksem")):
        logits, labels = model(batch, task, compute_loss=False)
        acc.add_bce(logits, (labels != 0).to(torch.uint8).contiguous())
    else:
        raise ValueError(f"Undefined task {task}")


def val_log(task, r, seconds):
    """The reference's val_log of ``task`` from the numbers ``ValAccumulator.finish`` read back."""
    div = lambda x, n: x / n if n else float("nan")           # an empty loader: NaN, where the reference divides by zero
    if task.startswith(("mlm", "og")):
        n = r["b"][0]
        return {"loss": div(r["sums"][0], n), "acc": div(r["a"][0], n), "tok_per_s": n / seconds}
    if task.startswith("mrc"):          # train_reverie_obj.py:415-446: KL sum and arg-max agreements over the masked objects
        n = r["b"][0]
        return {"loss": div(r["sums"][0], n), "acc": div(r["a"][0], n), "feat_per_s": n / seconds}
    if task.startswith("sap"):
        n = r["b"][0]
        return {"gloss": div(r["sums"][0], n), "lloss": div(r["sums"][1], n), "floss": div(r["sums"][2], n),
                "gacc": div(r["a"][0], n), "lacc": div(r["a"][1], n), "facc": div(r["a"][2], n), "tok_per_s": n / seconds}
    n = r["a"][0]
    return {"loss": div(r["sums"][0], n), "auc": auc_of(r["U2"], r["P"], r["N"]), "tok_per_s": n / seconds}


@torch.no_grad()
def validate(model, val_loaders, setname="", key_capacity=None, raw=None):
    """train_r2r.py:351-369: ``val_loaders`` maps a task name to an iterable of batches (StaticBatch or collate dicts on
    the device).  Returns {f"val{setname}_{task}_{k}": value} with the reference's keys and divisors.  The model is put
    into eval() and returned to the mode it was in.  ``raw``: a dict that receives the integers and sums of each task."""
    was_training = model.training
    model.eval()
    out = {}
    try:
        dev = next(model.parameters()).device
        for task, loader in val_loaders.items():
            if not task.startswith(("mlm", "mrc", "sap", "og", "sem", "masksem")):
                raise ValueError(f"Undefined task {task}")
            acc = ValAccumulator(dev, key_capacity)
            acc.reset()
            t0 = time.time()
            for batch in loader:
                add_batch(model, task, batch, acc)
            r = acc.finish(auc=task.startswith(("sem", "masksem")))
            if raw is not None:
                raw[task] = r
            for k, v in val_log(task, r, max(time.time() - t0, 1e-9)).items():
                out[f"val{setname}_{task}_{k}"] = v
    finally:
        model.train(was_training)
    return out
