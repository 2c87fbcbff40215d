"""ms per validation batch, device metrics against the reference-style loop, on the bench's R2R shapes.

    python scripts/bench_validate.py [--batch 64] [--rounds 9] [--out profiles/validate_bench.txt]

Two variants on ONE model (bf16 compute, fp32 residual, eval), the same two host batches per task, run in turns in one
process; the median over the rounds is reported:
  device     vln_bevbert_amd.validate (ValAccumulator, add_batch, finish) on static batches: no synchronisation inside,
             one read-back per pass
  (model.eval() / model.train(), which both loops pay once per validation, not per batch, are outside the timing)
  reference  the loop of pretrain_src/train_r2r.py:372-510: model(batch, task, compute_loss=False) on collate dicts,
             F.cross_entropy / argmax / BCE with one .item() per metric and batch, SEM logits copied to the host and
             sklearn's roc_auc_score on their sigmoid once per pass (left out, and said so, where sklearn is missing)
A pass is the two batches of a task; its time runs from a device synchronise to the last number on the host.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vln_bevbert_amd import synthetic, validate  # noqa: E402
from vln_bevbert_amd.config import BevBertConfig  # noqa: E402
from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining  # noqa: E402
from vln_bevbert_amd.static_step import StaticBatch  # noqa: E402

try:
    from sklearn.metrics import roc_auc_score
except ImportError:
    roc_auc_score = None


@torch.no_grad()
def device_pass(model, task, batches):
    acc = validate.ValAccumulator(batches[0].device)
    acc.reset()
    for b in batches:
        validate.add_batch(model, task, b, acc)
    return validate.val_log(task, acc.finish(auc=task == "masksem"), 1.0)


@torch.no_grad()
def reference_pass(model, task, batches):
    if task == "mlm":
        loss = hits = n = 0
        for b in batches:
            scores = model(b, task, compute_loss=False)
            labels = b["txt_labels"]
            labels = labels[labels != -1]
            loss += F.cross_entropy(scores, labels, reduction="sum").item()
            hits += (scores.max(dim=-1)[1] == labels).sum().item()
            n += labels.numel()
        return {"loss": loss / n, "acc": hits / n}
    if task == "sap":
        s, h, n = [0.0] * 3, [0] * 3, 0
        for b in batches:
            g, l, f, gl, ll = model(b, task, compute_loss=False)
            for i, (x, t) in enumerate(((g, gl), (l, ll), (f, gl))):
                s[i] += F.cross_entropy(x, t, reduction="sum").item()
                h[i] += torch.sum(torch.argmax(x, 1) == t).item()
            n += len(gl)
        return {"gloss": s[0] / n, "lloss": s[1] / n, "floss": s[2] / n, "gacc": h[0] / n, "lacc": h[1] / n, "facc": h[2] / n}
    loss, rows, outs, tgts = 0.0, 0, [], []
    for b in batches:
        logits, labels = model(b, task, compute_loss=False)
        outs.append(logits.cpu())
        tgts.append(labels.cpu())
        loss += F.binary_cross_entropy_with_logits(logits, labels, reduction="sum").cpu().item()
        rows += labels.size(0)
    out = {"loss": loss / rows}
    if roc_auc_score is not None:
        out["auc"] = roc_auc_score(y_score=torch.cat(outs).sigmoid().numpy(), y_true=torch.cat(tgts).numpy(), average="micro")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_validate.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    cfg = BevBertConfig()
    torch.manual_seed(0)
    model = GlocalTextPathCMTPreTraining(cfg)
    model.finalize(dev, torch.bfloat16, torch.float32)
    model.eval()
    tasks = ("mlm", "sap", "masksem")
    host = {t: [synthetic.make_batch(cfg, t, a.batch, seed=1000 + 97 * j, sems_as="ids") for j in range(2)] for t in tasks}
    static = {t: [StaticBatch(cfg, t, b, dev) for b in host[t]] for t in tasks}
    plain = {t: [synthetic.batch_to(b, dev) for b in host[t]] for t in tasks}
    times = {(v, t): [] for v in ("device", "reference") for t in tasks}
    last = {}
    for r in range(a.warmup + a.rounds):
        for t in tasks:
            for v in ("device", "reference"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if v == "device":
                    last[(v, t)] = device_pass(model, t, static[t])
                else:
                    last[(v, t)] = reference_pass(model, t, plain[t])
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[(v, t)].append((time.perf_counter() - t0) * 1e3 / len(host[t]))
    lines = [f"validation, ms per batch: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, R2R model, batch {a.batch}, "
             f"bf16 + fp32 residual, eval, 2 batches per pass, median of {a.rounds} rounds after {a.warmup} warm-up rounds, "
             f"variants in turns in one process; sklearn {'present' if roc_auc_score is not None else 'MISSING: the reference loop ran without its AUC'}",
             f"{'task':8s} {'device':>10s} {'reference':>10s} {'ratio':>7s}   (min .. max per variant)"]
    for t in tasks:
        d, f = times[("device", t)], times[("reference", t)]
        md, mf = statistics.median(d), statistics.median(f)
        lines.append(f"{t:8s} {md:10.3f} {mf:10.3f} {mf / md:7.2f}   device {min(d):.3f} .. {max(d):.3f}, reference {min(f):.3f} .. {max(f):.3f}")
    for t in tasks:
        dv = {k: round(v, 6) for k, v in last[("device", t)].items() if k != "tok_per_s"}
        lines.append(f"{t}: device {dv} reference { {k: round(float(v), 6) for k, v in last[('reference', t)].items()} }")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
