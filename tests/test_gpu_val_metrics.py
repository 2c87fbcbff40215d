"""Validation metrics on the MI355X (csrc/val_metrics.hip, vln_bevbert_amd/validate.py) against the fp64 / integer
restatement of the reference's validation loops (tests/val_metrics_ref.py)."""
import numpy as np
import pytest
import torch

from tests import val_metrics_ref as R
from vln_bevbert_amd import synthetic
from vln_bevbert_amd.config import BevBertConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64_MAX = 0x7fffffffffffffff


@pytest.fixture(scope="module")
def V():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, validate
    lib.load()
    return validate


@pytest.fixture(scope="module", autouse=True)
def _leave_the_runtime_as_found():
    """The training steps below rewrite the process-wide dropout salt (ops.RT) and finalize() sets the residual mode;
    later test files draw random numbers under whatever salt the files before them left, so put both back."""
    from vln_bevbert_amd import lib, ops
    salt = None if ops.RT._salt is None else ops.RT._salt.clone()
    res32 = ops.RT.res32
    yield
    if not torch.cuda.is_available():
        return
    torch.cuda.synchronize()
    if salt is not None:
        ops.RT._salt.copy_(salt)
    elif ops.RT._salt is not None:
        lib.load().bevbert_set_step_salt(None)
        ops.RT._salt = None
    ops.RT.res32 = res32
    torch.cuda.synchronize()


def _np(t):
    return t.float().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def _acc():
    return torch.zeros(3, dtype=torch.int64, device=DEV)


def _read(acc):
    h = acc.cpu()
    return float(h[0:1].view(torch.float64)), int(h[1]), int(h[2])


# ----------------------------------------------------------------------------------------------------- val_ce_rows
def _ce_case(R_, C, dtype, seed):
    """Three batches of (R, C) logits inside a wider buffer (row stride C + 3: rows start on and off 16-byte borders),
    with -inf entries, a maximum tied at three indices, ignored targets and invalid rows wherever the shape has room."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(3):
        x = (torch.randn(R_, C + 3, generator=g) * 2.0).to(dtype)
        t = torch.randint(0, C, (R_,), generator=g)
        valid = torch.ones(R_)
        if C >= 8:
            x[:, 1:C:5][torch.rand(x[:, 1:C:5].shape, generator=g) < 0.3] = float("-inf")
            top = x[:, :C].float().max(1).values + 1.0                      # a maximum tied at three indices, in every row
            for j in (C - 2, C // 2, 3):
                x[:, j] = top.to(dtype)
            t[torch.isinf(x[torch.arange(R_), t])] = C // 2                 # a finite loss: no target on a -inf entry
            t[0::4] = 3                                                     # hits: the lowest tied index
            t[1::4] = C - 2                                                 # misses although the value is the maximum
        if R_ >= 4:
            t[2::7] = -100
            valid[3::5] = 0
        out.append((x, t, valid))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 1), (5, 30522), (64, 1025), (257, 65), (130, 63)])
def test_val_ce_rows_matches_torch_counts_and_the_fp64_loss(V, shape, dtype):
    R_, C = shape
    batches = _ce_case(R_, C, dtype, seed=R_ * 131 + C)
    want_loss, want_hits, want_rows = 0.0, 0, 0
    for x, t, valid in batches:
        keep = valid != 0
        xs, ts = x[:, :C].float()[keep], t[keep]
        want_hits += int((torch.argmax(xs, 1) == ts).sum())                # torch on the CPU
        want_rows += int(keep.sum())
        l, h, n = R.ce_rows(xs.numpy(), ts.numpy())
        assert h == int((torch.argmax(xs, 1) == ts).sum()) and n == int(keep.sum())
        want_loss += l
    runs = []
    for _ in range(2):
        acc = _acc()
        for x, t, valid in batches:
            xd = x.to(DEV)
            assert xd.stride(0) > C
            V.val_ce_rows(xd[:, :C], t.to(DEV), valid.to(DEV), acc)
        runs.append(acc.cpu())
    loss, hits, rows = _read(runs[0])
    assert torch.equal(runs[0], runs[1])                                    # two runs, equal bits
    assert (hits, rows) == (want_hits, want_rows)
    err = abs(loss - want_loss) / max(abs(want_loss), 1e-300) if want_loss else abs(loss)
    print(f"val_ce_rows {shape} {dtype}: loss sum {loss:.9g} fp64 {want_loss:.9g} relative error {err:.2e}")
    assert err <= 1e-6
    # one call alone equals its own batch: the accumulation above was the sum of three
    acc = _acc()
    x, t, valid = batches[1]
    V.val_ce_rows(x.to(DEV)[:, :C], t.to(DEV), None, acc)
    l, h, n = R.ce_rows(x[:, :C].float().numpy(), t.numpy())
    got = _read(acc)
    assert got[1:] == (h, n) and abs(got[0] - l) <= 1e-6 * max(abs(l), 1e-300)


# ------------------------------------------------------------------------------------------ val_bce_keys + val_auc
def _auc_device(V, x, y, valid, C, capacity=None, guard=0):
    """x (R, C) logits, y (R, C) uint8, valid (R) -> (bce, rows, 2U, P, N, overflow, keys buffer)."""
    n = x.numel()
    cap = n if capacity is None else capacity
    keys = torch.full((cap + guard,), -7, dtype=torch.int64, device=DEV)
    acc, out, ovf = _acc(), _acc(), torch.zeros(1, dtype=torch.int64, device=DEV)
    cur = 0
    for lo in range(0, x.shape[0], max(1, (x.shape[0] + 1) // 2)):          # two calls: the cursor moves
        hi = min(x.shape[0], lo + max(1, (x.shape[0] + 1) // 2))
        cur = V.val_bce_keys(x[lo:hi].to(DEV), y.to(DEV), torch.arange(lo, hi, device=DEV), valid[lo:hi].to(DEV), acc, keys, cur,
                             cap, ovf)
    assert cur == n
    sk, _ = torch.sort(keys[:min(cap, n)])
    V.val_auc(sk, out)
    bce, rows, _ = _read(acc)
    o = out.cpu()
    return bce, rows, int(o[0]), int(o[1]), int(o[2]), int(ovf.item()), keys


def _auc_inputs(kind, n, dtype, seed):
    """n elements as (rows, C) with C = 1 for tiny n and 40 otherwise (n = rows C + a remainder folded into one more,
    partly invalid, row is not needed: n is reached exactly with C chosen to divide it)."""
    C = next(c for c in (40, 17, 13, 5, 3, 1) if n % c == 0) if n > 64 else 1
    rows = n // C
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(rows, C, generator=g) < 0.3).to(torch.uint8)
    y.view(-1)[0], y.view(-1)[-1] = 1, 0                                    # P > 0 and N > 0 among the first / last rows
    valid = (torch.rand(rows, generator=g) >= 0.1).float()
    valid[0] = valid[-1] = 1
    x = torch.randn(rows, C, generator=g) * 3
    if kind == "equal":
        x = torch.full((rows, C), 0.75)
    elif kind == "separated":
        x = torch.where(y != 0, x.abs() + 0.5, -x.abs() - 0.5)
    elif kind == "reversed":
        x = torch.where(y != 0, -x.abs() - 0.5, x.abs() + 0.5)
    elif kind == "zeros":                                                   # +0.0 / -0.0 are one tie group
        x = torch.where(torch.rand(rows, C, generator=g) < 0.5, torch.zeros(()), -torch.zeros(()))
        x.view(-1)[0], x.view(-1)[-1] = 0.0, -0.0                           # both signs among the valid rows at any n
    elif kind == "inf":
        m = torch.rand(rows, C, generator=g)
        x = torch.where(m < 0.2, torch.full((), float("inf")), torch.where(m > 0.8, torch.full((), float("-inf")), x))
    elif kind == "ties":
        x = torch.round(x * 2) / 2
    elif kind == "nopos":
        y.zero_()
    return x.to(dtype), y, valid, C


@pytest.mark.parametrize("n", [2, 63, 64, 65, 4097, 2 ** 17 + 3])
def test_val_bce_keys_sort_and_auc_are_exact(V, n):
    for kind, dtype in (("equal", torch.float32), ("separated", torch.float32), ("reversed", torch.float32),
                        ("zeros", torch.float32), ("inf", torch.float32), ("ties", torch.bfloat16), ("random", torch.bfloat16),
                        ("random", torch.float32), ("nopos", torch.float32)):
        x, y, valid, C = _auc_inputs(kind, n, dtype, seed=n + len(kind))
        bce, rows, u2, P, N, ovf, keys = _auc_device(V, x, y, valid, C)
        keep = valid != 0
        xs, ys = x.float().numpy()[keep.numpy()], y.numpy()[keep.numpy()]
        want = R.auc_counts(xs, ys)
        assert (u2, P, N) == want, (kind, n, (u2, P, N), want)
        assert ovf == 0 and rows == int(keep.sum())
        assert int((keys == I64_MAX).sum()) == int((~keep).sum()) * C       # invalid rows left sentinels, nothing else did
        auc = V.auc_of(u2, P, N)
        if kind == "equal":
            assert auc == 0.5
        elif kind == "separated":
            assert auc == 1.0
        elif kind == "reversed":
            assert auc == 0.0
        elif kind == "zeros":
            assert auc == 0.5 and bool((torch.signbit(x) & keep[:, None]).any()) and bool((~torch.signbit(x) & keep[:, None]).any())
        elif kind == "nopos":
            assert P == 0 and np.isnan(auc)
        want_bce, _ = R.bce_sum(xs, ys)
        if np.isfinite(want_bce):                                           # (0 when every kept logit is infinite on its label's side)
            assert abs(bce - want_bce) <= 1e-6 * want_bce, (kind, n, bce, want_bce)
        else:
            assert kind == "inf" and bce == want_bce                        # an infinite logit on the wrong side: +inf, not NaN


def test_val_bce_keys_overflow_sets_the_flag_and_keeps_the_guard_words(V):
    x, y, valid, C = _auc_inputs("random", 4000, torch.float32, seed=5)
    n, half = x.numel(), (x.shape[0] + 1) // 2 * C
    *_, ovf, keys = _auc_device(V, x, y, valid, C, capacity=n - half, guard=64)      # one batch too small
    assert ovf == 1
    assert bool((keys[n - half:] == -7).all())                              # nothing behind the capacity was written
    assert bool((keys[:n - half] != -7).all())
    *_, ovf, keys = _auc_device(V, x, y, valid, C, capacity=n, guard=64)
    assert ovf == 0 and bool((keys[n:] == -7).all())


# ------------------------------------------------------------------------------------------------------ end to end
TASKS = ("mlm", "sap", "masksem", "sem")


def _fresh(cfg, dtype):
    from vln_bevbert_amd import weights
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    model = GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    arena = model.finalize(DEV, dtype, torch.float32 if dtype == torch.bfloat16 else None)   # the bench's default arithmetic
    model.train()
    model.set_dropout(0.1)
    return model, arena


def _restate(task, calls):
    """The reference's val_log from the tensors the kernels consumed (validate.TAP)."""
    if task == "sap":
        trip = [calls[i:i + 3] for i in range(0, len(calls), 3)]
        return R.validate_sap([(_np(g["logits"]), _np(l["logits"]), _np(f["logits"]), _np(g["targets"]), _np(l["targets"]))
                               for g, l, f in trip])
    if task == "mlm":
        loss = hits = n = 0
        for c in calls:
            l, h, k = R.ce_rows(_np(c["logits"]), _np(c["targets"]), _np(c["valid"]))
            loss, hits, n = loss + l, hits + h, n + k
        return {"loss": loss / n, "acc": hits / n, "hits": hits, "n": n}
    xs, ys, loss, rows = [], [], 0.0, 0
    for c in calls:
        keep = _np(c["valid"]) != 0
        x, y = _np(c["logits"])[keep], _np(c["labels"])[_np(c["idx"])][keep]
        l, k = R.bce_sum(x, y)
        loss, rows = loss + l, rows + k
        xs.append(x)
        ys.append(y)
    u2, P, N = R.auc_counts(np.concatenate(xs), np.concatenate(ys))
    return {"loss": loss / rows, "U2": u2, "P": P, "N": N, "rows": rows}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_validate_static_batches_end_to_end(V, dtype, monkeypatch):
    """Three static batches per task: (1) the metrics are the restatement's on exactly the logits, targets and valid flags
    the kernels consumed; (2) those logits are the ``compute_loss=False`` outputs of the same batches, to the tolerance of
    tests/test_gpu_zz_streams.py::test_static_batch_step_equals_the_reference_api_step (1e-5 fp32, 2e-2 bf16, relative
    to max(1, |x|)); (3) a second call, under sync-debug "error" except for the one read-back per task, gives the same
    numbers bit for bit."""
    from vln_bevbert_amd.static_step import StaticBatch
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400, pretrain_tasks=("mlm", "sap", "masksem", "sem"))
    model, arena = _fresh(cfg, dtype)
    tr = PretrainTrainer(model, arena, warmup_steps=2, num_train_steps=20)
    host = {t: [synthetic.make_batch(cfg, t, 3, seed=700 + 10 * i + j, ragged=True, sems_as="ids") for j in range(3)]
            for i, t in enumerate(TASKS)}
    loaders = {t: [StaticBatch(cfg, t, b, DEV) for b in host[t]] for t in TASKS}
    tap, raw1, raw2 = [], {}, {}
    monkeypatch.setattr(V, "TAP", tap)
    log1 = tr.validate(loaders, setname="_seen", raw=raw1)
    monkeypatch.setattr(V, "TAP", None)
    assert model.training                                                   # the mode it was in
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    at = 0
    for task in TASKS:
        k = 9 if task == "sap" else 3
        calls, at = [c for _, c in tap[at:at + k]], at + k
        want, r = _restate(task, calls), raw1[task]
        pre = f"val_seen_{task}_"
        if task == "sap":
            assert r["b"] == [9, 9, 9]
            for i, (lk, ak) in enumerate((("gloss", "gacc"), ("lloss", "lacc"), ("floss", "facc"))):
                assert r["a"][i] == round(want[ak] * 9) and log1[pre + ak] == r["a"][i] / 9
                assert abs(log1[pre + lk] - want[lk]) <= 1e-6 * abs(want[lk]), (task, lk)
        elif task == "mlm":
            assert (r["a"][0], r["b"][0]) == (want["hits"], want["n"]) and log1[pre + "acc"] == want["hits"] / want["n"]
            assert want["n"] == sum(int((b["txt_labels"] != -1).sum()) for b in host[task])
            assert abs(log1[pre + "loss"] - want["loss"]) <= 1e-6 * abs(want["loss"])
            assert calls[0]["logits"].dtype == dtype                        # the head's logits as they come
        else:
            assert (r["U2"], r["P"], r["N"], r["a"][0]) == (want["U2"], want["P"], want["N"], want["rows"]), task
            assert want["P"] > 0 and want["N"] > 0 and log1[pre + "auc"] == want["U2"] / (2 * want["P"] * want["N"])
            assert abs(log1[pre + "loss"] - want["loss"]) <= 1e-6 * abs(want["loss"])
        assert log1[pre + "tok_per_s"] > 0
        # (2) against the reference API on the same batches
        with torch.no_grad():
            model.eval()
            for j, b in enumerate(host[task]):
                plain = model(synthetic.batch_to(b, DEV), task, compute_loss=False)
                if task == "sap":
                    pairs = [(calls[3 * j + i]["logits"], plain[i]) for i in range(3)]
                    assert torch.equal(calls[3 * j]["targets"], plain[3]) and torch.equal(calls[3 * j + 1]["targets"], plain[4])
                elif task == "mlm":
                    n = plain.shape[0]
                    assert int(calls[j]["valid"].sum()) == n and bool((calls[j]["valid"][:n] == 1).all())
                    pairs = [(calls[j]["logits"][:n], plain)]
                else:
                    keep = calls[j]["valid"] != 0
                    pairs = [(calls[j]["logits"][keep], plain[0])]
                    assert torch.equal(calls[j]["labels"][calls[j]["idx"]][keep].float(), plain[1])
                for got, ref in pairs:
                    got, ref = got.float()[:, :ref.shape[1]], ref.float()
                    assert got.shape == ref.shape, (task, got.shape, ref.shape)
                    assert torch.equal(torch.isinf(got), torch.isinf(ref))
                    fin = torch.isfinite(ref)
                    scale = max(1.0, float(ref[fin].abs().max()))
                    assert float((got[fin] - ref[fin]).abs().max()) <= tol * scale, (task, j)
            model.train()
    assert at == len(tap)
    # (3) no synchronisation but the read-back, and the same bits
    reads = []
    real = V._read_back

    def read_back(t):
        torch.cuda.set_sync_debug_mode("default")
        try:
            reads.append(1)
            return real(t)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    monkeypatch.setattr(V, "_read_back", read_back)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        log2 = tr.validate(loaders, setname="_seen", raw=raw2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(reads) == len(TASKS)
    assert raw1 == raw2
    assert {k: v for k, v in log1.items() if not k.endswith("tok_per_s")} == \
        {k: v for k, v in log2.items() if not k.endswith("tok_per_s")}
    assert set(log1) == {f"val_seen_{t}_{k}" for t, ks in (("mlm", ("loss", "acc", "tok_per_s")),
                                                          ("sap", ("gloss", "lloss", "floss", "gacc", "lacc", "facc", "tok_per_s")),
                                                          ("masksem", ("loss", "auc", "tok_per_s")),
                                                          ("sem", ("loss", "auc", "tok_per_s"))) for k in ks}


def test_validate_plain_batches_use_the_same_kernels(V):
    """Collate dicts go through ``compute_loss=False`` and the same kernels: the numbers of the static path on the same
    batches, to the static-versus-plain tolerance (fp32: 1e-5), counts exactly."""
    from vln_bevbert_amd.static_step import StaticBatch
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    model, _ = _fresh(cfg, torch.float32)
    host = {t: [synthetic.make_batch(cfg, t, 3, seed=760 + j, ragged=True, sems_as="ids") for j in range(2)]
            for t in ("mlm", "sap", "masksem")}
    rs, rp = {}, {}
    V.validate(model, {t: [StaticBatch(cfg, t, b, DEV) for b in bs] for t, bs in host.items()}, raw=rs)
    V.validate(model, {t: [synthetic.batch_to(b, DEV) for b in bs] for t, bs in host.items()}, raw=rp)
    for t in host:
        assert rs[t]["b"] == rp[t]["b"] and rs[t]["a"] == rp[t]["a"] and (rs[t]["P"], rs[t]["N"]) == (rp[t]["P"], rp[t]["N"]), t
        for a, b in zip(rs[t]["sums"], rp[t]["sums"]):
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), t
    assert model.training


def test_validation_leaves_training_untouched(V):
    """train 2 steps == train 1 step, validate, train 1 step: master parameters and AdamW moments bit for bit (dropout on:
    the second step's masks depend on the step counter alone)."""
    from vln_bevbert_amd.static_step import StaticBatch
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    state = {}
    for with_val in (False, True):
        model, arena = _fresh(cfg, torch.bfloat16)
        tr = PretrainTrainer(model, arena, learning_rate=1e-4, warmup_steps=2, num_train_steps=20)
        # the gradient fill in line: an arena's fill stream is one more draw from torch's cyclic stream pool, and the test
        # files after this one are sensitive to where in the pool their own streams land
        tr.overlap_zero = False
        sbs = {t: StaticBatch(cfg, t, synthetic.make_batch(cfg, t, 3, seed=800, ragged=True, sems_as="ids"), DEV)
               for t in ("mlm", "masksem")}
        val = {t: [StaticBatch(cfg, t, synthetic.make_batch(cfg, t, 3, seed=801, ragged=True, sems_as="ids"), DEV)]
               for t in ("mlm", "sap", "masksem")}
        tr.step("mlm", sbs["mlm"])
        if with_val:
            log = tr.validate(val)
            assert all(np.isfinite(v) for v in log.values()), log
        tr.step("masksem", sbs["masksem"])
        torch.cuda.synchronize()
        state[with_val] = (arena.params.clone(), arena.exp_avg.clone(), arena.exp_avg_sq.clone())
    for a, b in zip(state[False], state[True]):
        assert torch.equal(a, b)
