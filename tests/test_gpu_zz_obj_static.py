"""Object-token batches (REVERIE / SOON) as static, capturable batches on the MI355X: static_step.StaticBatch with
``obj_static=True`` against the reference-API path, captured and refilled, replayed against eager, and MRC / OG validation
on such batches (validate.py, bevbert_val_kl_rows).  It captures graphs, so it sorts behind the parity tests like
tests/test_gpu_zz_streams.py; the batches are those of tests/obj_static_cases.py (tests/test_obj_static_host.py pins their
tables and their shared bucket on the CPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.obj_static_cases import CFG, SEED_A, SEED_B, SHAPES_A, SHAPES_B, make
from vln_bevbert_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
TASKS = ("mlm", "mrc", "sap", "og")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib
    lib.load()
    return True


def _fresh(dtype, dropout=0.1):
    from vln_bevbert_amd import weights
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    model = GlocalTextPathCMTPreTraining(CFG)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    arena = model.finalize(DEV, dtype)
    model.train()
    model.set_dropout(dropout)
    return model, arena


def _static(task, seed=SEED_A, shapes=SHAPES_A):
    from vln_bevbert_amd.static_step import StaticBatch
    return StaticBatch(CFG, task, make(seed, task, shapes), DEV, obj_static=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_obj_static_batch_step_equals_the_reference_api_step(env, dtype):
    """Padded panoramas / views / objects / joint axis / object width and the loader-built tables give the loss and the
    arena gradients of the same batch fed through the reference API: every padding entry carries exactly zero weight.
    Tolerances of test_static_batch_step_equals_the_reference_api_step."""
    from vln_bevbert_amd import ops
    model, arena = _fresh(dtype, dropout=0.0)
    for task in TASKS:
        cpu = make(SEED_A, task)
        sb = _static(task)
        assert sb.capturable
        res = []
        for which in ("api", "static", "api", "static"):            # the first two settle the library plans
            ops.RT.new_step(5)
            arena.zero_grad()
            if which == "api":
                loss = model(synthetic.batch_to(cpu, DEV), task).mean()
            else:
                loss = model.loss_mean(sb.tensors, task)
            loss.backward()
            arena.sync()
            torch.cuda.synchronize()
            res.append((float(loss), arena.grads.clone()))
        (la, ga), (ls, gs_) = res[2], res[3]
        print(f"obj_static {task} {dtype}: api {la:.8g} static {ls:.8g} relative gradient distance {float((ga - gs_).norm() / ga.norm()):.2e}")
        assert np.isfinite(la) and float(ga.norm()) > 0
        tol = 1e-5 if dtype == torch.float32 else 2e-2
        assert abs(la - ls) <= tol * max(1.0, abs(la)), (task, la, ls)
        rel = float((ga - gs_).norm() / ga.norm())
        assert rel < (1e-4 if dtype == torch.float32 else 5e-2), (task, rel)


@pytest.mark.parametrize("task", ["mrc", "sap"])
def test_obj_static_batch_is_captured_and_a_refill_replays_the_new_batch(env, task):
    """The step on an object batch is captured; a refill with a batch of OTHER per-sample step counts and per-panorama object
    counts (same bucket) is replayed with that batch's tables: its loss is the reference-API loss of that batch.  A table
    the forward still derived on the host would be frozen in the graph and give the first batch's rows."""
    from vln_bevbert_amd.train import PretrainTrainer
    model, arena = _fresh(torch.float32, dropout=0.0)
    tr = PretrainTrainer(model, arena, learning_rate=0.0, warmup_steps=1, num_train_steps=10)
    sb = _static(task)
    first = [float(tr.step(task, sb)) for _ in range(tr.GRAPH_WARMUP + 1)]
    assert sb.graph is not None and tr.graph_error is None
    other = make(SEED_B, task, SHAPES_B)
    assert other["traj_step_lens"] != make(SEED_A, task)["traj_step_lens"]
    with torch.no_grad():                               # before the step: the step's optimiser moves the weights
        want = float(model(synthetic.batch_to(other, DEV), task).mean())
    sb.load(other)
    got = float(tr.step(task, sb))
    assert sb.graph is not None and tr.graph_error is None
    print(f"obj_static refill {task}: replayed {got:.8g} reference API {want:.8g} (first batch {first[-1]:.8g})")
    assert abs(first[-1] - want) > 1e-4 * max(1.0, abs(want))        # the two batches are told apart by their loss
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)


def test_captured_object_steps_replay_the_eager_steps(env):
    """hipGraph path against eager path on obj_static batches, same weights and (seed, step) sequence, dropout ON, lr > 0:
    four passes over the four tasks (two eager uses, the capture, one replay each).  First step bit for bit; later steps to
    the 5e-4 of test_captured_step_replays_the_eager_step (the reasons are given there)."""
    from vln_bevbert_amd.train import PretrainTrainer
    seq = TASKS * 4
    curves, finals = {}, {}
    for graphs in (False, True):
        model, arena = _fresh(torch.bfloat16)
        tr = PretrainTrainer(model, arena, learning_rate=1e-4, warmup_steps=4, num_train_steps=40)
        tr.use_graphs = graphs
        sbs = {t: _static(t) for t in TASKS}
        out = [float(tr.step(t, sbs[t])) for t in seq]
        torch.cuda.synchronize()
        assert tr.graph_error is None
        assert all((sb.graph is not None) == graphs for sb in sbs.values())
        curves[graphs], finals[graphs] = np.asarray(out), arena.params.clone()
    e, g = curves[False], curves[True]
    print("obj_static eager  ", e, "\nobj_static replay ", g)
    assert np.isfinite(g).all()
    assert e[0] == g[0], (e[0], g[0])
    assert np.max(np.abs(e - g) / np.maximum(1.0, np.abs(e))) < 5e-4, (e, g)
    rel = float((finals[False] - finals[True]).norm() / finals[False].norm())
    assert rel < 1e-4, rel


# ----------------------------------------------------------------------------- validation
def _lowest_argmax(x):
    C = x.shape[1]
    at = x == x.max(1, keepdim=True).values
    return torch.where(at, torch.arange(C)[None, :].expand_as(x), torch.full_like(x, C, dtype=torch.int64)).min(1).values


def kl_ref(logits, targets, idx, valid, dt=torch.float64):
    """(KL sum, arg-max agreements with the lowest index on a tie, rows) over the valid rows, logits as the kernel got them."""
    x = logits.detach().cpu().to(dt)
    t = targets.detach().cpu()
    t = (t if idx is None else t.index_select(0, idx.cpu())).to(dt)
    on = torch.ones(x.shape[0], dtype=torch.bool) if valid is None else valid.cpu() != 0
    x, t = x[on], t[on]
    loss = F.kl_div(F.log_softmax(x, -1), t, reduction="none").sum()
    return float(loss), int((_lowest_argmax(x) == _lowest_argmax(t)).sum()), int(on.sum())


def _check_kl(V, tapped, r):
    (entry, seen), = tapped
    assert entry == "val_kl_rows"
    want, hits, rows = kl_ref(seen["logits"], seen["targets"], seen["idx"], seen["valid"])
    w32, _, _ = kl_ref(seen["logits"].float(), seen["targets"], seen["idx"], seen["valid"], torch.float32)
    gate = max(1e-6 * abs(want), 4.0 * abs(w32 - want))
    print(f"val_kl_rows {tuple(seen['logits'].shape)} {seen['logits'].dtype}: sum {r['sums'][0]:.9g} fp64 {want:.9g} "
          f"error {abs(r['sums'][0] - want):.2e} torch-fp32 {abs(w32 - want):.2e} gate {gate:.2e}")
    assert r["a"][0] == hits and r["b"][0] == rows
    assert abs(r["sums"][0] - want) <= gate, (r["sums"][0], want, gate)
    return want, hits, rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_mrc_validation_on_static_batches_and_collate_dicts(env, dtype, monkeypatch):
    from vln_bevbert_amd import validate as V
    model, _ = _fresh(dtype)
    cpu = make(SEED_A, "mrc")
    n = int(cpu["vp_obj_mrc_masks"].sum())
    results = {}
    for kind, batch in (("static", _static("mrc")), ("dict", synthetic.batch_to(cpu, DEV))):
        tap, raw = [], {}
        monkeypatch.setattr(V, "TAP", tap)
        out = V.validate(model, {"mrc": [batch]}, raw=raw)
        monkeypatch.setattr(V, "TAP", None)
        assert set(out) == {"val_mrc_loss", "val_mrc_acc", "val_mrc_feat_per_s"}
        want, hits, rows = _check_kl(V, tap, raw["mrc"])
        assert rows == n
        assert out["val_mrc_loss"] == raw["mrc"]["sums"][0] / n and out["val_mrc_acc"] == hits / n
        assert out["val_mrc_feat_per_s"] > 0
        results[kind] = out["val_mrc_loss"]
    assert model.training                                  # validate returns the model to the mode it was in
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert abs(results["static"] - results["dict"]) <= tol * max(1.0, abs(results["dict"])), results


def test_og_validation_runs_on_an_obj_static_batch(env):
    from vln_bevbert_amd import validate as V
    model, _ = _fresh(torch.float32)
    cpu = make(SEED_A, "og")
    raws = {}
    for kind, batch in (("static", _static("og")), ("dict", synthetic.batch_to(cpu, DEV))):
        raws[kind] = {}
        out = V.validate(model, {"og": [batch]}, raw=raws[kind])
        assert set(out) == {"val_og_loss", "val_og_acc", "val_og_tok_per_s"} and np.isfinite(out["val_og_loss"])
    s, d = raws["static"]["og"], raws["dict"]["og"]
    assert s["b"][0] == d["b"][0] == 3 and s["a"][0] == d["a"][0]
    assert abs(s["sums"][0] - d["sums"][0]) <= 1e-5 * max(1.0, abs(d["sums"][0])), (s, d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_add_kl_ties_take_the_lowest_index_on_both_sides(env, dtype):
    """Ties in the logits and in the targets, in the one-wave rows (C = 4) and across the waves of the one-workgroup rows
    (C = 1500); rows read through an index with a duplicate; a row with valid == 0 adds nothing."""
    from vln_bevbert_amd import validate as V
    small_x = torch.tensor([[1., 3., 3., 0.], [5., 5., 1., 1.], [0., 0., 2., 2.], [9., 1., 1., 1.], [4., 0., 0., 0.]])
    small_t = torch.tensor([[.2, .4, .4, 0.], [0., .5, .5, 0.], [.1, .1, .4, .4], [0., 0., 0., 0.], [1., 0., 0., 0.]])
    big_x = torch.randn(4, 1500, generator=torch.Generator().manual_seed(2))
    big_t = torch.softmax(torch.randn(3, 1500, generator=torch.Generator().manual_seed(3)), -1)
    big_x[0, 70] = big_x[0, 1400] = 8.0
    big_t[0, 70] = big_t[0, 900] = 0.25                         # both sides tie: 70 == 70 -> hit
    big_x[1, 300] = big_x[1, 20] = 8.0
    big_t[1, 300] = 0.5                                         # logits: 20 (lowest of the tie), target: 300 -> miss
    big_x[2, 1499] = 9.0
    big_t[2, 1499] = big_t[2, 1498] = 0.5                       # logits: 1499, target: 1498 -> miss
    big_x[3, 1498] = 9.0                                        # reads target row 2 through the index: 1498 == 1498 -> hit
    cases = [(small_x, small_t, None, torch.tensor([1., 1., 1., 1., 0.]), 3, 4),
             (big_x, big_t, torch.tensor([0, 1, 2, 2]), None, 2, 4)]
    for x, t, idx, valid, want_hits, want_rows in cases:
        acc = V.ValAccumulator(DEV)
        acc.reset()
        xd = x.to(dtype).to(DEV)
        acc.add_kl(xd, t.to(DEV), None if idx is None else idx.to(DEV), None if valid is None else valid.to(DEV))
        r = acc.finish()
        want, hits, rows = kl_ref(xd, t, idx, valid)
        w32, _, _ = kl_ref(xd.float(), t, idx, valid, torch.float32)
        assert (hits, rows) == (want_hits, want_rows)           # the restatement itself
        assert r["a"][0] == hits and r["b"][0] == rows, (r, hits, rows)
        assert abs(r["sums"][0] - want) <= max(1e-6 * abs(want), 4.0 * abs(w32 - want)), (r["sums"][0], want, w32)
