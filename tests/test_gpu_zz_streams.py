"""Stream / collective plumbing of the training step on the MI355X (sorts after the parity tests on purpose: these
compare the product with ITSELF under different launch orders; every oracle / golden comparison runs before them).

  * the RCCL exchange (side stream, text-embedding hook, in-place all-reduce of arena slices) on a one-rank group must
    leave exactly the gradients of a run without collectives -- compared BEFORE clip + AdamW, where a difference means
    an ordering bug and not chaotic amplification of fp32 summation order;
  * the precondition of the overlapped phase A: the arena region it reduces is final when the hook fires.
"""
import os
import socket

import numpy as np
import pytest
import torch

from vln_bevbert_amd import synthetic
from vln_bevbert_amd.config import BevBertConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"

@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib
    lib.load()
    return True


def _fresh(cfg, dtype):
    from vln_bevbert_amd import weights
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    model = GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    arena = model.finalize(DEV, dtype)
    model.train()
    model.set_dropout(0.1)
    return model, arena


@pytest.fixture(scope="module")
def one_rank_group(env):
    import torch.distributed as dist
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rccl_reducer_leaves_the_gradients_of_a_run_without_collectives(one_rank_group, dtype):
    """One backward per task with the collectives forced / not forced, same (seed, step): ``arena.grads`` before
    clip + AdamW.  A one-rank all-reduce is the identity, so the two must agree bit for bit (no atomics on the path;
    pretrain_src/utils/misc.py:64-77 semantics: the wrapper changes where gradients are summed, never their value)."""
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=2, num_x_layers=2, vocab_size=400)
    grads = {}
    for force in (None, False, True):            # the first pass only settles the hipBLASLt plans
        model, arena = _fresh(cfg, dtype)
        tr = PretrainTrainer(model, arena, warmup_steps=2, num_train_steps=20, force_collectives=bool(force))
        assert tr.reducer.active == bool(force) and tr.overlap == bool(force)
        for i, task in enumerate(("sap", "mlm", "masksem")):
            b = synthetic.batch_to(synthetic.make_batch(cfg, task, 3, seed=80 + i, ragged=True), DEV)
            loss = tr.forward_backward(task, b)
            torch.cuda.synchronize()
            grads[(force, task)] = (float(loss), arena.grads.clone())
    for task in ("sap", "mlm", "masksem"):
        (l0, g0), (l1, g1) = grads[(False, task)], grads[(True, task)]
        assert l0 == l1, task
        assert float(g0.norm()) > 0
        bad = (g0 != g1).nonzero()
        if bad.numel():
            off = int(bad[0])
            name = [n for n, (o, k) in arena.slices.items() if o <= off < o + k]
            raise AssertionError(f"{task}: {bad.shape[0]} gradient elements differ with the collectives on, first in {name}")


def test_four_steps_with_forced_collectives_track_a_run_without(one_rank_group):
    """Smoke of the whole step (hook, side stream, clip, AdamW) with the exchange on: finite, and the losses of four
    steps agree with a run without collectives to 1e-3 (parameters after AdamW are NOT compared: bias-corrected Adam
    turns last-bit differences of near-zero gradients into +-lr updates)."""
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    curves = {}
    for force in (None, False, True):
        model, arena = _fresh(cfg, torch.bfloat16)
        tr = PretrainTrainer(model, arena, warmup_steps=2, num_train_steps=20, force_collectives=bool(force))
        out = []
        for i, task in enumerate(("sap", "mlm", "masksem", "sap")):
            out.append(float(tr.step(task, synthetic.batch_to(synthetic.make_batch(cfg, task, 2, seed=80 + i, ragged=True), DEV))))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(arena.params).all())
        curves[force] = np.asarray(out)
    assert np.isfinite(curves[True]).all()
    assert np.max(np.abs(curves[True] - curves[False]) / np.maximum(1.0, np.abs(curves[False]))) < 1e-3, curves


def test_a_failed_capture_with_collectives_active_continues_eagerly_on_the_same_curve(one_rank_group, monkeypatch):
    """a rank whose hipGraph capture fails must not leave the group -- it redoes the step eagerly and
    keeps issuing the SAME sequence of collectives per step as the ranks that replay their graphs (regions in hook order,
    then the remainder), with nothing of the dead capture left behind (deferred weight-gradient closures, queued
    reductions, collective work handles).  Injected here on a one-rank RCCL group with forced collectives: the capture
    of the third use of each batch raises at the top of the captured step; the run must continue, report the error, and
    reproduce the losses of a run that never tried to capture -- bit for bit (training is deterministic)."""
    from vln_bevbert_amd import train
    from vln_bevbert_amd.static_step import StaticBatch
    cfg = BevBertConfig.tiny(num_l_layers=2, num_x_layers=2, vocab_size=400)
    seq = ("sap", "mlm") * 4
    real = train.PretrainTrainer._forward_backward

    def failing(self, task, batch):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("injected capture failure")
        return real(self, task, batch)

    curves, calls = {}, {}
    for mode in ("eager", "capture_fails"):
        model, arena = _fresh(cfg, torch.bfloat16)
        tr = train.PretrainTrainer(model, arena, learning_rate=1e-4, warmup_steps=2, num_train_steps=40,
                                   force_collectives=True)
        assert tr.reducer.active
        tr.use_graphs = mode != "eager"
        n_coll = [0]
        launch = tr.reducer._launch

        def counted(lo, hi, launch=launch, n_coll=n_coll):
            n_coll[0] += 1
            return launch(lo, hi)
        tr.reducer._launch = counted
        if mode == "capture_fails":
            monkeypatch.setattr(train.PretrainTrainer, "_forward_backward", failing)
        sbs = {t: StaticBatch(cfg, t, synthetic.make_batch(cfg, t, 3, seed=90, ragged=True, sems_as="ids"), DEV)
               for t in ("sap", "mlm")}
        with pytest.warns(UserWarning, match="capture") if mode == "capture_fails" else _no_warning():
            curves[mode] = np.asarray([float(tr.step(t, sbs[t])) for t in seq])
        torch.cuda.synchronize()
        calls[mode] = n_coll[0]
        if mode == "capture_fails":
            assert tr.graph_error is not None and "injected" in tr.graph_error and tr.use_graphs is False
            assert all(sb.graph is None for sb in sbs.values())
            monkeypatch.setattr(train.PretrainTrainer, "_forward_backward", real)
        assert not tr.reducer._works and not tr.reducer._done
    assert calls["eager"] == calls["capture_fails"], calls               # the same collectives, step for step
    assert np.array_equal(curves["eager"], curves["capture_fails"]), curves


class _no_warning:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_phase_a_gradients_are_final_when_the_text_hook_fires(env, dtype):
    """The overlapped all-reduce (train.GradReducer.phase_a) reduces the arena region [split, end) -- map encoders and
    heads -- as soon as d loss / d text-embeddings is complete.  That is only correct if every kernel that writes that
    region has been issued by then (a one-rank RCCL group cannot show a violation: its all-reduce is the identity).
    Snapshot the region at the moment the hook fires and compare with the region after the whole backward."""
    from vln_bevbert_amd import ops
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=2, num_x_layers=2, vocab_size=400)
    model, arena = _fresh(cfg, dtype)
    split = PretrainTrainer(model, arena, overlap=False).reducer.split
    assert 0 < split < arena.numel
    snap = {}

    def at_hook(g):
        ops.WgradStream.flush_all()                  # what GradReducer._launch does before it issues the collective
        torch.cuda.synchronize()
        snap["region"] = arena.grads[split:].clone()
        return g

    def fwd_hook(mod, inputs, output):
        if output.requires_grad and torch.is_grad_enabled():
            output.register_hook(at_hook)

    handle = model.bert.lang_encoder.register_forward_hook(fwd_hook)
    try:
        for step, task in enumerate(("sap", "mlm", "masksem")):
            snap.clear()
            ops.RT.new_step(500 + step)
            arena.zero_grad()
            b = synthetic.batch_to(synthetic.make_batch(cfg, task, 3, seed=90 + step, ragged=True), DEV)
            model(b, task).mean().backward()
            arena.sync()
            torch.cuda.synchronize()
            assert "region" in snap, task                # the hook fired: every task here reads the text encoder
            final = arena.grads[split:]
            late = (snap["region"] != final).nonzero()
            if late.numel():
                off = int(late[0]) + split
                name = [n for n, (o, k) in arena.slices.items() if o <= off < o + k]
                raise AssertionError(f"{task}: {late.shape[0]} gradient elements of [split, end) changed after the "
                                     f"text hook, first in {name}")
            assert float(final.abs().sum()) > 0
    finally:
        handle.remove()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_text_layer_regions_are_final_when_their_hooks_fire(env, dtype):
    """Phase B of the gradient exchange is pipelined through the text encoder's backward: the arena region of the text
    layers >= k is all-reduced when d loss / d (input of layer k) is complete (train.PretrainTrainer.text_layer_regions).
    Same check as for phase A: snapshot each region when its hook fires (after the flush GradReducer._launch does),
    compare with the region after the whole backward -- bit for bit, for every task."""
    from vln_bevbert_amd import ops
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=4, num_x_layers=1, vocab_size=400)
    model, arena = _fresh(cfg, dtype)
    regions = PretrainTrainer.text_layer_regions(model, arena, "1,2,3")
    assert [k for k, _, _ in regions] == [3, 2, 1] and all(lo < hi for _, lo, hi in regions)
    n3 = sum(k for n, (o, k) in arena.slices.items() if n.startswith("bert.lang_encoder.layer.3."))
    assert n3 <= regions[0][2] - regions[0][1] < n3 + 1024 * 32          # (tensors start on 1024-element boundaries)
    auto = PretrainTrainer.text_layer_regions(model, arena, "auto")
    assert [k for k, _, _ in auto] == [3, 1]
    snap, handles = {}, []

    def make(k, lo, hi):
        def at_hook(g):
            ops.WgradStream.flush_all()
            torch.cuda.synchronize()
            snap[k] = arena.grads[lo:hi].clone()
            return g

        def pre_hook(mod, inputs):
            if inputs[0].requires_grad and torch.is_grad_enabled():
                inputs[0].register_hook(at_hook)
        return pre_hook

    for k, lo, hi in regions:
        handles.append(model.bert.lang_encoder.layer[k].register_forward_pre_hook(make(k, lo, hi)))
    try:
        for step, task in enumerate(("sap", "mlm", "masksem")):
            snap.clear()
            ops.RT.new_step(700 + step)
            arena.zero_grad()
            b = synthetic.batch_to(synthetic.make_batch(cfg, task, 3, seed=95 + step, ragged=True), DEV)
            model(b, task).mean().backward()
            arena.sync()
            torch.cuda.synchronize()
            for k, lo, hi in regions:
                assert k in snap, (task, k)
                final = arena.grads[lo:hi]
                late = (snap[k] != final).nonzero()
                if late.numel():
                    off = int(late[0]) + lo
                    name = [n for n, (o, kk) in arena.slices.items() if o <= off < o + kk]
                    raise AssertionError(f"{task}: {late.shape[0]} gradient elements of text layers >= {k} changed after "
                                         f"their hook, first in {name}")
                assert float(final.abs().sum()) > 0
    finally:
        for h in handles:
            h.remove()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_map_layer_regions_are_final_when_their_hooks_fire(env, dtype):
    """Round 5: the gradient exchange follows backward THROUGH the map encoders -- the heads' region and the region of every
    x-layer k >= 1 of the local / global encoder go out when d loss / d (streaming input of layer k) is complete
    (train.PretrainTrainer.map_layer_regions / install_map_layer_hooks).  Same check as for the other phases: snapshot each
    region when the trainer's hook would launch it (after the flush GradReducer._launch does) and compare with the region
    after the whole backward, bit for bit, for every task -- including that the hoisted K | V projections, whose gradient
    is final only at the end of an encoder, are outside every layer region."""
    from vln_bevbert_amd import ops
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=2, num_x_layers=3, vocab_size=400)
    model, arena = _fresh(cfg, dtype)
    tr = PretrainTrainer(model, arena, overlap=False)
    tr.install_map_layer_hooks()
    regions = tr._map_regions
    assert set(regions) == {"heads", ("local", 1), ("local", 2), ("global", 1), ("global", 2)}
    for enc in ("local", "global"):
        kv = {n for grp in getattr(model.bert, f"{enc}_encoder").encoder.arena_groups(f"bert.{enc}_encoder.encoder.") for n in grp}
        for n in kv:
            o, _ = arena.slices[n]
            assert not any(lo <= o < hi for key, (lo, hi) in regions.items() if key != "heads"), n
    snap = {}

    class Spy:                                       # stands in for the reducer: records instead of reducing
        active = True

        def launch_region(self, lo, hi):
            ops.WgradStream.flush_all()
            torch.cuda.synchronize()
            snap[(lo, hi)] = arena.grads[lo:hi].clone()

    real, tr.reducer = tr.reducer, Spy()
    try:
        for step, task in enumerate(("sap", "mlm", "masksem")):
            snap.clear()
            tr._reset_map_hooks()
            ops.RT.new_step(900 + step)
            arena.zero_grad()
            b = synthetic.batch_to(synthetic.make_batch(cfg, task, 3, seed=60 + step, ragged=True), DEV)
            model(b, task).mean().backward()
            arena.sync()
            torch.cuda.synchronize()
            want = {"heads", ("local", 1), ("local", 2)} | ({("global", 1), ("global", 2)} if task != "masksem" else set())
            assert {k for k, r in regions.items() if r in snap} >= want, (task, sorted(map(str, snap)))
            for (lo, hi), got in snap.items():
                final = arena.grads[lo:hi]
                late = (got != final).nonzero()
                if late.numel():
                    off = int(late[0]) + lo
                    name = [n for n, (o, kk) in arena.slices.items() if o <= off < o + kk]
                    raise AssertionError(f"{task}: {late.shape[0]} gradient elements of region [{lo}, {hi}) changed after "
                                         f"its hook, first in {name}")
                assert float(final.abs().sum()) > 0 or task == "masksem"
    finally:
        tr.reducer = real
        for enc in ("local", "global"):
            getattr(model.bert, f"{enc}_encoder").encoder.region_hook = None


# ----------------------------------------------------------------------------- static batches and captured steps
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_static_batch_step_equals_the_reference_api_step(env, dtype):
    """A static_step.StaticBatch (loader-built fusion table / masked positions / CSR, padded row counts, padded
    global-map width) gives the loss and the gradients of the same batch fed through the reference API
    (GlocalTextPathCMTPreTraining.forward(batch, task).mean()): padding rows carry exactly zero weight."""
    from vln_bevbert_amd import ops
    from vln_bevbert_amd.static_step import StaticBatch
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    model, arena = _fresh(cfg, dtype)
    model.set_dropout(0.0)
    for task in ("sap", "mlm", "masksem"):
        cpu = synthetic.make_batch(cfg, task, 3, seed=70, ragged=True, sems_as="ids")
        sb = StaticBatch(cfg, task, cpu, DEV)
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
        tol = 1e-5 if dtype == torch.float32 else 2e-2
        assert abs(la - ls) <= tol * max(1.0, abs(la)), (task, la, ls)
        rel = float((ga - gs_).norm() / ga.norm())
        assert rel < (1e-4 if dtype == torch.float32 else 5e-2), (task, rel)


def test_captured_step_replays_the_eager_step(env):
    """The hipGraph path against the eager path, same weights, same (seed, step) sequence, dropout ON: four passes over
    three static batches (two eager uses, the capture, one replay each).  The first step is compared bit for bit
    (identical parameters on both sides); later steps to 5e-4 -- the only run-to-run freedom of either path is the
    order of the fp32 atomics in the word-embedding / graph-bias gradients, which AdamW carries into the weights, where
    a last-bit difference can flip the bf16 rounding of a compute copy (observed: ten steps bit-identical, then 6e-5).
    Replays must also follow the learning-rate schedule and draw fresh dropout masks (device-resident lr / salt)."""
    from vln_bevbert_amd.static_step import StaticBatch
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    seq = ("sap", "mlm", "masksem") * 4
    curves, finals = {}, {}
    for graphs in (False, True):
        model, arena = _fresh(cfg, torch.bfloat16)
        tr = PretrainTrainer(model, arena, learning_rate=1e-4, warmup_steps=4, num_train_steps=40)
        tr.use_graphs = graphs
        sbs = {t: StaticBatch(cfg, t, synthetic.make_batch(cfg, t, 3, seed=60, ragged=True, sems_as="ids"), DEV)
               for t in ("sap", "mlm", "masksem")}
        out = [float(tr.step(t, sbs[t])) for t in seq]
        torch.cuda.synchronize()
        assert all((sb.graph is not None) == graphs for sb in sbs.values())
        curves[graphs], finals[graphs] = np.asarray(out), arena.params.clone()
    e, g = curves[False], curves[True]
    assert np.isfinite(g).all()
    assert e[0] == g[0], (e[0], g[0])
    assert np.max(np.abs(e - g) / np.maximum(1.0, np.abs(e))) < 5e-4, (e, g)
    # the same batch at different steps: different dropout masks and a moving learning rate -> different losses
    assert len({round(x, 6) for x in g[0::3]}) == 4, g[0::3]
    rel = float((finals[False] - finals[True]).norm() / finals[False].norm())
    assert rel < 1e-4, rel


def test_static_batch_refill_keeps_the_captured_graph(env):
    """load() writes the next batch of the same shape bucket into the buffers a graph was captured on; the replay then
    trains on the new batch (loss equals a fresh eager step on that batch from the same weights)."""
    from vln_bevbert_amd.static_step import StaticBatch
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    b1 = synthetic.make_batch(cfg, "sap", 3, seed=61, sems_as="ids")
    b2 = synthetic.make_batch(cfg, "sap", 3, seed=62, sems_as="ids")
    losses = {}
    for graphs in (False, True):
        model, arena = _fresh(cfg, torch.float32)
        model.set_dropout(0.0)
        tr = PretrainTrainer(model, arena, learning_rate=0.0, warmup_steps=1, num_train_steps=10)   # lr 1e-8: weights ~fixed
        tr.use_graphs = graphs
        sb = StaticBatch(cfg, "sap", b1, DEV)
        if sb.signature != StaticBatch(cfg, "sap", b2, "cpu").signature:
            pytest.skip("the two synthetic batches fell into different shape buckets")
        for _ in range(3):
            tr.step("sap", sb)
        assert (sb.graph is not None) == graphs
        sb.load(b2)
        losses[graphs] = float(tr.step("sap", sb))
    assert abs(losses[True] - losses[False]) <= 1e-5 * max(1.0, abs(losses[False])), losses


def test_static_batch_with_object_tokens_runs_eagerly_and_survives_a_refill(env):
    """REVERIE-style batches (traj_obj_img_fts): the forward uploads host-derived object-token indices, so such a
    StaticBatch is never captured (a graph would replay the indices of the batch it was captured on); a refill with a
    batch of different per-sample step / object counts in the same bucket gives that batch's loss."""
    from vln_bevbert_amd.static_step import StaticBatch
    from vln_bevbert_amd.train import PretrainTrainer
    cfg = BevBertConfig.tiny(image_feat_size=768, obj_feat_size=768, obj_prob_size=50, num_l_layers=1, num_x_layers=1,
                             vocab_size=400, pretrain_tasks=("mlm", "mrc", "sap", "og"))
    # two batches with the same per-sample step counts and text lengths (they are part of the bucket signature of an
    # object-token batch) but their own random content: different object counts per panorama at every position
    def mk(seed):
        rng = np.random.default_rng(seed)
        samples = [synthetic.make_sample(rng, i, cfg, T, L, ragged_views=True) for i, (T, L) in enumerate([(5, 70), (2, 48), (4, 76)])]
        return synthetic.collate(samples, cfg, "sap", rng)
    b1, other = mk(71), mk(75)          # 72 differs in the joint [views | objects] width: another bucket (signature)
    assert b1.get("traj_obj_img_fts") is not None
    assert not torch.equal(other["traj_vp_obj_lens"], b1["traj_vp_obj_lens"])
    model, arena = _fresh(cfg, torch.float32)
    model.set_dropout(0.0)
    tr = PretrainTrainer(model, arena, learning_rate=0.0, warmup_steps=1, num_train_steps=10)
    sb = StaticBatch(cfg, "sap", b1, DEV)
    assert not sb.capturable
    for _ in range(tr.GRAPH_WARMUP + 2):
        tr.step("sap", sb)
    assert sb.graph is None and tr.graph_error is None
    assert StaticBatch(cfg, "sap", other, "cpu").signature == sb.signature
    with pytest.raises(ValueError, match="shape bucket"):       # same step counts, other joint token width: refused
        sb.load(mk(72))
    sb.load(other)
    with torch.no_grad():                               # before the step: the step's optimiser moves the weights
        want = float(model(synthetic.batch_to(other, DEV), "sap").mean())
    got = float(tr.step("sap", sb))
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)


def _run_direct(cfg, order, host, lr, dtype=torch.float32, dropout=0.0):
    from vln_bevbert_amd.static_step import StaticBatch
    from vln_bevbert_amd.train import PretrainTrainer
    model, arena = _fresh(cfg, dtype)
    model.set_dropout(dropout)
    tr = PretrainTrainer(model, arena, learning_rate=lr, warmup_steps=1, num_train_steps=100)
    tr.use_graphs = False
    out = [float(tr.step(t, StaticBatch(cfg, t, b, DEV))) for t, b in zip(order, host)]
    torch.cuda.synchronize()
    return np.asarray(out), arena.params.clone()


def _run_stream(cfg, order, host, lr, depth=2, prefetch=1, dtype=torch.float32, dropout=0.0, graphs=True):
    from vln_bevbert_amd.loader import BucketManager, StreamingLoader
    from vln_bevbert_amd.train import PretrainTrainer
    model, arena = _fresh(cfg, dtype)
    model.set_dropout(dropout)
    tr = PretrainTrainer(model, arena, learning_rate=lr, warmup_steps=1, num_train_steps=100)
    tr.use_graphs = graphs
    mgr = BucketManager(cfg, DEV, depth=depth, max_buckets=8)
    loader = StreamingLoader(((t, b) for t, b in zip(order, host)), mgr, prefetch=prefetch)
    out = []
    for t, sb in loader:
        out.append(float(tr.step(t, sb)))
        loader.release(sb)
    torch.cuda.synchronize()
    return np.asarray(out), arena.params.clone(), mgr


def test_training_is_bit_reproducible_run_to_run(env):
    """The direct-vs-direct control VERDICT r3 asked for: two runs of the same 12 eager training steps (dropout ON, bf16
    compute copies, AdamW) from the same seed give the same losses and the same parameters BIT FOR BIT -- there is no
    atomic accumulation left on the path (word-embedding gradients: first-row leaders summing in row order; graph-bias
    gradients: per-head stores folded on the host; everything else was already a fixed-order reduction)."""
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    order = ["sap", "mlm", "masksem"] * 4
    host = [synthetic.make_batch(cfg, t, 3, seed=500 + i % 5, ragged=True, sems_as="ids") for i, t in enumerate(order)]
    for dtype in (torch.float32, torch.bfloat16):
        a, pa = _run_direct(cfg, order, host, 1e-4, dtype=dtype, dropout=0.1)
        b, pb = _run_direct(cfg, order, host, 1e-4, dtype=dtype, dropout=0.1)
        assert np.array_equal(a, b), (dtype, a, b)
        assert torch.equal(pa, pb), dtype


def test_streaming_loader_refills_double_buffered_batches_and_trains_like_direct_steps(env):
    """loader.StreamingLoader + BucketManager (producer thread, copy stream, two buffer sets per shape bucket, graphs
    captured per buffer set) against stepping on freshly built StaticBatches of the same host batches.
    (1) identical weights (learning rate 0, as test_static_batch_refill_keeps_the_captured_graph): every step's loss is
    a function of the batch in the buffers alone -> 1e-5; a stale or half-refilled buffer set shows here.
    (2) a real training curve (AdamW, lr 1e-4): the gate of test_captured_step_replays_the_eager_step (5e-4) -- eager
    and replayed steps run the same kernels; since round 4 they are free of atomics, so the observed difference is 0."""
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    order = ["sap", "mlm"] * 8
    host = [synthetic.make_batch(cfg, t, 3, seed=300 + i % 3, sems_as="ids") for i, t in enumerate(order)]
    d0, _ = _run_direct(cfg, order, host, 0.0)
    s0, _, mgr = _run_stream(cfg, order, host, 0.0)
    assert mgr.stats["refills"] > 0 and mgr.captured_graphs() > 0 and len(mgr.buckets) <= 6
    assert np.allclose(d0, s0, rtol=1e-5, atol=1e-6), (d0, s0)
    d1, pd = _run_direct(cfg, order, host, 1e-4)
    s1, ps, _ = _run_stream(cfg, order, host, 1e-4)
    dev = np.max(np.abs(d1 - s1) / np.maximum(1.0, np.abs(d1)))
    assert dev < 5e-4, (dev, d1, s1)
    assert float((pd - ps).norm() / pd.norm()) < 1e-4


@pytest.mark.parametrize("graphs", [False, True])
def test_streaming_loader_single_task_stream_reuses_one_bucket_safely(env, graphs):
    """consecutive batches of ONE task land in one shape bucket, so with two buffer sets and one queued
    batch the producer wants to refill the set of batch k while step k is still being enqueued.  The ownership flag of
    loader.BucketManager makes it wait: every step's loss (identical weights, lr 0) is its own batch's loss."""
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1, vocab_size=400)
    order = ["mlm"] * 12
    base = synthetic.make_batch(cfg, "mlm", 3, seed=410, sems_as="ids")
    host = []
    for i in range(len(order)):      # same shapes (one bucket), different tokens / labels -> different losses
        b = synthetic.make_batch(cfg, "mlm", 3, seed=410 + i, sems_as="ids")
        host.append(b)
    d0, _ = _run_direct(cfg, order, host, 0.0)
    s0, _, mgr = _run_stream(cfg, order, host, 0.0, graphs=graphs)
    assert len(set(np.round(d0, 5))) > 6, d0                      # the batches are distinguishable by their loss
    assert np.allclose(d0, s0, rtol=1e-5, atol=1e-6), (d0, s0)
    assert max(len(b["sets"]) for b in mgr.buckets.values()) == 2 and mgr.stats["refills"] >= 4


def test_loader_copy_stream_is_off_the_compute_streams_hardware_queue(env):
    """A process has four in-order hardware queues and its streams are dealt onto them: a refill enqueued on a copy stream
    that shares the compute stream's queue runs behind the whole step in flight, and the next step starts one copy time
    late (0.54 ms idle per step, r06w).  BucketManager probes a few fresh streams and keeps one whose work overtakes work
    queued earlier on the compute stream."""
    from vln_bevbert_amd.loader import BucketManager, shares_hw_queue
    dev = torch.device("cuda", torch.cuda.current_device())
    main = torch.cuda.current_stream(dev)
    assert shares_hw_queue(main, main, dev)                      # the probe sees serialisation when there is some
    mgr = BucketManager(BevBertConfig.tiny(), dev)
    probe = mgr.copy_stream_probe
    assert probe is not None and probe["picked"] is not None, probe
    assert probe["shares_compute_queue"][-1] is False and all(probe["shares_compute_queue"][:-1]), probe
    assert not shares_hw_queue(mgr.copy_stream, main, dev)       # and the answer is stable for the stream's lifetime


def test_gradient_exchange_runs_off_the_compute_streams_hardware_queue(one_rank_group):
    """The collective library issues on the next stream of torch's pool; one in four of those shares the compute stream's
    in-order hardware queue, and an all-reduce there waits behind the backward kernels enqueued before it and holds up the
    ones after it.  GradReducer.settle_collective_queue steers the pool before the group's first collective (or moves the
    exchange to a group of its own) and reports what it found; afterwards a collective overtakes work queued earlier on
    the compute stream."""
    from vln_bevbert_amd.hwqueues import steer_stream_pool, shares_hw_queue
    from vln_bevbert_amd.train import GradReducer
    dev = torch.device("cuda", torch.cuda.current_device())
    flat = torch.zeros(1 << 16, device=dev)
    red = GradReducer(flat, 1 << 15, force=True)
    rep = red.settle_collective_queue()
    final = rep.get("own_group") or rep
    assert final["waits_behind_compute"] is False, rep
    assert red.collectives_wait_behind_compute() is False
    assert not shares_hw_queue(red.stream, torch.cuda.current_stream(dev), dev)
    # a second reducer of the process reuses the outcome
    red2 = GradReducer(flat, 1 << 15, force=True)
    assert red2.settle_collective_queue() is rep and red2.group is red.group
    # the pool walk itself: 32 streams, cyclic, one in four on the compute stream's queue
    st = steer_stream_pool(dev)
    assert st["pool"] == 32 and 20 <= sum(st["wanted"]) <= 28 and st["next"] is not None, st
    nxt = torch.cuda.Stream(dev)
    assert not shares_hw_queue(nxt, torch.cuda.current_stream(dev), dev)


def test_gradient_exchange_moves_to_a_group_of_its_own_when_the_default_group_waits_behind_compute(one_rank_group, monkeypatch):
    """The other branch of GradReducer.settle_collective_queue: the default group's communicator was bound to a stream on
    the compute stream's queue before the trainer came (here: the first check is made to say so) -> the pool is steered, the
    exchange moves to a new_group(), the new group is checked for real, and regions reduce through it."""
    from vln_bevbert_amd.train import GradReducer
    dev = torch.device("cuda", torch.cuda.current_device())
    monkeypatch.setattr(GradReducer, "_settled", {})
    real = GradReducer.collectives_wait_behind_compute
    calls = []

    def first_says_yes(self, *a, **k):
        calls.append(1)
        return True if len(calls) == 1 else real(self, *a, **k)
    monkeypatch.setattr(GradReducer, "collectives_wait_behind_compute", first_says_yes)
    flat = torch.arange(1 << 16, device=dev, dtype=torch.float32)
    red = GradReducer(flat, 1 << 15, force=True)
    assert red.group is None
    rep = red.settle_collective_queue()
    assert rep["waits_behind_compute"] is True and rep["own_group"]["waits_behind_compute"] is False, rep
    assert red.group is not None and len(calls) == 2
    want = flat.clone()
    red.launch_region(1 << 15, 1 << 16)
    red.finish()
    torch.cuda.synchronize()
    assert torch.equal(flat, want)                 # one rank: the sum over ranks is the tensor itself


# ----------------------------------------------------------------------------- capture.py: one capture-and-recover path
# (a Python exception raised while a capture is open, as in the failed-capture test above: nothing here faults the device)
def test_capture_records_without_running_and_graphs_of_one_pool_replay_in_turn(env):
    from vln_bevbert_amd import capture
    x, y = torch.arange(8.0, device=DEV), torch.zeros(8, device=DEV)
    g1, res = capture.capture(lambda: y.copy_(x * 2))
    torch.cuda.synchronize()
    assert res is y and not bool(y.any())                        # recorded, not run: the caller replays
    x.add_(1)
    g1.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.arange(1.0, 9.0, device=DEV) * 2)
    x2, y2 = torch.full((8,), 5.0, device=DEV), torch.zeros(8, device=DEV)
    g2, _ = capture.capture(lambda: y2.copy_(x2 * 2), pool=g1.pool())
    assert g2.pool() == g1.pool()
    x.fill_(3)
    g1.replay()
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((8,), 6.0, device=DEV)) and torch.equal(y2, torch.full((8,), 10.0, device=DEV))


def test_a_failed_capture_with_an_open_fork_is_ended_and_leaves_nothing_behind(env):
    """The body forks a side stream that only ``extra_streams`` names, queues deferred work the way a backward pass does, and
    raises with the fork still open: ``capture`` joins it, ends the capture, drops the queued work and reports."""
    from vln_bevbert_amd import capture, lib, ops
    from vln_bevbert_amd.hwqueues import side_stream
    side = side_stream(DEV)
    x, z, ran = torch.arange(8.0, device=DEV), torch.zeros(8, device=DEV), []
    sentinel, record, made = (lambda: ran.append(1)), (0, 1, 1, 8, 0, 0, 0, 1), []

    def body():
        assert torch.cuda.is_current_stream_capturing()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            z.add_(1)
        h = lib.stream()
        if h not in ops.WgradStream._pending:
            made.append(h)
            ops.WgradStream._pending[h] = (torch.cuda.current_stream(), [])
        ops.WgradStream._pending[h][1].append(sentinel)
        ops.ReduceQueue.jobs.append(record)
        raise RuntimeError("injected")

    try:
        with pytest.raises(capture.CaptureFailed) as info:
            capture.capture(body, extra_streams=[side])
        assert "injected" in info.value.message and len(info.value.message) <= 400
        assert isinstance(info.value.__cause__, RuntimeError) and "injected" in str(info.value.__cause__)
        assert not torch.cuda.is_current_stream_capturing()
        assert ops.ReduceQueue.jobs == [] and ops.ReduceQueue.accum_jobs == []
        assert not any(fns for _, fns in ops.WgradStream._pending.values())
        ops.WgradStream.flush_all()                              # what the next backward pass does with deferred work
        assert ran == []
        y = x + 1
        torch.cuda.synchronize()
        assert torch.equal(y, torch.arange(1.0, 9.0, device=DEV)) and not bool(z.any())
        g, _ = capture.capture(lambda: z.copy_(x * 2))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(z, x * 2)
    finally:                                                     # whatever failed above, the next test starts clean
        ops.ReduceQueue.jobs = [j for j in ops.ReduceQueue.jobs if j is not record]
        for _, fns in ops.WgradStream._pending.values():
            fns[:] = [f for f in fns if f is not sentinel]
        for h in made:
            ops.WgradStream._pending.pop(h, None)


def test_nav_graph_runner_goes_on_eagerly_after_a_failed_capture(env):
    from types import SimpleNamespace
    from vln_bevbert_amd.nav_static import NavGraphRunner
    runner = NavGraphRunner(SimpleNamespace(training=False, vln_bert=None), eager_uses=1)

    def fn(x):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("injected " + "x" * 600)
        return {"o": x["a"] * 3}

    for i in range(3):                                           # eager, capture (fails, eager), eager
        a = torch.full((2, 8), float(i + 1), device=DEV)
        out = runner._run(("k", 2, 8), {"a": a}, fn)
        torch.cuda.synchronize()
        assert torch.equal(out["o"], a * 3), i
        assert not torch.cuda.is_current_stream_capturing()
        assert runner.stats == {"replays": 0, "eager": i + 1, "captures": 0}
        assert (runner.graph_error is None) == (i == 0)
    assert "injected" in runner.graph_error and len(runner.graph_error) <= 400
    assert runner.captured_graphs() == 0 and len(runner.buckets) == 1


def test_nav_train_runner_drops_every_graph_after_a_failed_capture_and_trains_on_eagerly(env):
    """Two segments per episode, o1 = a * w and o2 = o1 * w, one backward through both.  With graphs the second episode is
    the capture episode: segment 1's forward is captured, segment 2's raises.  That episode trains nothing (as a capture
    episode never does) and keeps no graph -- a backward graph of segment 1 alone would later replay against a forward
    that no longer exists -- and the episodes before and after it leave exactly the gradients of a runner without graphs."""
    from types import SimpleNamespace
    from vln_bevbert_amd.nav_static import NavTrainRunner
    grads = {}
    for graphs in (False, True):
        w = torch.linspace(0.5, 2.0, 16, device=DEV).view(2, 8).requires_grad_(True)
        runner = NavTrainRunner(SimpleNamespace(training=True, vln_bert=None), SimpleNamespace(sync=lambda: None),
                                eager_uses=1, graphs=graphs)

        def fn1(x):
            return {"o": x["a"] * w}

        def fn2(x):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("injected")
            return {"o": x["a"] * w}

        for ep in range(3):
            a = (torch.arange(16.0, device=DEV).view(2, 8) + ep).requires_grad_(True)
            w.grad = None
            runner.begin_episode()
            capture_episode = runner.capturing
            assert capture_episode == (graphs and ep == 1)
            o1 = runner._segment("navigation", (2, 8), {"a": a}, ("a",), fn1, {}, ("o",))["o"]
            o2 = runner._segment("navigation", (2, 8), {"a": o1}, ("a",), fn2, {}, ("o",))["o"]
            torch.cuda.synchronize()
            assert torch.equal(o2, a.detach() * w.detach() * w.detach())
            if capture_episode:
                runner.end_capture()
                assert w.grad is None and a.grad is None
                assert "injected" in runner.graph_error and "injected" in runner.graph_traceback
                assert "fn2" in runner.graph_traceback
            else:
                (o2 * o2).sum().backward()
                torch.cuda.synchronize()
                grads[(graphs, ep)] = (w.grad.clone(), a.grad.clone())
            assert not runner.capturing and not torch.cuda.is_current_stream_capturing()
            assert len(runner.segs) == 2 and all(s.fwd is None and s.bwd is None for s in runner.segs.values())
        assert runner.captured_graphs() == 0
        assert runner.stats["captures"] == (1 if graphs else 0) and runner.stats["replays"] == 0
    for ep in (0, 2):
        for got, want in zip(grads[(True, ep)], grads[(False, ep)]):
            assert float(want.abs().sum()) > 0 and torch.equal(got, want), ep
