"""Store-mode split-K folds that carry the clip norm: the STORE and NORM task flags of bevbert_multi_accum,
bevbert_sumsq_tasks, bevbert_clip_from_slots, and the trainer step that uses them (ops.ReduceQueue, ParamArena).

The folds only add, so STORE is compared for EQUALITY: with the accumulate path on a zeroed sink and with the numpy float32
sum ((0 + p0) + p1) + ... .  A NORM slot is a float32 sum of squares -- a 64-term chain per thread (16 float4 groups of 4
squares) plus an 8-level tree over 256 threads and 2 roundings per square-and-add -- so about 74 * 2^-24 = 4.4e-6 relative to
the fp64 sum of the same stored values; the gate is 1e-5.  bevbert_clip_from_slots sums in fp64 and rounds sqrt, the
product with pre_scale, the sum with 1e-6 and the quotient to float32: a few 2^-24, gate 1e-6.
"""
import numpy as np
import pytest
import torch

from vln_bevbert_amd import synthetic
from vln_bevbert_amd.config import BevBertConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32_CODE, BF16_CODE = 0, 1
STORE, NORM = 0x100, 0x200
ACCUM_TASK = np.dtype([("partials", "<u8"), ("sink", "<u8"), ("n4_total", "<u8"), ("off4", "<u4"), ("n4", "<u4"),
                       ("S", "<i4"), ("dtype", "<i4")])
SUMSQ_TASK = np.dtype([("ptr", "<u8"), ("n4", "<u4"), ("slot", "<u4")])
GUARD = 8           # floats left alone before and after every sink range
SENTINEL = -7.0     # slots nobody may write keep this value


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


@pytest.fixture
def slots(ops):
    """A registered slot array of 64 floats (prefilled with SENTINEL), unregistered again afterwards."""
    from vln_bevbert_amd import lib
    s = torch.full((64,), SENTINEL, device=DEV)
    lib.load().bevbert_set_fold_norm_slots(s.data_ptr(), 64)
    yield s
    torch.cuda.synchronize()
    lib.load().bevbert_set_fold_norm_slots(None, 0)


def _call(name, *args):
    from vln_bevbert_amd import lib
    lib.call(name, *args, lib.stream())
    torch.cuda.synchronize()


def _table(records, dtype):
    host = np.array(records, dtype=dtype)
    return torch.from_numpy(host.view(np.uint8).copy()).to(DEV)


def _rnd(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _records(part, sink, n4, S, code, flags, slot0=0):
    """Tasks of at most 4 096 float4 groups over one weight of n4 groups whose sink range starts GUARD floats in."""
    recs = []
    for k, off in enumerate(range(0, n4, 4096)):
        word = code | flags | (((slot0 + k) << 12) if flags & NORM else 0)
        recs.append((part.data_ptr(), sink.data_ptr() + (GUARD + off * 4) * 4, n4, off, min(4096, n4 - off), S,
                     int(np.uint32(word).view(np.int32))))
    return recs


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("dt", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n4", [1, 5, 4096, 4097])
@pytest.mark.parametrize("S", [1, 3, 4, 5, 9])
def test_store_equals_accumulate_into_zeros(ops, S, n4, dt):
    """STORE over a sink full of NaNs == the accumulate path on a zeroed sink == the float32 sum in the documented order,
    bit for bit; both sides of the four-slice batch, one task and two, a clamped tail; the guard floats stay."""
    part = _rnd(100 * S + n4 % 97, S, n4 * 4).to(dt).contiguous()
    code = BF16_CODE if dt == BF16 else F32_CODE
    nan_sink = torch.full((n4 * 4 + 2 * GUARD,), float("nan"), device=DEV)
    nan_sink[:GUARD] = 3.0
    nan_sink[-GUARD:] = 5.0
    zero_sink = torch.zeros_like(nan_sink)
    _call("bevbert_multi_accum", _table(_records(part, nan_sink, n4, S, code, STORE), ACCUM_TASK).data_ptr(), (n4 + 4095) // 4096)
    _call("bevbert_multi_accum", _table(_records(part, zero_sink, n4, S, code, 0), ACCUM_TASK).data_ptr(), (n4 + 4095) // 4096)
    got, ref = nan_sink[GUARD:-GUARD], zero_sink[GUARD:-GUARD]
    assert torch.equal(_bits(got), _bits(ref)), f"{int((_bits(got) != _bits(ref)).sum())} of {n4 * 4} floats differ"
    want = np.zeros(n4 * 4, np.float32)
    for p in part.float().cpu().numpy():
        want = (want + p).astype(np.float32)
    assert np.array_equal(got.cpu().numpy(), want)
    assert nan_sink[:GUARD].tolist() == [3.0] * GUARD and nan_sink[-GUARD:].tolist() == [5.0] * GUARD


@pytest.mark.parametrize("dt", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n4,S", [(1, 1), (5, 3), (4096, 4), (4097, 5), (3 * 4096 + 77, 9)])
@pytest.mark.parametrize("flags", [STORE | NORM, NORM], ids=["store", "accumulate"])
def test_norm_slot_is_the_sum_of_squares_of_what_was_stored(ops, slots, flags, n4, S, dt):
    """Every NORM task leaves the sum of squares of ITS stored values (clamped duplicates not counted) in its slot; the
    other slots keep their contents."""
    part = _rnd(7 + n4 % 89 + S, S, n4 * 4).to(dt).contiguous()
    sink = _rnd(11, n4 * 4 + 2 * GUARD)
    code = BF16_CODE if dt == BF16 else F32_CODE
    ntasks = (n4 + 4095) // 4096
    _call("bevbert_multi_accum", _table(_records(part, sink, n4, S, code, flags, slot0=3), ACCUM_TASK).data_ptr(), ntasks)
    stored = sink[GUARD:-GUARD].double()
    got = slots.cpu().numpy()
    for k in range(ntasks):
        want = float(stored[k * 16384:(k + 1) * 16384].pow(2).sum())
        assert abs(float(got[3 + k]) - want) <= 1e-5 * want, (k, float(got[3 + k]), want)
    untouched = np.delete(got, np.arange(3, 3 + ntasks))
    assert (untouched == SENTINEL).all()


def test_tasks_without_norm_and_slots_out_of_range_write_no_slot(ops, slots):
    """Three weights in one launch: NORM into slot 0, no flag (its slot bits are zero: slot 0 must not be hit twice), NORM
    with a slot beyond the registered capacity.  Only slot 0 is written, with the first weight's sum."""
    from vln_bevbert_amd import lib
    lib.load().bevbert_set_fold_norm_slots(slots.data_ptr(), 4)        # capacity 4 of the 64 floats
    n4, S = 300, 2
    parts = [_rnd(20 + i, S, n4 * 4) for i in range(3)]
    sinks = [torch.zeros(n4 * 4 + 2 * GUARD, device=DEV) for _ in range(3)]
    recs = (_records(parts[0], sinks[0], n4, S, F32_CODE, STORE | NORM, slot0=0)
            + _records(parts[1], sinks[1], n4, S, F32_CODE, 0)
            + _records(parts[2], sinks[2], n4, S, F32_CODE, STORE | NORM, slot0=9))
    _call("bevbert_multi_accum", _table(recs, ACCUM_TASK).data_ptr(), 3)
    want = float(sinks[0].double().pow(2).sum())
    got = slots.cpu().numpy()
    assert abs(float(got[0]) - want) <= 1e-5 * want
    assert (got[1:] == SENTINEL).all()
    for p, s in zip(parts, sinks):                                      # all three folds happened
        assert torch.equal(s[GUARD:-GUARD], (p[0] + p[1]))


def test_without_a_registered_array_norm_is_ignored_and_sumsq_tasks_refuses(ops):
    from vln_bevbert_amd import lib
    lib.load().bevbert_set_fold_norm_slots(None, 0)
    part, sink = _rnd(1, 1, 64), torch.zeros(64 + 2 * GUARD, device=DEV)
    _call("bevbert_multi_accum", _table(_records(part, sink, 16, 1, F32_CODE, STORE | NORM), ACCUM_TASK).data_ptr(), 1)
    assert torch.equal(sink[GUARD:-GUARD], part[0])
    t = _table([(sink.data_ptr(), 4, 0)], SUMSQ_TASK)
    with pytest.raises(lib.BevBertHipError, match="slot array"):
        _call("bevbert_sumsq_tasks", t.data_ptr(), 1)


def test_a_weight_folded_in_two_rounds_stores_first_and_takes_its_norm_from_the_second(ops):
    """ReduceQueue.flush with a store context: a sink hit twice gets STORE in round 0 only and NORM in round 1 only; a sink
    hit once gets both; a sink the predicate refuses gets neither.  The record it leaves sums to the norm of the result."""
    Q = ops.ReduceQueue
    n = 4 * 5000                                        # two tasks per weight
    twice, once, refused = (torch.full((n,), float("nan"), device=DEV) for _ in range(3))
    refused.fill_(1.0)
    pa, pb, pc, pd = (_rnd(30 + i, 2, n).to(BF16) for i in range(4))
    saved = Q.accum_jobs, Q.store_ok, Q.fold_norm
    try:
        Q.accum_jobs = []
        Q.add_accum(pa.data_ptr(), twice.data_ptr(), 2, n, BF16_CODE)
        Q.add_accum(pb.data_ptr(), once.data_ptr(), 2, n, BF16_CODE)
        Q.add_accum(pc.data_ptr(), twice.data_ptr(), 2, n, BF16_CODE)
        Q.add_accum(pd.data_ptr(), refused.data_ptr(), 2, n, BF16_CODE)
        rounds, flags = Q._plan_fold(tuple(Q.accum_jobs), lambda p, k: p != refused.data_ptr())
        assert [len(r) for r in rounds] == [3, 1]
        assert flags == [[STORE, STORE | NORM, 0], [NORM]]
        Q.store_ok = lambda p, k: p != refused.data_ptr()
        Q.flush(torch.device(DEV))
        torch.cuda.synchronize()
        rec = Q.fold_norm
        assert Q.store_ok is None and rec is not None and rec["entry"]["nslots"] == 4
        f = lambda p: p.float()
        assert torch.equal(twice, ((f(pa[0]) + f(pa[1])) + f(pc[0])) + f(pc[1]))
        assert torch.equal(once, f(pb[0]) + f(pb[1]))
        assert torch.equal(refused, (1.0 + f(pd[0])) + f(pd[1]))
        want = float(twice.double().pow(2).sum() + once.double().pow(2).sum())
        got = float(Q.slots(DEV)[:4].double().sum())
        assert abs(got - want) <= 1e-5 * want
        assert Q.table_bytes[rec["entry"]["tables"][0][0].data_ptr()] == 2 * (2 * n * 2 + 4 * n) + (2 * n * 2 + 8 * n)
        # a second accumulate-flush of the same step: no context left, plain tables, the record is void
        Q.add_accum(pa.data_ptr(), once.data_ptr(), 2, n, BF16_CODE)
        before = once.clone()
        Q.flush(torch.device(DEV))
        torch.cuda.synchronize()
        assert Q.fold_norm is None
        assert torch.equal(once, (before + f(pa[0])) + f(pa[1]))
    finally:
        Q.accum_jobs, Q.store_ok, Q.fold_norm = saved
        Q._accum_tables.clear()
        from vln_bevbert_amd import lib
        lib.load().bevbert_set_fold_norm_slots(None, 0)


def test_sumsq_tasks_against_float64(ops, slots):
    """One workgroup per record: below one group per thread, exactly one, a remainder, the full 4 096 groups."""
    sizes = [1, 255, 256, 257, 1000, 4096]
    g = _rnd(5, 4 * sum(sizes))
    recs, pos = [], 0
    for k, n4 in enumerate(sizes):
        recs.append((g.data_ptr() + 16 * pos, n4, 2 * k + 1))
        pos += n4
    _call("bevbert_sumsq_tasks", _table(recs, SUMSQ_TASK).data_ptr(), len(recs))
    got, pos = slots.cpu().numpy(), 0
    for k, n4 in enumerate(sizes):
        want = float(g[4 * pos:4 * (pos + n4)].double().pow(2).sum())
        assert abs(float(got[2 * k + 1]) - want) <= 1e-5 * want, (n4, float(got[2 * k + 1]), want)
        pos += n4
    assert (got[0::2] == SENTINEL).all() and (got[2 * len(sizes) + 1:] == SENTINEL).all()


@pytest.mark.parametrize("case", ["clips", "does_not_clip", "no_max_norm", "all_zero", "one_slot", "many_slots"])
def test_clip_from_slots_against_float64(ops, case):
    n = {"one_slot": 1, "many_slots": 20000}.get(case, 700)             # past 256: several slots per thread
    s = _rnd(9, n).abs() * (0.0 if case == "all_zero" else 1.0) + (0.0 if case == "all_zero" else 1e-3)
    pre = {"clips": 0.5, "does_not_clip": 0.125, "no_max_norm": 0.5}.get(case, 1.0)
    max_norm = {"clips": 1.0, "does_not_clip": 1e4, "no_max_norm": -1.0}.get(case, 5.0)
    scal = torch.full((2,), SENTINEL, device=DEV)
    _call("bevbert_clip_from_slots", s.data_ptr(), n, pre, max_norm, scal.data_ptr())
    norm = float(s.double().sum().sqrt()) * pre
    mult = pre * (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)
    got_norm, got_mult = scal.tolist()
    assert abs(got_norm - norm) <= 1e-6 * norm, (got_norm, norm)
    assert abs(got_mult - mult) <= 1e-6 * mult, (got_mult, mult)
    if case == "clips":
        assert mult < pre
    if case == "all_zero":
        assert got_norm == 0.0 and got_mult == pre


# ----------------------------------------------------------------------------- the trainer step
def _trainer(monkeypatch, fold_store):
    from vln_bevbert_amd import weights
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    from vln_bevbert_amd.train import PretrainTrainer
    monkeypatch.setenv("BEVBERT_FOLD_STORE", "1" if fold_store else "0")
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1)
    model = GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    arena = model.finalize(DEV, torch.bfloat16)
    model.train()
    model.set_dropout(0.1)
    trainer = PretrainTrainer(model, arena, learning_rate=1e-3, warmup_steps=1, num_train_steps=100)
    assert arena.fold_store == fold_store
    return cfg, model, arena, trainer


def _launches(monkeypatch, ops):
    """Names of the C-ABI launches issued from here on (eager steps and captures; a replay issues none)."""
    from vln_bevbert_amd import ops_core
    names, real = [], ops_core._raw_call
    monkeypatch.setattr(ops_core, "_raw_call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


def test_trainer_step_same_gradients_with_and_without_store_mode(ops, monkeypatch):
    """Tiny model, batch 2, bf16, static batch: two eager warm-up steps, the capture and two replays.  The parameters are
    put back after every step, so every step of the two trainers starts from the same ones (the moments go on).  Store
    mode on against off: arena.grads bit for bit after every step, the norm to 1e-5, the clip multiplier to 2e-5 and the
    AdamW displacement to 2e-4 (the gates of tests/test_gpu_optimizer_arena.py)."""
    from vln_bevbert_amd.static_step import StaticBatch
    names = _launches(monkeypatch, ops)
    runs = {}
    for fold_store in (False, True):
        cfg, model, arena, trainer = _trainer(monkeypatch, fold_store)
        sb = StaticBatch(cfg, "sap", synthetic.make_batch(cfg, "sap", 2, seed=5, ragged=True, sems_as="ids"), DEV)
        del names[:]
        steps = []
        before, shadow = arena.params.clone(), arena.shadow.clone()
        for k in range(trainer.GRAPH_WARMUP + 3):
            trainer.step("sap", sb)
            torch.cuda.synchronize()
            steps.append((arena.grads.clone(), arena._scalars[:2].tolist(), arena.params - before))
            arena.params.copy_(before)
            arena.shadow.copy_(shadow)
        assert sb.graph is not None, trainer.graph_error
        fused = names.count("bevbert_clip_from_slots")
        assert fused == (trainer.GRAPH_WARMUP + 1 if fold_store else 0), names
        assert names.count("bevbert_grad_norm_clip") == (0 if fold_store else trainer.GRAPH_WARMUP + 1)
        assert names.count("bevbert_sumsq_tasks") == fused and "bevbert_multi_accum" in names
        runs[fold_store] = steps
        if fold_store:
            stores = [e for e in ops.ReduceQueue._accum_tables.values() if e["stores"]]
            assert stores and all(e["nslots"] > 0 for e in stores)
    for k, ((g0, (n0, m0), d0), (g1, (n1, m1), d1)) in enumerate(zip(runs[False], runs[True])):
        assert float(g0.abs().max()) > 0
        assert torch.equal(_bits(g0), _bits(g1)), (k, int((_bits(g0) != _bits(g1)).sum()))
        assert abs(n1 - n0) <= 1e-5 * n0 and abs(m1 - m0) <= 2e-5 * m0, (k, n0, n1, m0, m1)
        assert float(d0.norm()) > 0 and float((d1 - d0).norm()) <= 2e-4 * float(d0.norm()), (k, float((d1 - d0).norm()), float(d0.norm()))


def test_eager_step_warns_about_a_sink_that_is_not_zero_before_the_fold(ops, monkeypatch):
    """Self-check (a): something wrote an eligible weight's gradient between the arena fill and the fold."""
    from vln_bevbert_amd import lib
    cfg, model, arena, trainer = _trainer(monkeypatch, True)
    batch = synthetic.batch_to(synthetic.make_batch(cfg, "sap", 2, seed=5, ragged=True), DEV)
    name = "global_sap_head.net.0.weight"
    real = arena.wait_zero
    monkeypatch.setattr(arena, "wait_zero", lambda: (real(), model.get_parameter(name).main_grad.view(-1)[3].fill_(1.0)))
    ops.ReduceQueue._accum_tables.clear()
    try:
        with pytest.raises(lib.BevBertHipError, match=name.replace(".", r"\.")):
            trainer.step("sap", batch)
    finally:
        torch.cuda.synchronize()
        ops.WgradStream.drop_pending()
        ops.ReduceQueue.drop_pending()
        ops.ReduceQueue._accum_tables.clear()
        ops.ReduceQueue.store_ok = ops.ReduceQueue.fold_norm = None


def test_eager_step_warns_about_a_gradient_that_changed_after_the_fold(ops, monkeypatch):
    """Self-check (b): something wrote an eligible weight's gradient between the fold and the optimiser."""
    from vln_bevbert_amd import lib
    cfg, model, arena, trainer = _trainer(monkeypatch, True)
    batch = synthetic.batch_to(synthetic.make_batch(cfg, "sap", 2, seed=5, ragged=True), DEV)
    name = "global_sap_head.net.0.weight"
    real = trainer.reducer.finish
    monkeypatch.setattr(trainer.reducer, "finish", lambda: (real(), model.get_parameter(name).main_grad.mul_(3.0)))
    ops.ReduceQueue._accum_tables.clear()
    try:
        with pytest.raises(lib.BevBertHipError, match=name.replace(".", r"\.")):
            trainer.step("sap", batch)
    finally:
        torch.cuda.synchronize()
        ops.ReduceQueue._accum_tables.clear()
        ops.ReduceQueue.store_ok = ops.ReduceQueue.fold_norm = None
