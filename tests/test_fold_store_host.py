"""Host side of the store-mode folds (ops.ReduceQueue, ParamArena, train.fold_store_allowed): which sinks may store, which
tasks carry which flag, when the fused norm is used -- on CPU tensors, with the C-ABI launches recorded instead of run."""
import numpy as np
import pytest
import torch

from vln_bevbert_amd import arena as arena_mod
from vln_bevbert_amd import lib, ops, ops_core, ops_reduce
from vln_bevbert_amd.config import BevBertConfig
from vln_bevbert_amd.train import fold_store_allowed

STORE, NORM = ops.ReduceQueue.STORE, ops.ReduceQueue.NORM
ACCUM_TASK = np.dtype([("partials", "<u8"), ("sink", "<u8"), ("n4_total", "<u8"), ("off4", "<u4"), ("n4", "<u4"),
                       ("S", "<i4"), ("dtype", "<i4")])


@pytest.fixture
def calls(monkeypatch):
    """[(name, args)] of the launches issued from here on; nothing runs, nothing needs a device."""
    out = []
    monkeypatch.setattr(ops_core, "_raw_call", lambda name, *a: out.append((name, a)))
    for mod in (lib, ops_reduce, arena_mod):
        monkeypatch.setattr(mod, "stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(arena_mod, "ptr", lambda t: None if t is None else t.data_ptr())
    slots = torch.zeros(ops.ReduceQueue.SLOT_CAPACITY)
    monkeypatch.setattr(ops.ReduceQueue, "register_slots", classmethod(lambda cls, device: slots))
    monkeypatch.setattr(ops.ReduceQueue, "_note_producer", classmethod(lambda cls: None))
    monkeypatch.setattr(ops.ReduceQueue, "FOLD_STORE", True)
    for name in ("accum_jobs", "jobs"):
        monkeypatch.setattr(ops.ReduceQueue, name, [])
    for name in ("_accum_tables", "_tables", "table_bytes"):
        monkeypatch.setattr(ops.ReduceQueue, name, {})
    monkeypatch.setattr(ops.ReduceQueue, "store_ok", None)
    monkeypatch.setattr(ops.ReduceQueue, "fold_norm", None)
    return out


@pytest.fixture(scope="module")
def model_arena():
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    torch.manual_seed(0)
    model = GlocalTextPathCMTPreTraining(BevBertConfig.tiny(num_l_layers=1, num_x_layers=1))
    model.tie_weights()
    return model, model.finalize("cpu", torch.float32)


def _sink(model, name):
    g = model.get_parameter(name).main_grad
    return g.data_ptr(), g.numel()


def _flags_of(entry):
    """per launch, the (STORE, NORM, slot) triples of its task records"""
    out = []
    for table, n in entry["tables"]:
        words = table.numpy().view(ACCUM_TASK)["dtype"].view(np.uint32)
        assert len(words) == n
        out.append([(bool(w & STORE), bool(w & NORM), int(w >> 12)) for w in words])
    return out


def test_only_fold_written_weights_may_store(model_arena):
    model, arena = model_arena
    word = model.bert.embeddings.word_embeddings.weight
    assert model.mlm_head.predictions.decoder.weight is word            # tied: one parameter, one sink
    assert not arena.store_ok(word.main_grad.data_ptr(), word.numel())
    assert not arena.store_ok(word.main_grad.data_ptr() + 4 * word.shape[1], word.shape[1])       # nor a row of it
    names = dict(model.named_parameters())
    tables = {id(m.weight) for m in model.modules() if isinstance(m, torch.nn.Embedding)}
    assert len(tables) >= 3
    n_ok = 0
    for n, p in names.items():
        ok = arena.store_ok(p.main_grad.data_ptr(), p.numel())
        assert ok == (p.dim() >= 2 and id(p) not in tables), n
        n_ok += ok
    assert n_ok >= 10
    p, k = _sink(model, "global_sap_head.net.0.weight")
    assert arena.store_ok(p, k) and arena.store_ok(p + 16, k - 4)
    assert not arena.store_ok(p, k + 4)                 # runs into the padding / the next tensor
    assert not arena.store_ok(p - 16, k)
    assert not arena.store_ok(p + 2, 4)                 # not an element address
    assert not arena.store_ok(arena.params.data_ptr(), 4)               # another buffer
    # a packed group (q | k | v side by side) is one range: the fold of the packed operand may store
    qkv = [n for n in names if n.endswith("attention.self.query.weight")][0]
    kk, vv = qkv.replace("query", "key"), qkv.replace("query", "value")
    if arena.slices[kk][0] == sum(arena.slices[qkv]) and arena.slices[vv][0] == sum(arena.slices[kk]):
        assert arena.store_ok(_sink(model, qkv)[0], 3 * names[qkv].numel())


def test_first_flush_after_zero_grad_stores_and_the_second_does_not(model_arena, calls):
    model, arena = model_arena
    Q = ops.ReduceQueue
    lin, word = _sink(model, "global_sap_head.net.0.weight"), _sink(model, "bert.embeddings.word_embeddings.weight")
    arena.fold_store = True
    try:
        arena._arm_fold()
        assert Q.store_ok == arena.store_ok
        Q.add_accum(1 << 20, lin[0], 2, lin[1], lib.BF16)
        Q.add_accum(2 << 20, word[0], 2, word[1], lib.BF16)
        Q.add_accum(3 << 20, lin[0], 1, lin[1], lib.F32)               # the same weight again: a second round
        checked = []
        arena.fold_check_zero = lambda stores: checked.append(list(stores))
        try:
            Q.flush(torch.device("cpu"))
        finally:
            del arena.fold_check_zero
        assert [c[0] for c in calls] == ["bevbert_multi_accum", "bevbert_multi_accum"]
        assert checked == [[lin]]                              # self-check (a) saw the one sink that stores
        rec = Q.fold_norm
        assert Q.store_ok is None and rec["owner"] is arena
        ntl, ntw = (lin[1] // 4 + 4095) // 4096, (word[1] // 4 + 4095) // 4096
        first, second = _flags_of(rec["entry"])
        assert first == [(True, False, 0)] * ntl + [(False, False, 0)] * ntw          # STORE in round 0; the table: neither
        assert second == [(False, True, k) for k in range(ntl)]                        # NORM from the last round
        assert rec["entry"]["nslots"] == ntl and rec["entry"]["norm_jobs"] == [(lin[0], lin[1], 0)]
        assert Q.table_bytes[rec["entry"]["tables"][0][0].data_ptr()] == (2 * lin[1] * 2 + 4 * lin[1]) + (2 * word[1] * 2 + 8 * word[1])
        # the complement: everything but that weight, in records of at most 4 096 groups, slots following the fold's
        table, ntasks, nbytes = arena._fold_complement(rec["entry"])
        t = table.numpy().view(np.dtype([("ptr", "<u8"), ("n4", "<u4"), ("slot", "<u4")]))
        assert nbytes == 4 * (arena.numel - lin[1]) and int(t["n4"].max()) <= 4096 and int(t["n4"].min()) >= 1
        assert t["slot"].tolist() == list(range(ntl, ntl + ntasks))
        covered = np.zeros(arena.numel, bool)
        for p, n4 in zip(t["ptr"].tolist(), t["n4"].tolist()):
            o = (p - arena.grads.data_ptr()) // 4
            assert not covered[o:o + 4 * n4].any()
            covered[o:o + 4 * n4] = True
        o = (lin[0] - arena.grads.data_ptr()) // 4
        assert not covered[o:o + lin[1]].any() and covered.sum() == arena.numel - lin[1]
        # a second accumulate-flush in the same step: plain records, and the fused norm is off for this step
        del calls[:]
        Q.add_accum(1 << 20, lin[0], 2, lin[1], lib.BF16)
        Q.flush(torch.device("cpu"))
        assert Q.fold_norm is None and [c[0] for c in calls] == ["bevbert_multi_accum"]
        plain = [e for k, e in Q._accum_tables.items() if k[1] is None]
        assert len(plain) == 1 and _flags_of(plain[0]) == [[(False, False, 0)] * ntl]
        del calls[:]
        arena.clip_and_step(1e-4, fused_norm=True)
        assert [c[0] for c in calls] == ["bevbert_grad_norm_clip", "bevbert_adamw_step"]
    finally:
        arena.fold_store = False


def test_the_cache_key_separates_the_contexts(model_arena, calls):
    model, arena = model_arena
    Q = ops.ReduceQueue
    lin = _sink(model, "global_sap_head.net.0.weight")
    arena.fold_check_zero = lambda stores: None
    try:
        for ctx in (None, arena.store_ok, None, arena.store_ok):
            Q.store_ok = ctx
            Q.add_accum(1 << 20, lin[0], 2, lin[1], lib.BF16)
            Q.flush(torch.device("cpu"))
            assert (Q.fold_norm is not None) == (ctx is not None)
    finally:
        del arena.fold_check_zero
    assert sorted(k[1] is None for k in Q._accum_tables) == [False, True]
    by_ctx = {k[1] is None: e for k, e in Q._accum_tables.items()}
    assert by_ctx[True]["stores"] == [] and not by_ctx[True]["flagged"] and by_ctx[False]["stores"] == [lin]
    assert [c[1][0] for c in calls][0::2] == [by_ctx[True]["tables"][0][0].data_ptr()] * 2
    assert [c[1][0] for c in calls][1::2] == [by_ctx[False]["tables"][0][0].data_ptr()] * 2
    # BEVBERT_FOLD_STORE=0 at import: the context is ignored
    Q.FOLD_STORE = False
    Q.store_ok = arena.store_ok
    Q.add_accum(1 << 20, lin[0], 2, lin[1], lib.BF16)
    Q.flush(torch.device("cpu"))
    assert Q.fold_norm is None and calls[-1][1][0] == by_ctx[True]["tables"][0][0].data_ptr()


def test_the_fused_norm_is_used_once_by_its_owner_and_only_on_request(model_arena, calls):
    model, arena = model_arena
    Q = ops.ReduceQueue
    lin = _sink(model, "global_sap_head.net.0.weight")
    names = lambda: [c[0] for c in calls]
    arena._fold_check_norm = lambda *a: None             # (self-check (b) reads device scalars)
    arena.fold_check_zero = lambda stores: None
    try:
        def fold():
            del calls[:]
            Q.store_ok = arena.store_ok
            Q.add_accum(1 << 20, lin[0], 2, lin[1], lib.BF16)
            Q.flush(torch.device("cpu"))
            del calls[:]
        # a bare clip_and_step -- gradients filled by hand, or edited after the backward pass: the whole arena is read
        arena.clip_and_step(1e-4)
        assert names() == ["bevbert_grad_norm_clip", "bevbert_adamw_step"]
        fold()
        arena.clip_and_step(1e-4)
        assert names() == ["bevbert_grad_norm_clip", "bevbert_adamw_step"]
        assert calls[0][1][:2] == (arena.grads.data_ptr(), arena.numel)
        # on request, with this step's record: the rest of the arena, the slots, AdamW -- once
        fold()
        arena.clip_and_step(1e-4, max_norm=None, grad_pre_scale=0.5, fused_norm=True)
        assert names() == ["bevbert_sumsq_tasks", "bevbert_clip_from_slots", "bevbert_adamw_step"]
        ntasks = calls[0][1][1]
        assert calls[1][1][1:4] == ((lin[1] // 4 + 4095) // 4096 + ntasks, 0.5, -1.0)
        del calls[:]
        arena.clip_and_step(1e-4, fused_norm=True)
        assert names() == ["bevbert_grad_norm_clip", "bevbert_adamw_step"]
        # zero_grad voids the record; so does a record another arena owns
        fold()
        arena._arm_fold()
        arena.clip_and_step(1e-4, fused_norm=True)
        assert names() == ["bevbert_grad_norm_clip", "bevbert_adamw_step"]
        fold()
        Q.fold_norm = dict(Q.fold_norm, owner=object())
        arena.clip_and_step(1e-4, fused_norm=True)
        assert names() == ["bevbert_grad_norm_clip", "bevbert_adamw_step"]
    finally:
        del arena._fold_check_norm, arena.fold_check_zero


def test_an_arena_whose_trainer_exchanges_gradients_never_stores(model_arena, calls):
    """reducer.active (or the early flush) leaves ``fold_store`` off: zero_grad arms nothing, the fold accumulates, no
    record is left and the optimiser reads the whole arena -- also when asked for the fused norm."""
    model, arena = model_arena
    Q = ops.ReduceQueue
    lin = _sink(model, "global_sap_head.net.0.weight")
    assert arena.fold_store is False
    Q.store_ok = lambda p, n: True                      # (a context another arena left behind)
    arena._arm_fold()
    assert Q.store_ok is None
    Q.add_accum(1 << 20, lin[0], 2, lin[1], lib.BF16)
    Q.flush(torch.device("cpu"))
    (entry,) = Q._accum_tables.values()
    assert Q.fold_norm is None and not entry["flagged"] and not any(s or n for s, n, _ in _flags_of(entry)[0])
    del calls[:]
    arena.clip_and_step(1e-4, fused_norm=True)
    assert [c[0] for c in calls] == ["bevbert_grad_norm_clip", "bevbert_adamw_step"]


def test_the_trainer_allows_store_mode_only_alone_on_a_gpu():
    assert fold_store_allowed("cuda", False, env={})
    assert not fold_store_allowed("cuda", True, env={})          # gradients change after the fold (all-reduce)
    assert not fold_store_allowed("cpu", False, env={})
    assert not fold_store_allowed("cuda", False, env={"BEVBERT_FOLD_STORE": "0"})
    assert fold_store_allowed("cuda", False, env={"BEVBERT_FOLD_STORE": "1"})
