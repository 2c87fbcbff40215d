"""The one rule for where a parameter gradient goes (ops_core.grad_dest / grad_dests), on the CPU: every op that produces a
parameter gradient runs on a CPU ParamArena with the C ABI stubbed -- the stubs of scripts/host_dryrun_profile.py, installed
through monkeypatch -- and the recorded calls say which destination pointers the kernels were handed.

A trainable parameter is touched exactly when the backward ran and its kernel got a non-null pointer; a frozen one is not
touched, gets a null pointer (or no launch) and leaves the others as they were.  CPU tensors take the direct route of every
two-stage reduction (ops.defers_finalize wants a device), so the lists below are the direct forms."""
import importlib.util
import os

import pytest
import torch

from tests import grad_dest_cases as gc

_spec = importlib.util.spec_from_file_location(
    "host_dryrun_profile", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "host_dryrun_profile.py"))
dry = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dry)

# op -> label -> (entry, index of the destination among the entry's arguments); None: the gradient is made by torch ops on
# the CPU (sink.add_ / addmm_), seen in the arena itself
LN = "bevbert_layernorm_bwd_add"
WHERE = {
    "layernorm": {"gamma": (LN, 8), "beta": (LN, 9)},
    "bdrl": {"gamma": (LN, 8), "beta": (LN, 9), "bias": (LN, 10)},
    "bdrl_row": {"gamma": (LN, 8), "beta": (LN, 9), "bias": (LN, 10)},
    "prenorm": {"gamma": (LN, 8), "beta": (LN, 9), "bias": (LN, 10)},
    "gelu": {"bias": ("bevbert_bias_gelu_bwd", 4)},
    "relu": {"bias": ("bevbert_bias_relu_bwd", 4)},
    "linear": {"weight": None, "bias": ("bevbert_colsum", 1)},
    "linear3": {"weight": None, "bias": None},
    "linear_packed": {"weight": None, "bias": ("bevbert_colsum", 1)},
    "hoisted_kv": {"weight": None, "bias": ("bevbert_colsum", 1)},
    "embed_ln": {"word": ("bevbert_embedding_grad", 2), "pos": ("bevbert_colsum_any", 1), "typ": ("bevbert_layernorm_bwd", 9),
                 "gamma": ("bevbert_layernorm_bwd", 7), "beta": ("bevbert_layernorm_bwd", 8)},
    "smallk": {"W": ("bevbert_smallk_linear_layernorm_bwd", 7), "b": ("bevbert_smallk_linear_layernorm_bwd", 8),
               "gamma": ("bevbert_smallk_linear_layernorm_bwd", 9), "beta": ("bevbert_smallk_linear_layernorm_bwd", 10),
               "table": ("bevbert_embedding_grad_sliced", 0)},
    "graph_bias": {"weight": ("bevbert_graph_bias_bwd", 6), "bias": ("bevbert_graph_bias_bwd", 7)},
    "use_param": {"p": None},
    "lookup": {"table": None},
}

# the calls of the all-trainable case, forward and backward: the name, then "1" per pointer argument handed over and "0" per
# null one (the stream included).  This is the sequence before the rule existed, but for the two sites that used to defer
# on CPU tensors too, which no launch can reach: bevbert_bias_{gelu,relu}_bwd (then 1111011, a scratch address in the
# workspace's place) and the Linear biases (then bevbert_colsum_partials 111).
CALLS = {
    "layernorm": ["bevbert_bias_dropout_residual_layernorm_fwd 1001110111", "bevbert_layernorm_bwd_add 1111110011011"],
    "bdrl": ["bevbert_bias_dropout_residual_layernorm_fwd 1111111111", "bevbert_layernorm_bwd_add 1111110011111"],
    "bdrl_row": ["bevbert_bias_dropout_residual_layernorm_fwd 1111111111", "bevbert_layernorm_bwd_add 1111110011111"],
    "prenorm": ["bevbert_bias_dropout_residual_layernorm_fwd 1111111111", "bevbert_layernorm_bwd_add 1111110111111"],
    "gelu": ["bevbert_bias_gelu_fwd 1111", "bevbert_bias_gelu_bwd 1111111"],
    "relu": ["bevbert_bias_relu_fwd 1111", "bevbert_bias_relu_bwd 1111111"],
    "linear": ["bevbert_colsum 1111"],
    "linear3": [],
    "linear_packed": ["bevbert_colsum 1111"],
    "hoisted_kv": ["bevbert_colsum 1111"],
    "embed_ln": ["bevbert_embed_sum_layernorm_fwd 11111111111", "bevbert_layernorm_bwd 111111011111",
                 "bevbert_embedding_grad 1111", "bevbert_colsum_any 111"],
    "smallk": ["bevbert_smallk_linear_layernorm_fwd 111111111111", "bevbert_smallk_linear_layernorm_bwd 1111111111111",
               "bevbert_embedding_grad_sliced 1111"],
    "graph_bias": ["bevbert_graph_bias_fwd 11111", "bevbert_graph_bias_bwd 111111"],
    "use_param": [],
    "lookup": [],
}


@pytest.fixture
def stubbed(monkeypatch):
    from vln_bevbert_amd import ops
    dry.install_stubs(monkeypatch.setattr)
    monkeypatch.setattr(dry, "RECORD", True)
    monkeypatch.setattr(ops.RT, "res32", False)
    dry.CALLS.clear()
    yield ops
    dry.CALLS.clear()
    ops.ReduceQueue.drop_pending()


def _run(ops, op, frozen=()):
    """(arena, recorded calls, whether a backward ran) of one forward + backward of ``op`` with the labels ``frozen``."""
    from vln_bevbert_amd.arena import ParamArena
    labels, _, run = gc.OPS[op]
    torch.manual_seed(0)
    m = gc.Params(torch.float32)
    gc.freeze(m, {n for l in frozen for n in labels[l]})
    m.arena = ParamArena(m, "cpu", torch.float32, groups=gc.GROUPS)
    del dry.CALLS[:]
    outs, grads = run(ops, m, gc.inputs(torch.float32, "cpu"))
    ran = any(o.requires_grad for o in outs)
    if ran:
        torch.autograd.backward(outs, grads)
    return m.arena, list(dry.CALLS), ran


def _nonnull(calls, where):
    entry, i = where
    return any(c[0] == entry and c[1 + i] == "ptr" for c in calls)


def _changed(arena, names):
    return {n for n in names if bool(arena.grads[arena.slices[n][0]:sum(arena.slices[n])].any())}


def _mask(calls):
    return [c[0] + " " + "".join("1" if a == "ptr" else "0" for a in c[1:] if a in ("ptr", "null")) for c in calls]


@pytest.mark.parametrize("op", list(gc.OPS))
def test_trainable_is_touched_and_gets_a_pointer_frozen_gets_neither(stubbed, op):
    labels = gc.OPS[op][0]
    everything = {n for names in labels.values() for n in names}
    arena, calls, ran = _run(stubbed, op)
    assert ran and arena._touched == everything
    for label, names in labels.items():
        where = WHERE[op][label]
        assert _nonnull(calls, where) if where else _changed(arena, names) == set(names), label
    assert _mask(calls) == CALLS[op], _mask(calls)
    for label, names in labels.items():
        arena, calls, ran = _run(stubbed, op, frozen=(label,))
        # the other inputs still want their gradients; use_param and lookup have none, so autograd never calls them
        assert ran == (op not in ("use_param", "lookup")), label
        assert arena._touched == everything - set(names), (label, arena._touched)
        assert not _changed(arena, names), label
        for other, onames in labels.items():
            where = WHERE[op][other]
            if where:
                assert _nonnull(calls, where) == (other != label), (label, other)
            else:
                assert _changed(arena, onames) == (set() if other == label else set(onames)), (label, other)


def test_all_frozen_touches_nothing(stubbed):
    """The issue's probe: a LayerNorm, a GELU bias and a Linear, all frozen, inside a graph whose input wants a gradient."""
    for op in ("bdrl", "gelu", "linear"):
        arena, calls, ran = _run(stubbed, op, frozen=tuple(gc.OPS[op][0]))
        assert ran and not arena._touched and not bool(arena.grads.any()), op
        assert not any(_nonnull(calls, w) for w in WHERE[op].values() if w), op


def test_arena_gamma_with_a_plain_bias_is_refused(stubbed):
    from vln_bevbert_amd.arena import ParamArena
    ops = stubbed
    m = gc.Params(torch.float32)
    arena = ParamArena(m, "cpu", torch.float32, groups=gc.GROUPS)
    i = gc.inputs(torch.float32, "cpu")
    plain = torch.zeros(gc.H, requires_grad=True)
    y = ops.bias_dropout_residual_layernorm(i["x"].clone().requires_grad_(True), plain, i["res"], m.ln.weight, m.ln.bias, gc.EPS)
    with pytest.raises(AssertionError, match="mixed"):
        y.backward(i["dy"])
    assert not arena._touched                               # (refused before anything was flagged)


def test_params_in_arena():
    from vln_bevbert_amd import ops
    from vln_bevbert_amd.arena import ParamArena
    lin = torch.nn.Linear(3, 2)
    assert not ops.params_in_arena(lin.parameters())
    lin.bias.requires_grad_(False)
    assert not ops.params_in_arena(lin.parameters()) and ops.params_in_arena([lin.bias])
    ParamArena(lin, "cpu")
    assert ops.params_in_arena(lin.parameters())
    assert not ops.params_in_arena([torch.zeros(2, dtype=torch.bfloat16)])
