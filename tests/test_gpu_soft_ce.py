"""bevbert_soft_ce_fwd / _bwd (csrc/sap_loss.hip, ops.soft_ce_rows) on the MI355X against fp64 torch:
F.kl_div(F.log_softmax(x, -1), t[idx], reduction="none").sum(1) and its autograd gradient on the values the kernel gets
(tests/soft_ce_cases.py holds the case matrix and the reference; tests/test_soft_ce_host.py shows on the CPU that every
case has finite fp64 losses and that the kernel's gradient formula is that gradient).

Gates, none taken from the code under test (the scheme of tests/test_gpu_loss_kernels.py, floors of the CE sibling):
  loss       max |got - want| <= max(2e-5 max(1, |want|max), 4 x e32)
  d logits   max |got - want| <= max(1e-6 max(1, |want|max), 4 x e32), plus 2^-8 |want| per element when stored in bf16
with e32 the distance of torch's fp32 composition (CPU) from fp64 on the same inputs.  Sentinels behind every output stay
untouched, and a second run gives the same bits.  Under ``-s`` every test prints its worst errors (lines that begin with
"loss-kernel-errors:"); profiles/loss_kernel_errors.txt holds them from the MI355X."""
import pytest
import torch

from tests import soft_ce_cases as S
from tests.kernel_gates import Worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
_ID = {torch.float32: "f32", torch.bfloat16: "bf16"}.get
PAD = 24                # sentinel elements behind every output
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


def _run_raw(case):
    """The two C-ABI entries on buffers with sentinels behind them: (loss, stats (3, R), d logits), each checked."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    x, t = case["x"].to(DEV), case["t"].to(DEV)
    idx = None if case["idx"] is None else case["idx"].to(DEV)
    w = case["w"].to(DEV)
    R, C = x.shape
    loss = torch.full((R + PAD,), SENTINEL, device=DEV)
    stats = torch.full((3 * R + PAD,), SENTINEL, device=DEV)
    d = torch.full((R * C + PAD,), SENTINEL, device=DEV, dtype=x.dtype)
    call("bevbert_soft_ce_fwd", ptr(x), ptr(t), ptr(idx), ptr(loss), ptr(stats), R, C, dtype_code(x), stream())
    call("bevbert_soft_ce_bwd", ptr(x), ptr(t), ptr(idx), ptr(stats), ptr(w), ptr(d), R, C, dtype_code(x), stream())
    torch.cuda.synchronize()
    for name, buf, n in (("loss", loss, R), ("stats", stats, 3 * R), ("d_logits", d, R * C)):
        assert bool((buf[n:].float() == SENTINEL).all()), f"{name}: the kernel wrote behind its output"
    return loss[:R].clone(), stats[:3 * R].view(3, R).clone(), d[:R * C].view(R, C).clone()


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
@pytest.mark.parametrize("C", S.C_VALUES)
def test_soft_ce_rows_against_fp64(ops, C, dtype):
    worst = Worst(f"soft_ce {_ID(dtype)} C={C}")
    for where, case in S.inner_cases(C, dtype):
        loss, stats, d = _run_raw(case)
        (want, dwant), (l32, d32) = S.reference(case, torch.float64), S.reference(case, torch.float32)
        assert bool(torch.isfinite(want).all())
        worst.check("loss", loss, want, l32, 2e-5, where=where)
        worst.check("d_logits", d, dwant, d32, 1e-6, bf16_out=dtype == torch.bfloat16, where=where)
        # the third statistic is the sum of the target row
        t64 = S.picked(case).double()
        worst.bound("sum_t", stats[2], t64.sum(1), (C + 16) * 2.0 ** -24 * t64.abs().sum(1) + 1e-30, where=where)
        # an all-zero target row: loss and gradient exactly zero
        zero = (t64.abs().sum(1) == 0).to(DEV)
        assert bool((loss[zero] == 0).all()) and bool((d[zero].float() == 0).all()), where
        # equal bits on a second run
        loss2, stats2, d2 = _run_raw(case)
        assert torch.equal(loss, loss2) and torch.equal(stats, stats2) and torch.equal(d, d2), where
    worst.report()


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
@pytest.mark.parametrize("C,R", [(5, 7), (1000, 65), (1025, 7)])
def test_soft_ce_autograd_function_gives_the_bits_of_the_entries(ops, C, R, dtype):
    """ops.soft_ce_rows (the autograd Function the MRC head calls) against the raw entries on the same inputs; targets get
    no gradient; a strided upstream gradient and a non-contiguous logits view are made contiguous, not misread."""
    for mode in S.IDX_MODES:
        case = S.make_case(C, R, 30.0, dtype, mode, seed=1)
        loss_raw, _, d_raw = _run_raw(case)
        # the logits as a column slice of a wider tensor (row stride C + 3) and the upstream gradient as a column of a
        # (R, 2) tensor (stride 2), handed to backward as it is
        wide = torch.zeros(R, C + 3, dtype=dtype, device=DEV)
        wide[:, :C] = case["x"].to(DEV)
        wide.requires_grad_(True)
        x = wide[:, :C]
        t = case["t"].to(DEV).requires_grad_(True)
        idx = None if case["idx"] is None else case["idx"].to(DEV)
        w2 = torch.stack([case["w"], -case["w"]], 1).to(DEV)
        assert not x.is_contiguous() and not w2[:, 0].is_contiguous()
        loss = ops.soft_ce_rows(x, t, idx)
        assert loss.dtype == torch.float32 and loss.shape == (R,)
        loss.backward(w2[:, 0])
        assert torch.equal(loss.detach(), loss_raw) and t.grad is None, mode
        assert torch.equal(wide.grad[:, :C], d_raw) and not bool(wide.grad[:, C:].any()), mode
    with pytest.raises(Exception):
        ops.soft_ce_rows(case["x"], case["t"], None)               # CPU tensors: no fallback
