"""CPU pins of the soft-target cross-entropy (tests/soft_ce_cases.py): the gradient bevbert_soft_ce_bwd computes is the
autograd gradient of the reference, an all-zero target row costs nothing, and every case the GPU test builds has finite
fp64 losses (so a finite kernel result there is never compared with inf / NaN)."""
import pytest
import torch

from tests import soft_ce_cases as S


@pytest.mark.parametrize("C", S.C_VALUES)
def test_restated_gradient_equals_autograd_in_fp64(C):
    """dlogits = (softmax * S - t) * dloss with S = sum_c t -- the factor S matters on the rows scaled by 0.5 and 2."""
    worst = 0.0
    for dtype in S.DTYPES:
        for where, case in S.inner_cases(C, dtype):
            _, want = S.reference(case)
            x, t, w = case["x"].double(), S.picked(case).double(), case["w"].double()
            got = (torch.softmax(x, -1) * t.sum(1, keepdim=True) - t) * w[:, None]
            worst = max(worst, float((got - want).abs().max()))
            assert float((got - want).abs().max()) <= 1e-12, (C, dtype, where)
            if x.shape[0] >= 5 and case["idx"] is None:
                no_s = (torch.softmax(x, -1) - t) * w[:, None]             # the S = 1 shortcut is visibly wrong on rows 3, 4
                assert float((no_s - want)[3:5].abs().max()) > 1e-5, (C, dtype, where)
    print(f"soft-ce restated gradient C={C}: worst |restated - autograd| {worst:.2e}")


@pytest.mark.parametrize("C", S.C_VALUES)
def test_every_gpu_case_has_finite_fp64_losses_and_zero_rows_cost_nothing(C):
    for dtype in S.DTYPES:
        for where, case in S.inner_cases(C, dtype):
            loss, grad = S.reference(case)
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all()), (C, dtype, where)
            zero = S.picked(case).abs().sum(1) == 0
            if case["x"].shape[0] >= 3:
                assert bool(zero.any()) or case["idx"] is not None, (C, dtype, where)
            assert torch.equal(loss[zero], torch.zeros_like(loss[zero])), (C, dtype, where)
            assert torch.equal(grad[zero], torch.zeros_like(grad[zero])), (C, dtype, where)


def test_case_matrix_covers_every_target_kind_and_index_mode():
    case = S.make_case(5, 7, 1.0, torch.float32, "dup")
    t = case["t"]
    assert t.shape == (7, 5) and t.dtype == torch.float32 and t.is_contiguous()
    assert float(t[1, 4]) == 1.0 and float(t[1].sum()) == 1.0 and float(t[2].abs().sum()) == 0.0
    assert abs(float(t[3].sum()) - 0.5) < 1e-6 and abs(float(t[4].sum()) - 2.0) < 1e-6
    top = torch.topk(t[5], 2).values
    assert float(top[0]) == float(top[1])
    assert len(set(case["idx"].tolist())) < 7
    assert sorted(S.make_case(5, 7, 1.0, torch.float32, "perm")["idx"].tolist()) == list(range(7))
    w = case["w"]
    assert float(w[1]) == 0.0 and float(w[2]) < 0.0
