"""Inputs and fp64 reference of the soft-target cross-entropy rows (bevbert_soft_ce_fwd / _bwd, ops.soft_ce_rows), shared
by tests/test_soft_ce_host.py (CPU: the restated gradient, the finiteness of every case) and tests/test_gpu_soft_ce.py.

The reference is torch's own composition in fp64 on the values the kernel gets (bf16 logits are rounded first, then
widened): F.kl_div(F.log_softmax(x, -1), t, reduction="none").sum(1) and its autograd gradient.

Case matrix: C in C_VALUES (odd C: rows start at every residue of four elements; 1023 / 1025 straddle the switch from one
wave to one workgroup per row; 2053: the strided vector loop runs twice), R in R_VALUES (one row, a partly filled workgroup
of four waves, more than one workgroup), fp32 and bf16 logits at scale 1 and 30, target rows read directly (idx None),
through a permutation and through an index with duplicates.  Target row r is of kind r % 6:
  0  softmax of 8 x randn             1  one-hot on column C - 1          2  all zero
  3  kind 0 scaled by 0.5             4  kind 0 scaled by 2               5  kind 0 with two equal maxima
(3 and 4: a backward that assumes sum(t) = 1 fails there).  dloss has a zero and a negative entry."""
import torch
import torch.nn.functional as F

C_VALUES = (1, 3, 5, 64, 255, 1000, 1023, 1025, 2053)
R_VALUES = (1, 7, 65)
SCALES = (1.0, 30.0)
IDX_MODES = ("none", "perm", "dup")
DTYPES = (torch.float32, torch.bfloat16)
KINDS = 6


def target_rows(n, C, g):
    """(n, C) fp32 target rows, row r of kind r % 6 (see the module docstring)."""
    t = torch.softmax(8.0 * torch.randn(n, C, generator=g), -1)
    for r in range(n):
        k = r % KINDS
        if k == 1:
            t[r] = 0.0
            t[r, C - 1] = 1.0
        elif k == 2:
            t[r] = 0.0
        elif k == 3:
            t[r] *= 0.5
        elif k == 4:
            t[r] *= 2.0
        elif k == 5 and C >= 2:
            top = torch.topk(t[r], 2).indices
            t[r, top[1]] = t[r, top[0]]
    return t.contiguous()


def dloss_rows(n, g):
    w = torch.randn(n, generator=g)
    w[1 % n] = 0.0
    w[2 % n] = -0.5 - w[2 % n].abs()
    return w


def make_case(C, R, scale, dtype, idx_mode, seed=0):
    """{x (R, C) in dtype, t (R, C) fp32, idx (R) int64 or None, w (R) fp32}; row r reads t[idx[r]]."""
    g = torch.Generator().manual_seed(1000 * C + 10 * R + int(scale) + seed)
    x = (scale * torch.randn(R, C, generator=g)).to(dtype)
    t = target_rows(R, C, g)
    if idx_mode == "none":
        idx = None
    elif idx_mode == "perm":
        idx = torch.randperm(R, generator=g)
    else:
        idx = torch.randint(0, R, (R,), generator=g)
        idx[-1] = idx[0]                          # at least one duplicate whenever R > 1
    return {"x": x, "t": t, "idx": idx, "w": dloss_rows(R, g)}


def picked(case):
    return case["t"] if case["idx"] is None else case["t"].index_select(0, case["idx"])


def reference(case, dt=torch.float64):
    """(loss (R), d logits (R, C)) of torch's composition in ``dt`` for the upstream gradient ``w``."""
    xr = case["x"].detach().cpu().to(dt).requires_grad_(True)
    loss = F.kl_div(F.log_softmax(xr, -1), picked(case).to(dt), reduction="none").sum(1)
    (loss * case["w"].to(dt)).sum().backward()
    return loss.detach(), xr.grad


def inner_cases(C, dtype):
    """The inner cases of one (C, dtype): every R, scale and index mode."""
    for R in R_VALUES:
        for scale in SCALES:
            for mode in IDX_MODES:
                yield f"R={R} scale {scale:g} idx {mode}", make_case(C, R, scale, dtype, mode)
