"""The fp64 references, the inputs and the derived gates of tests/test_gpu_body_kernels.py, checked without a GPU
(tests/body_cases.py holds them): every reference against the plain torch composition on fp64 inputs to 1e-12 of the
result's scale, the GELU gate's K against two fp32 forms on the GPU test's own inputs, the edges the cases are there for,
and the fp32 restatements behind the two gates whose derivation the kernels' arithmetic forces."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import body_cases as bc
from tests.body_cases import DT_ID, DTYPES, U22, U24

TIGHT = 1e-12


def _close(a, b):
    a, b = a.double(), b.double()
    return float((a - b).detach().abs().max()) <= TIGHT * max(1.0, float(b.detach().abs().max()))


# ----------------------------------------------------------------------------- GELU
@pytest.mark.parametrize("rows,C", bc.GELU_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
def test_gelu_gate_holds_for_two_fp32_forms_with_half_its_K(dtype, rows, C):
    """K = 4 units of 2^-22 max(1, |x + bias|) is not read off the kernel: torch's own fp32 GELU (forward and autograd) and
    the numpy fp32 restatement of the Abramowitz-Stegun form (exact division, numpy's exp2) stay within K / 2 on the very
    inputs the GPU test uses, which leaves a factor 2 for the device's rcp and exp2."""
    x, bias, dy = bc.gelu_case(rows, C, dtype)
    a, y, grad, _, _ = bc.gelu_ref(x, bias, dy)
    unit = U22 * a.clamp_min(1.0)
    u32 = (x.float() + bias).requires_grad_(True)
    y32 = F.gelu(u32)
    y32.sum().backward()
    fy, fg = bc.gelu_fast_f32(u32.detach().numpy())
    worst = {}
    for name, got, want in (("torch y", y32.detach(), y), ("torch dy", u32.grad, grad),
                            ("fast y", torch.from_numpy(fy), y), ("fast dy", torch.from_numpy(fg), grad)):
        worst[name] = float(((got.double() - want).abs() / unit).max())
    print(f"body-kernel-errors: host gelu {DT_ID(dtype)} {rows}x{C} units of 2^-22 max(1, a): " +
          "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v <= bc.GELU_K / 2 for v in worst.values()), worst


@pytest.mark.parametrize("rows,C", [(1, 4), (7, 36), (17, 1028), (8192, 8)])
def test_gelu_reference_equals_torch_fp64_and_cases_hold_their_edges(rows, C):
    x, bias, dy = bc.gelu_case(rows, C, torch.float64)
    u = (x + bias.double()).requires_grad_(True)
    yt = F.gelu(u)
    yt.backward(dy)
    a, y, grad, dx, dbias = bc.gelu_ref(x, bias, dy)
    assert _close(y, yt) and _close(dx, u.grad) and _close(dbias, u.grad.sum(0))
    for dtype in DTYPES:
        x, bias, dy = bc.gelu_case(rows, C, dtype)
        s = x.float() + bias
        assert s[0, 0] == 0 and s[0, 1] == 0 and math.copysign(1.0, float(s[0, 1])) == -1.0 and s[0, 2] == 40 and s[0, 3] == -40
        assert bool((dy == 0).any()) and bool((dy != 0).any())
    if rows * C >= 64:                      # every unit interval of [-14, 14] occurs, the negative tail included
        s = (x.float() + bias).view(-1)
        assert all(bool(((s >= lo) & (s < lo + 1)).any()) for lo in range(-14, 14))


def test_gelu_fast_form_is_accurate_absolutely_and_not_relatively():
    """What csrc/common.h may claim for the Abramowitz-Stegun form: absolute error below 1e-6 everywhere, relative error on
    the negative tail growing to percents (measured: 4.2e-7 absolute; 3.6e-3 on [-6, -4], 1.0e-2 on [-8, -6], 3.7e-2 on
    [-13, -10])."""
    u = torch.linspace(-14, 14, 280001, dtype=torch.float64).float()
    _, y, grad, _, _ = bc.gelu_ref(u[None], torch.zeros(1), torch.ones(1, len(u)))
    fy, fg = bc.gelu_fast_f32(u.numpy())
    ey, eg = (torch.from_numpy(fy).double() - y[0]).abs(), (torch.from_numpy(fg).double() - grad[0]).abs()
    assert float(ey.max()) < 1e-6 and float(eg.max()) < 1e-6
    rel = ey / y[0].abs().clamp_min(1e-300)
    tail = lambda lo, hi: float(rel[(u >= lo) & (u <= hi)].max())
    assert tail(-6, -4) > 1e-3 and tail(-13, -10) > 1e-2 and tail(-13, -10) < 0.1


# ----------------------------------------------------------------------------- scatter, segments
@pytest.mark.parametrize("kind", bc.SCATTER_KINDS)
def test_scatter_reference_equals_index_add_and_cases_hold_their_edges(kind):
    ids = bc.scatter_ids(kind)
    g = torch.Generator().manual_seed(1)
    d = torch.randn(len(ids), 40, generator=g, dtype=torch.float64)
    base = torch.randn(bc.TABLE_ROWS, 40, generator=g, dtype=torch.float64)
    want, _, touched = bc.scatter_ref(ids, d)
    assert _close(want, torch.zeros_like(base).index_add_(0, ids, d))
    want2, _, _ = bc.scatter_ref(ids, d, base)
    assert _close(want2, base.clone().index_add_(0, ids, d)) and torch.equal(want2[~touched], base[~touched])
    assert not bool(touched[30:36].any()) and int(ids.min()) >= 0 and int(ids.max()) < bc.TABLE_ROWS
    if kind == "r257":
        assert len(ids) == 257 and (ids == 0).nonzero().view(-1).tolist() == [0, 256]
    if kind == "quarters":
        rows = (ids == 2).nonzero().view(-1)
        assert len(ids) == 1000 and len(rows) == 700 and int(rows[0]) == 0
        assert all(bool(((rows >= 250 * q) & (rows < 250 * (q + 1))).any()) for q in range(4))
        assert (ids == 36).nonzero().view(-1).tolist() == [999]
    if kind == "firstlast":
        assert (ids == 9).nonzero().view(-1).tolist() == [0, len(ids) - 1]
    if kind == "r1100":
        first = int((ids == ids[0]).nonzero()[0])
        assert (len(ids) - first + 3) // 4 > 256


def test_second_scatter_gate_counts_the_stored_row_as_a_term():
    """Sum of k rows onto a stored value v in fp32: the last addition alone errs by up to 2^-24 |v + sum|, which
    (k + 2) 2^-24 sum |d| over the k new rows cannot cover when |v| is large; with v as one more term it does."""
    v, d = np.float32(1024.0), np.float32(1.0 + 2.0 ** -15)
    err = abs(float(np.float32(v + d)) - (float(v) + float(d)))
    assert err > 3 * U24 * abs(float(d)) and err <= 4 * U24 * (abs(float(v)) + abs(float(d)))


@pytest.mark.parametrize("segments", [bc.SEGMENTS_A, bc.SEGMENTS_B], ids=["A", "B"])
def test_segment_reference_equals_a_dense_matrix_product(segments):
    rowptr, idx, w = bc.segment_lists(segments)
    g = torch.Generator().manual_seed(2)
    src = torch.randn(bc.SEG_N_SRC, 40, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(len(segments), 40, generator=g, dtype=torch.float64)
    A = torch.zeros(len(segments), bc.SEG_N_SRC, dtype=torch.float64)
    for r in range(len(segments)):
        for e in range(rowptr[r], rowptr[r + 1]):
            A[r, idx[e]] += float(np.float32(w[e]))
    out = A @ src
    out.backward(dy)
    want, _, dsrc, _ = bc.segment_ref(rowptr, idx, w, src.detach(), bc.SEG_N_SRC, dy)
    assert _close(want, out) and _close(dsrc, src.grad)
    assert [len(s) for s in bc.SEGMENTS_A] == [0, 1, 5, 130, 2, 0] and sum(map(len, bc.SEGMENTS_B)) < sum(map(len, bc.SEGMENTS_A))
    unread = sorted(set(range(bc.SEG_N_SRC)) - {i for s in segments for i in s})
    assert unread and bool((dsrc[unread] == 0).all()) and bool((want[[r for r, s in enumerate(segments) if not s]] == 0).all())


# ----------------------------------------------------------------------------- BertEmbeddings
@pytest.mark.parametrize("V,H,B,L", bc.EMBED_SHAPES)
@pytest.mark.parametrize("padding_idx", [None, 0])
def test_embedding_reference_equals_layer_norm_autograd(V, H, B, L, padding_idx):
    case = bc.embed_case(V, H, B, L)
    ref, tor = bc.embed_ref(case, torch.float64, padding_idx), bc.embed_torch(case, torch.float64, padding_idx, torch.float64)
    for k in ("y", "word", "pos", "typ", "gamma", "beta"):
        assert _close(ref[k], tor[k]), k
    ids = case["ids"].view(-1)
    assert bool((ids == 0).any()) and (B * L == 1 or (int((ids == 0).sum()) >= 2 and int((ids == (7 if V > 7 else 3)).sum()) >= 2))
    if padding_idx == 0:
        assert bool((ref["word"][0] == 0).all())
    assert bool((ref["typ"][1 - case["type_index"]] == 0).all())


# ----------------------------------------------------------------------------- graph bias
@pytest.mark.parametrize("layers,B,nh,G", bc.GRAPH_SHAPES)
def test_graph_bias_reference_equals_the_broadcast_product(layers, B, nh, G):
    dbias, dists = bc.graph_case(layers, B, nh, G)
    w = torch.tensor(0.0, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(0.0, dtype=torch.float64, requires_grad=True)
    bias = (dists.double() * w + b)[None, :, None].expand(layers, B, nh, G, G)
    bias.backward(dbias.double())
    dw, db, gw, gb = bc.graph_ref(dbias, dists)
    scale = max(1.0, abs(dw), abs(db))
    assert abs(dw - bc.GRAPH_DW0 - float(w.grad)) <= TIGHT * scale * 10 and abs(db - bc.GRAPH_DB0 - float(b.grad)) <= TIGHT * scale * 10
    n = dbias.numel()
    assert bc.graph_blocks(n) == (512 if n > 512 * 4096 else (n + 4095) // 4096)
    if B > 1:
        assert not torch.equal(dists[0], dists[1]) and float(dists.min()) >= 0
    assert (layers, B, nh, G) != (2, 3, 12, 63) or (n == 285768 and n % 256 and n % 4096)
    assert (layers, B, nh, G) != (4, 8, 12, 80) or n == 2457600


# ----------------------------------------------------------------------------- dropout_add, cast_f32
def test_dropout_add_gate_against_the_fp32_restatement():
    """y = x * fl(1 / fl(1 - p)) + res in numpy fp32 (every element kept) against the fp64 want on randn inputs.  With a
    residual this plain arithmetic exceeds 2 x 2^-24 (|x| / (1 - p) + |res|), the gate as first stated (four roundings touch
    the x term, see body_cases.dropout_want), and holds 2^-24 (4 |x| / (1 - p) + 2 |res|), which the GPU test uses."""
    g = torch.Generator().manual_seed(9)
    n = 1 << 20
    x, res = torch.randn(n, generator=g), torch.randn(n, generator=g)
    keep = torch.ones(n, dtype=torch.bool)
    ks = np.float32(1.0) / (np.float32(1.0) - np.float32(bc.DROP_P))
    scale_err = abs(float(ks) - 1.0 / (1.0 - float(np.float32(bc.DROP_P)))) * (1.0 - float(np.float32(bc.DROP_P)))
    assert 0.7 * U24 < scale_err < 0.8 * U24
    for r in (None, res):
        got = torch.from_numpy((x.numpy() * ks + (0 if r is None else r.numpy())).astype(np.float32)).double()
        want, gate, stated = bc.dropout_want(x, r, keep)
        ratio, ratio_stated = float(((got - want).abs() / gate).max()), float(((got - want).abs() / stated).max())
        print(f"body-kernel-errors: host dropout_add fp32 restatement, residual {r is not None}: worst error / gate {ratio:.3f}"
              f"  / gate as first stated {ratio_stated:.3f}")
        assert ratio <= 1.0 and (ratio_stated > 1.0) == (r is not None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=DT_ID)
def test_cast_values_hold_their_edges(dtype):
    v = bc.cast_values(bc.CAST_BIG_N, dtype)
    out = v.to(dtype)
    assert len(v) == bc.CAST_BIG_N and bool(out.isnan().any()) and bool(out.isinf().any())
    fin = torch.isfinite(v)
    assert bool((out[fin].isinf()).any())                                      # finite values that round to inf
    assert bool(((out == 0) & (v != 0)).any())                                 # underflow to zero
    tiny = torch.finfo(dtype).tiny
    assert bool(((out != 0) & (out.float().abs() < tiny)).any())               # subnormal results
    h = 2.0 ** (-8 if dtype == torch.bfloat16 else -11)
    assert float(torch.tensor(1 + h).to(dtype)) == 1.0 and float(torch.tensor(1 + 3 * h).to(dtype)) == 1 + 4 * h
    assert bool((v[:4] == torch.tensor([1 + h, 1 + 3 * h, -(1 + h), -(1 + 3 * h)])).all())
    assert torch.equal(v[-4:].flip(0).view(torch.int32), v[:4].view(torch.int32))
    assert len(bc.cast_values(4, dtype)) == 4
