"""The loss-head kernels on the MI355X against plain fp64 torch, at the edges of their shapes and magnitudes:
bevbert_sap_loss_fwd/bwd, bevbert_cross_entropy_fwd/bwd, bevbert_bce_rows_fwd/bwd, bevbert_sem_select,
bevbert_weighted_mean_fwd/bwd (csrc/sap_loss.hip) and bevbert_colsum_any (csrc/colwise.hip).

Every reference is written here in fp64 on the values the kernel gets (bf16 inputs are rounded to bf16 first, then
widened).  The SAP reference (sap_logits_ref / sap_ref) restates forward_sap's tail without pretrain_cmt.fuse_sap_logits;
tests/test_loss_refs_host.py pins it to that function and to F.cross_entropy's ignore_index, and shows on the CPU that
every SAP case built here has finite fp64 losses.

Gates -- none is taken from the code under test:

* index and selection work, sentinels behind the outputs, masked gradient entries, the weighted mean's backward: exact;
* fp32 results of the SAP, CE and BCE kernels: max |got - want| <= max(floor, 4 x e32), e32 being the distance of torch's
  own fp32 composition (CPU) from the fp64 reference on the same inputs; the factor 4 covers the fast exp / log
  intrinsics, a few ulp each, against libm.  Floors are the gates these kernels had before: 2e-5 max(1, |want|max) for the
  losses and the SAP gradients, 1e-6 max(1, |want|max) for the CE gradient, 1e-5 |want|max for BCE;
* a gradient stored in bf16: elementwise 2^-8 |want| for the one output rounding, plus the fp32 gate above;
* weighted mean forward: (n + 16) 2^-24 sum |w x| / |denom|;
* colsum_any: (rows + 4) 2^-24 sum_r |dy[r, c]| per column, plus 2^-24 |want| for the rounding of the accumulated value.

Every test prints the worst error of the kernel and of torch-fp32 per case under ``-s`` (lines that begin with
"loss-kernel-errors:"); profiles/loss_kernel_errors.txt is that output from the MI355X.

What the cases found.  (1) A label of -100 (the dataset's "no target") made sap_loss_kernel read lane 28 and return a
non-zero loss and a full softmax as gradient; the kernel now drops the term as F.cross_entropy does
(test_sap_ignored_labels fails on the kernel before that change).  (2) ce_bwd_kernel formed softmax = exp(x - lse) with
lse = m + log s rounded at the size of the row maximum m.  On the MI355X at logits of scale 30 (m about 100) the fp32
gradient was off by 1.4e-6 (C = 5), 2.3e-6 (C = 1023) and 3.0e-6 (C = 2053) where torch-fp32 is off by 1e-7, outside
max(1e-6 max(1, |want|max), 4 x e32) = 1.1e-6, 1.7e-6, 1.9e-6; half an ulp of m = 340 at scale 80 is 1.5e-5 of every
probability.  The forward now leaves m and log s
apart and the backward forms exp((x - m) - log s).
"""
import pytest
import torch
import torch.nn.functional as F

from tests.kernel_gates import U8, U24, Worst            # (Worst's default prefix: "loss-kernel-errors:")

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = -float("inf")
DTYPES = [torch.float32, torch.bfloat16]
_ID = {torch.float32: "f32", torch.bfloat16: "bf16"}.get


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


# ----------------------------------------------------------------------------- SAP: reference and inputs
def sap_logits_ref(graw, lraw, fraw, visited, gmap_lens, nav_masks, cand_idxs, src, vis_c):
    """(global, local, fused) logits of forward_sap behind the three heads, in the heads' dtype: fw = sigmoid(fuse_raw) (0.5
    without a fuse head), the two masked fills, ext = [ll | sum of ll over vis_c | 0], fu = gl + ext.gather(src)."""
    fw = torch.sigmoid(fraw) if fraw is not None else 0.5
    G = graw.shape[1]
    gl = (graw * fw).masked_fill(visited, NEG)
    gl = gl.masked_fill(torch.arange(G)[None] >= gmap_lens[:, None], NEG)
    cm = nav_masks.gather(1, cand_idxs)
    ll = (lraw * (1 - fw)).masked_fill(cm.logical_not(), NEG)
    bw = torch.where(vis_c, ll, torch.zeros_like(ll)).sum(1, keepdim=True)
    ext = torch.cat([ll, bw, torch.zeros_like(bw)], 1)
    return gl, ll, gl + ext.gather(1, src)


def sap_ref(case, dt=torch.float64):
    """[loss (B), d global_raw, d local_raw, d fuse_raw or None] of the case in ``dt`` on the CPU.  F.cross_entropy's
    default ignore_index is -100: such a term is 0 and has no gradient."""
    heads = [None if t is None else t.detach().cpu().to(dt).requires_grad_(True) for t in case["heads"]]
    gl, ll, fu = sap_logits_ref(*heads, *case["ints"])
    loss = F.cross_entropy(gl, case["glab"], reduction="none") + F.cross_entropy(ll, case["llab"], reduction="none") \
        + F.cross_entropy(fu, case["glab"], reduction="none")
    (loss * case["dloss"].to(dt)).sum().backward()
    return [loss.detach()] + [None if h is None else h.grad for h in heads]


SAP_B = 8
SAP_SHAPES = [(64, 62), (1, 1), (64, 1), (2, 62), (5, 40), (23, 6)]
SAP_SRC = ["one", "sum", "none", "random"]
SAP_VIS = ["none", "all"]
SAP_IGNORE = {0: "g", 1: "g", 2: "l", 3: "l", 4: "gl", 5: "gl"}       # sample -> which labels are -100 (6, 7: none)


def sap_case(G, K, P, dtype, fuse, src_kind, vis_kind, mag, seed, ignore=False):
    """One batch of SAP_B samples on the CPU.  Per sample a labelled node and a labelled candidate that stay selectable
    (unvisited and inside gmap_lens; a navigable cell), so every fp64 loss is finite:
    sample 0: gmap_lens G, global label G - 1, local label K - 1;      sample 1: gmap_lens 1, both labels 0;
    sample 2: gmap_lens G, global label 0;     sample 3: local label K - 1;     sample 4: gmap_lens G, global label G - 1;
    the others random.  src: every node to the labelled candidate ("one"), to K, the visited-sum slot ("sum"), to K + 1
    ("none"), or random with the labelled node on a finite entry.  vis_c: nothing, or every navigable candidate.
    fuse_raw holds -30, 0 and 30 (rotated by the seed); dloss a zero and a negative entry."""
    B, g = SAP_B, torch.Generator().manual_seed(seed)
    ar = torch.arange(B)
    rint = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g)
    graw = (mag * torch.randn(B, G, generator=g)).to(dtype)
    lraw = (mag * torch.randn(B, K, generator=g)).to(dtype)
    fraw = None
    if fuse:
        fraw = torch.cat([torch.tensor([-30.0, 0.0, 30.0]), torch.randn(B - 3, generator=g)]).roll(seed % B)[:, None].to(dtype)
    node = rint(0, G, B)
    node[0], node[1], node[2], node[4] = G - 1, 0, 0, G - 1
    lens = torch.stack([rint(int(node[b]) + 1, G + 1, 1)[0] for b in range(B)])
    lens[0], lens[1], lens[2], lens[4] = G, 1, G, G
    cand = rint(0, K, B)
    cand[0], cand[1], cand[3] = K - 1, 0, K - 1
    visited = torch.rand(B, G, generator=g) < 0.3
    visited[ar, node] = False
    cand_idxs = rint(0, P, B, K)
    nav_masks = torch.rand(B, P, generator=g) < 0.7
    nav_masks[ar, cand_idxs[ar, cand]] = True
    cm = nav_masks.gather(1, cand_idxs)
    vis_c = cm.clone() if vis_kind == "all" else torch.zeros(B, K, dtype=torch.bool)
    if src_kind == "one":
        src = cand[:, None].expand(B, G).contiguous()
    elif src_kind == "sum":
        src = torch.full((B, G), K)
    elif src_kind == "none":
        src = torch.full((B, G), K + 1)
    else:
        src = rint(0, K + 2, B, G)
        src[ar, node] = torch.stack([cand, torch.full((B,), K), torch.full((B,), K + 1)])[ar % 3, ar]
    dloss = torch.randn(B, generator=g)
    dloss[3], dloss[5] = 0.0, -1.0 - dloss[5].abs()
    glab, llab = node.clone(), cand.clone()
    if ignore:
        for b, kinds in SAP_IGNORE.items():
            if "g" in kinds:
                glab[b] = -100
            if "l" in kinds:
                llab[b] = -100
    return {"heads": [graw, lraw, fraw], "ints": [visited, lens, nav_masks, cand_idxs, src, vis_c], "glab": glab, "llab": llab,
            "dloss": dloss, "cm": cm}


def _run_sap(ops, case):
    heads = [None if t is None else t.clone().to(DEV).requires_grad_(True) for t in case["heads"]]
    ints = [t.to(DEV) for t in case["ints"]]
    loss = ops.sap_loss(*heads, *ints, case["glab"].to(DEV), case["llab"].to(DEV))
    (loss * case["dloss"].to(DEV)).sum().backward()
    return [loss.detach()] + [None if h is None else h.grad for h in heads]


def _check_sap(ops, worst, case, dtype, where):
    got, want, ref32 = _run_sap(ops, case), sap_ref(case), sap_ref(case, torch.float32)
    assert bool(torch.isfinite(want[0]).all()), (where, want[0])                 # no sample left out: every loss is finite
    for name, a, w, r in zip(("loss", "d_global", "d_local", "d_fuse"), got, want, ref32):
        assert (a is None) == (w is None)
        if a is not None:
            worst.check(name, a, w, r, 2e-5, bf16_out=dtype == torch.bfloat16 and name != "loss", where=where)
    visited, lens = case["ints"][0], case["ints"][1]
    gmasked = visited | (torch.arange(visited.shape[1])[None] >= lens[:, None])
    assert bool((got[1].cpu()[gmasked] == 0).all()) and bool((got[2].cpu()[case["cm"].logical_not()] == 0).all()), where
    again = _run_sap(ops, case)
    assert all(torch.equal(a, b) for a, b in zip(got, again) if a is not None), where
    return got


@pytest.mark.parametrize("G,K", SAP_SHAPES)
@pytest.mark.parametrize("fuse", [True, False], ids=["fuse", "nofuse"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_sap_loss_at_the_lane_limits(ops, dtype, fuse, G, K):
    """Loss and the three gradients against fp64 with a label on the last lane, src == K + 1 == 63, all 64 nodes on one
    candidate, G = 1 / K = 1, one-cell and full BEV masks, head outputs of scale 1 and 20; masked entries exactly 0; equal
    bits twice."""
    worst = Worst(f"sap {_ID(dtype)} {'fuse' if fuse else 'nofuse'} G={G} K={K}")
    seed = 0
    for P in (1, 441):
        for src_kind in SAP_SRC:
            for vis_kind in SAP_VIS:
                for mag in (1.0, 20.0):
                    seed += 1
                    case = sap_case(G, K, P, dtype, fuse, src_kind, vis_kind, mag, seed)
                    _check_sap(ops, worst, case, dtype, f"P={P} src={src_kind} vis_c={vis_kind} x{mag:g}")
    worst.report()


@pytest.mark.parametrize("G,K", [(64, 62), (5, 40)])
@pytest.mark.parametrize("fuse", [True, False], ids=["fuse", "nofuse"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_sap_ignored_labels(ops, dtype, fuse, G, K):
    """Label -100 (the dataset's "no target"): samples 0-1 global only, 2-3 local only, 4-5 both, 6-7 neither.  The fp64
    reference drops the term (F.cross_entropy's ignore_index); the kernel must give its loss and gradients, so an ignored
    term changes nothing but its own contribution, and a sample with both ignored has loss 0 and no gradient at all."""
    worst = Worst(f"sap -100 {_ID(dtype)} {'fuse' if fuse else 'nofuse'} G={G} K={K}")
    seed = 100
    for src_kind in ("one", "random"):
        for mag in (1.0, 20.0):
            seed += 1
            case = sap_case(G, K, 441, dtype, fuse, src_kind, "all", mag, seed, ignore=True)
            got = _check_sap(ops, worst, case, dtype, f"src={src_kind} x{mag:g}")
            both = [b for b, kinds in SAP_IGNORE.items() if kinds == "gl"]
            for t in got:
                assert t is None or bool((t[both] == 0).all()), (src_kind, mag, t)
    worst.report()


def test_sap_loss_refuses_shapes_beyond_a_wave():
    from vln_bevbert_amd import lib
    l = lib.load()
    N = None
    for G, K in ((65, 1), (1, 63), (0, 1), (1, 0)):
        for rc in (l.bevbert_sap_loss_fwd(*[N] * 15, 8, G, K, 1, 0, N), l.bevbert_sap_loss_bwd(*[N] * 7, 8, G, K, 0, N)):
            assert rc == -1 and f"sap_loss: G={G} (<= 64) / K={K} (<= 62) out of range".encode() in l.bevbert_last_error()


# ----------------------------------------------------------------------------- cross-entropy rows
def ce_span(row, C):
    """(head, tail0) of ce_span in csrc/sap_loss.hip: the scalar head ends at the row's first element whose index in the
    tensor is a multiple of 4, the scalar tail starts behind the last whole group of 4."""
    head = min(C, (4 - (row * C) % 4) % 4)
    return head, head + 4 * ((C - head) // 4)


def ce_targets(rows, C):
    """Nine target vectors: per row 0, head - 1, head, head + 1, head + 2, head + 3, tail0 - 1, tail0, C - 1, clipped to
    [0, C) -- the head span, each lane of the first vector, the last vector and the tail."""
    out = []
    for k in range(9):
        t = []
        for r in range(rows):
            head, tail0 = ce_span(r, C)
            t.append(min(max((0, head - 1, head, head + 1, head + 2, head + 3, tail0 - 1, tail0, C - 1)[k], 0), C - 1))
        out.append(torch.tensor(t))
    return out


def _ce_dloss(rows, g):
    w = torch.randn(rows, generator=g)
    w[1 % rows] = 0.0
    w[2 % rows] = -0.5 - w[2 % rows].abs()
    return w


def _ce_ref(x, t, w, dt):
    xr = x.detach().cpu().to(dt).requires_grad_(True)
    loss = F.cross_entropy(xr, t, reduction="none")
    (loss * w.to(dt)).sum().backward()
    return loss.detach(), xr.grad


def _check_ce(ops, worst, x, t, w, where):
    xd = x.clone().to(DEV).requires_grad_(True)
    loss = ops.cross_entropy_rows(xd, t.to(DEV))
    (loss * w.to(DEV)).sum().backward()
    (want, dwant), (l32, d32) = _ce_ref(x, t, w, torch.float64), _ce_ref(x, t, w, torch.float32)
    assert bool(torch.isfinite(want).all())
    worst.check("loss", loss, want, l32, 2e-5, where=where)
    worst.check("d_logits", xd.grad, dwant, d32, 1e-6, bf16_out=x.dtype == torch.bfloat16, where=where)


CE_SHAPES = [(5, C, dt) for dt in DTYPES for C in (1, 2, 3, 4, 5)] \
    + [(r, C, dt) for dt in DTYPES for r, C in ((9, 41), (5, 1023), (6, 2053))] + [(3, 30522, torch.bfloat16)]


@pytest.mark.parametrize("rows,C,dtype", CE_SHAPES, ids=lambda v: _ID(v) or str(v))
def test_cross_entropy_every_row_start_and_target_position(ops, rows, C, dtype):
    """Odd C: the rows start at all four residues of 4, so every head length runs in both dtypes; C < 4: no vector at
    all; 2053: the strided vector loop runs twice.  Targets in the head span, in each vector lane and in the tail; logits
    of scale 3, 30 and 80; dloss with a zero and a negative entry."""
    worst = Worst(f"ce {_ID(dtype)} rows={rows} C={C}")
    g = torch.Generator().manual_seed(13 + C)
    for scale in (3.0, 30.0, 80.0):
        x = (scale * torch.randn(rows, C, generator=g)).to(dtype)
        w = _ce_dloss(rows, g)
        for k, t in enumerate(ce_targets(rows, C)):
            _check_ce(ops, worst, x, t, w, f"scale {scale:g} targets {k}")
    worst.report()


@pytest.mark.parametrize("rows,C", [(9, 41), (6, 2053)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_cross_entropy_rows_with_one_large_value_or_none(ops, dtype, rows, C):
    """Rows of equal logits (loss log C); rows whose only large value is the last element of the head span; rows whose
    only large value is the last element of the tail.  Targets on that element and away from it."""
    worst = Worst(f"ce special {_ID(dtype)} rows={rows} C={C}")
    g = torch.Generator().manual_seed(5)
    spans = [ce_span(r, C) for r in range(rows)]
    assert any(h > 0 for h, _ in spans) and any(t0 < C for _, t0 in spans)
    at_head = torch.tensor([max(h - 1, 0) for h, _ in spans])
    at_tail = torch.full((rows,), C - 1)
    w = _ce_dloss(rows, g)
    for kind, pos in (("equal", at_head), ("head", at_head), ("tail", at_tail)):
        x = torch.full((rows, C), 7.5) if kind == "equal" else 0.5 * torch.randn(rows, C, generator=g)
        if kind != "equal":
            x[torch.arange(rows), pos] = 60.0
        for name, t in (("on", pos), ("off", torch.full((rows,), C // 2))):
            _check_ce(ops, worst, x.to(dtype), t, w, f"{kind} target {name}")
    worst.report()


@pytest.mark.parametrize("rows,C", [(9, 41), (6, 2053)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_cross_entropy_backward_in_place(ops, dtype, rows, C):
    """The C ABI's documented aliasing: dlogits == logits gives the bits of the separate output."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    g = torch.Generator().manual_seed(21)
    x = (30.0 * torch.randn(rows, C, generator=g)).to(dtype).to(DEV)
    t = ce_targets(rows, C)[2].to(DEV)
    w = _ce_dloss(rows, g).to(DEV)
    loss = torch.empty(rows, device=DEV)
    lse = torch.empty(2, rows, device=DEV)
    apart, inplace = torch.full_like(x, 3.0), x.clone()
    call("bevbert_cross_entropy_fwd", ptr(x), ptr(t), ptr(loss), ptr(lse), rows, C, dtype_code(x), stream())
    call("bevbert_cross_entropy_bwd", ptr(x), ptr(t), ptr(lse), ptr(w), ptr(apart), rows, C, dtype_code(x), stream())
    call("bevbert_cross_entropy_bwd", ptr(inplace), ptr(t), ptr(lse), ptr(w), ptr(inplace), rows, C, dtype_code(x), stream())
    assert torch.equal(apart, inplace)
    worst = Worst(f"ce in place {_ID(dtype)} rows={rows} C={C}")
    worst.check("d_logits", inplace, _ce_ref(x, t.cpu(), w.cpu(), torch.float64)[1], _ce_ref(x, t.cpu(), w.cpu(), torch.float32)[1],
                1e-6, bf16_out=dtype == torch.bfloat16)
    worst.report()


# ----------------------------------------------------------------------------- bce_rows
BCE_VALUES = [0.0, 2.0 ** -10, -2.0 ** -10, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0]      # all exact in bf16


@pytest.mark.parametrize("rows,C", [(1, 1), (3, 40), (5, 64), (6, 65), (7, 130)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_bce_rows_widths_row_tails_and_saturated_logits(ops, dtype, rows, C):
    """C > 64: a lane takes a second and third class; rows % 4 != 0: the last waves of a workgroup have no row.  Logits
    where log1p(exp(-|x|)) is 0, 2^-10 and log 2; labels read directly and through an unsorted index with duplicates;
    sentinel rows behind ``rows`` in both outputs."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    worst = Worst(f"bce_rows {_ID(dtype)} rows={rows} C={C}")
    g = torch.Generator().manual_seed(3)
    vals = torch.tensor(BCE_VALUES + ([200.0, -200.0] if dtype == torch.float32 else []))
    assert torch.equal(vals.to(dtype).float(), vals)
    x = vals[torch.randint(0, len(vals), (rows * C,), generator=g)]
    x[0] = 0.0                                                                   # log1p(exp(0)) = log 2, sigmoid = 0.5
    if rows * C >= len(vals):
        x[torch.randperm(rows * C, generator=g)[:len(vals)]] = vals              # every value is there
    x = x.reshape(rows, C).to(dtype)
    table = (torch.rand(rows + 3, C, generator=g) < 0.5).to(torch.uint8)
    gr = torch.randn(rows, generator=g)
    gr[0] = -1.5
    gr[1 % rows] = 0.0 if rows > 1 else -1.5
    shuffled = torch.randperm(rows + 3, generator=g)[:rows]
    shuffled[rows // 2] = shuffled[0]                                            # a duplicate; not sorted
    for idx in (None, shuffled):
        lab = table[:rows] if idx is None else table[idx]
        assert rows * C == 1 or (bool(lab.any()) and not bool(lab.all()))
        ref = []
        for dt in (torch.float64, torch.float32):
            xr = x.detach().clone().to(dt).requires_grad_(True)
            per = F.binary_cross_entropy_with_logits(xr, lab.to(dt), reduction="none").sum(1)
            (per * gr.to(dt)).sum().backward()
            ref.append((per.detach(), xr.grad))
        xd, table_d, gr_d, idx_d = x.to(DEV), table.to(DEV), gr.to(DEV), None if idx is None else idx.to(DEV)
        out, dx = torch.full((rows + 2,), 12345.0, device=DEV), torch.full((rows + 2, C), 3.0, device=DEV).to(dtype)
        call("bevbert_bce_rows_fwd", ptr(xd), ptr(table_d), ptr(idx_d), ptr(out), rows, C, dtype_code(xd), stream())
        call("bevbert_bce_rows_bwd", ptr(xd), ptr(table_d), ptr(idx_d), ptr(gr_d), ptr(dx), rows, C, dtype_code(xd), stream())
        where = "idx NULL" if idx is None else "idx shuffled"
        assert bool((out[rows:] == 12345.0).all()) and bool((dx[rows:] == 3.0).all()), where
        worst.check("per_row", out[:rows], ref[0][0], ref[1][0], 1e-5, relative=True, where=where)
        worst.check("d_logits", dx[:rows], ref[0][1], ref[1][1], 1e-5, relative=True, bf16_out=dtype == torch.bfloat16, where=where)
    worst.report()


# ----------------------------------------------------------------------------- sem_select
def _mask(kind, n):
    m = torch.zeros(n, dtype=torch.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[-1] = 255                         # any non-zero byte counts
    elif kind == "alternating":
        m[::2] = 2
    return m


MASKS = ["none", "all", "first", "last", "alternating"]


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 2049])
def test_sem_select_equals_nonzero_at_every_size(ops, n):
    """n below, at and above one cell per thread (1024 threads), so threads with no cell and with a ragged last cell;
    capacities that cut the selection, fit it and exceed it; one mask and two.  idx, valid, denom and the padding zeros
    against torch.nonzero, exactly; sentinels behind ``cap`` stay."""
    from vln_bevbert_amd.lib import call, ptr, stream
    classes = 40
    for k1 in MASKS:
        for k2 in [None] + MASKS:
            m1, m2 = _mask(k1, n).to(DEV), None if k2 is None else _mask(k2, n).to(DEV)
            both = (m1 != 0) if m2 is None else (m1 != 0) & (m2 != 0)
            nz = torch.nonzero(both).squeeze(1)
            count = int(nz.numel())
            for cap in (1, n, n + 7):
                idx = torch.full((cap + 3,), -7, dtype=torch.int64, device=DEV)
                valid = torch.full((cap + 3,), -7.0, device=DEV)
                denom = torch.full((2,), -7.0, device=DEV)
                call("bevbert_sem_select", ptr(m1), ptr(m2), n, cap, classes, ptr(idx), ptr(valid), ptr(denom), stream())
                kept = min(count, cap)
                want_idx = torch.full((cap + 3,), -7, dtype=torch.int64, device=DEV)
                want_idx[:cap] = 0
                want_idx[:kept] = nz[:kept]
                want_valid = torch.full((cap + 3,), -7.0, device=DEV)
                want_valid[:cap] = (torch.arange(cap, device=DEV) < kept).float()
                assert torch.equal(idx, want_idx), (k1, k2, cap)
                assert torch.equal(valid, want_valid), (k1, k2, cap)
                assert denom.tolist() == [float(count * classes), -7.0], (k1, k2, cap, denom)


# ----------------------------------------------------------------------------- weighted_mean
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4608])
def test_weighted_mean_forward_bound_and_exact_backward(ops, n):
    """One workgroup of 1024 threads: n below a wave, around one element per thread, several per thread.  Forward within
    the summation bound (n + 16) 2^-24 sum |w x| / |denom|; backward equal to w * float32(dout / denom), bit for bit."""
    g = torch.Generator().manual_seed(n)
    x = 3.0 * torch.randn(n, generator=g)
    wt = torch.rand(n, generator=g)
    wt[::3] = 0.0
    dout = 0.3
    worst = Worst(f"weighted_mean n={n}")
    for w in (None, wt):
        for denom in (37.5, -3.0, torch.tensor(13.0)):
            d32 = denom.clone() if torch.is_tensor(denom) else torch.tensor(denom, dtype=torch.float32)
            xd = x.clone().to(DEV).requires_grad_(True)
            out = ops.weighted_mean(xd, None if w is None else w.to(DEV), denom.to(DEV) if torch.is_tensor(denom) else denom)
            (out * dout).backward()
            wx = x.double() if w is None else w.double() * x.double()
            want = wx.sum() / d32.double()
            ref32 = (x if w is None else w * x).sum() / d32
            bound = (n + 16) * U24 * float(wx.abs().sum()) / abs(float(d32))
            err = abs(float(out.detach()) - float(want))
            where = f"w {'NULL' if w is None else 'given'} denom {'device' if torch.is_tensor(denom) else denom}"
            row = worst.rows.get("mean")
            if row is None or err > row[0]:
                worst.rows["mean"] = (err, abs(float(ref32) - float(want)), bound, where)
            assert err <= bound, (where, err, bound)
            want_dx = (torch.ones(n) if w is None else w) * (torch.tensor(dout, dtype=torch.float32) / d32)
            assert torch.equal(xd.grad.cpu(), want_dx), where
    worst.report()


# ----------------------------------------------------------------------------- colsum_any
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_colsum_any_narrow_branch_and_unroll_tails(ops, dtype):
    """C <= 4: one workgroup walks the rows; wider: 64 columns x 4 row groups with a 16-row unroll and its tail (rows
    1 .. 29 hit every remainder, 300 the unrolled body), column counts around one and two workgroups.  Overwrite and
    accumulate, against fp64 within the summation bound; equal bits twice; nothing written behind C; rows = 0 with
    accumulate leaves ``out`` alone."""
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    g = torch.Generator(device=DEV).manual_seed(11)
    worst = Worst(f"colsum_any {_ID(dtype)}")
    for rows in (1, 3, 4, 5, 13, 16, 17, 29, 300):
        for C in (1, 2, 3, 4, 5, 63, 64, 65, 130):
            dy = torch.randn(rows, C, generator=g, device=DEV).to(dtype)
            before = torch.randn(C + 2, generator=g, device=DEV)
            sums, mags = dy.double().sum(0), dy.double().abs().sum(0)
            for accumulate in (0, 1):
                want = sums + before[:C].double() if accumulate else sums
                runs = []
                for _ in range(2):
                    out = before.clone()
                    if not accumulate:
                        out[:C] = float("nan")                                  # overwritten, never read
                    call("bevbert_colsum_any", ptr(dy), ptr(out), rows, C, dtype_code(dy), accumulate, stream())
                    runs.append(out)
                where = f"rows={rows} C={C} accumulate={accumulate}"
                assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0][C:], before[C:]), where
                err, bound = (runs[0][:C].double() - want).abs(), (rows + 4) * U24 * mags + U24 * want.abs()
                ratio = float((err / bound.clamp_min(1e-300)).max())
                row = worst.rows.get("colsum")
                if row is None or ratio > row[3]:
                    e32 = (dy.float().sum(0) + (before[:C] if accumulate else 0.0)).double() - want
                    k = int((err / bound.clamp_min(1e-300)).argmax())
                    worst.rows["colsum"] = (float(err[k]), float(e32.abs()[k]), float(bound[k]), ratio, where)
                assert bool((err <= bound).all()), (where, err, bound)
    e, e32, b, _, where = worst.rows["colsum"]
    worst.rows["colsum"] = (e, e32, b, where + " (the case nearest its bound)")
    worst.report()
    out = before.clone()
    call("bevbert_colsum_any", ptr(dy), ptr(out), 0, 130, dtype_code(dy), 1, stream())
    torch.cuda.synchronize()
    assert torch.equal(out, before)
