"""Every attention kernel of the dispatch (csrc/capi.hip: 16 kernels) against the fp64 reference of tests/attn_cases.py, per
element, at the lengths where its launcher switches tile counts or forms and at the lengths one off them, with key masks
that have holes, a graph bias and dropout under the exported keep mask.

The calls go through the C ABI (bevbert_attn_fwd / bevbert_attn_bwd / bevbert_attn_drop_bits), so that the kernel each call was
dispatched to is readable on this thread and the per-head dbias is visible; both recorded paths must be the ones the case
names (tests/test_attn_refs_host.py holds the same table to bevbert_attn_plan without a device).

Gates (attn_cases.gates; all elementwise, none comes from the code under test):
  bf16 MFMA kernels   |got - want| <= C16 2^-8 b_x + 2^-8 |want|   for o, dq, dk, dv;  dbias (fp32): C16 2^-8 b_dbias
  fp32 kernels        |got - want| <= C32 2^-24 b_x;   exact kernels on bf16 storage: the same + 2^-8 |want|
  lse                 |got - want| <= 2^-18 b_lse
with b_o = Pd |V|, b_dv = Pd^T |do|, e_S = P (keep / (1 - p) |dPd| + |delta| + sum_d |o||do|), b_dq = scale e_S |K|,
b_dk = scale e_S^T |Q|, b_dbias = e_S, b_lse = 1 + max over the row's unmasked keys of scale sum_d |q_d||k_d|.  The host test
shows that a bf16 restatement needs C16 / 4 of these at the most, that C32 is four times what torch's fp32 composition needs,
and that one dropped, mis-masked, mis-dropped or misplaced key at a tile edge leaves the bf16 gates by more than a factor 2.
Measured on the MI355X: the MFMA kernels need 0.90 of C16's units at the most, the fp32 kernels 40.8 of C32's.

Run with -s for one line per kernel and quantity ("attn-edge-errors:", profiles/attn_edge_errors.txt): the element nearest
its bound over all cases of the kernel, and "<quantity> units", the largest error in units of 2^-8 b_x (2^-24 b_x for the
exact kernels; output rounding taken off) against C16 / C32."""
import functools
import time

import pytest
import torch

from tests import attn_cases as ac
from tests.kernel_gates import Worst as _Worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
Worst = functools.partial(_Worst, prefix="attn-edge-errors:")
SEED = 11
FWD_Q, BWD_Q = ("o", "lse"), ("dq", "dk", "dv", "dbias")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def per_kernel():
    """Worst per kernel over the cases of this module; printed when the module is done."""
    book, t0 = {}, time.perf_counter()
    yield book
    for name in sorted(book):
        book[name].report()
    print(f"attn-edge-errors: module wall time {time.perf_counter() - t0:.1f} s")


def _set_knobs(monkeypatch, knobs):
    for name in ac.ATTN_KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)


def _run(ops, c, q, k, v, do, km, bias):
    """One forward + backward call on the device under the knobs the environment holds; every output starts as NaN.  Returns
    the outputs on the CPU, the exported keep mask (or None) and the two recorded paths."""
    from vln_bevbert_amd import lib
    from vln_bevbert_amd.lib import call, dtype_code, ptr, stream
    L = lib.load()
    B, nh, Lq, Lk = q.shape[0], c.nh, q.shape[1], k.shape[1]
    nan = float("nan")
    q, k, v, do = (t.to(DEV).contiguous() for t in (q, k, v, do))
    km = None if km is None else km.to(DEV).contiguous()
    bias = None if bias is None else bias.to(DEV).contiguous()
    ops.RT.new_step(4321)
    bits, ready = None, 0
    if c.bits != "none":
        bits = torch.zeros(ops._drop_bits_words(B, nh, Lq, Lk), dtype=torch.int64, device=DEV)
    if c.bits == "ready":
        call("bevbert_attn_drop_bits", ptr(bits), B, nh, Lq, Lk, c.p, SEED, 0, stream())
        ready = 1
    o = torch.full_like(q, nan)
    lse = torch.full((B, nh, Lq), nan, device=DEV)
    st = ops._strides(q, k, v, o)
    call("bevbert_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(km), ptr(bias), st, B, nh, Lq, Lk, ac.D, ac.SCALE,
         dtype_code(q), c.impl, c.p, SEED, 0, ptr(bits), ready, stream())
    dq, dk, dv = torch.full_like(q, nan), torch.full_like(k, nan), torch.full_like(v, nan)
    dbias = torch.full((B, nh, Lq, Lk), nan, device=DEV) if c.bias else None
    delta = torch.empty_like(lse)
    call("bevbert_attn_bwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv),
         ptr(dbias), ptr(km), ptr(bias), st, B, nh, Lq, Lk, ac.D, ac.SCALE, dtype_code(q), c.impl, c.p, SEED, 0, ptr(bits), stream())
    paths = (L.bevbert_attn_last_path(0).decode(), L.bevbert_attn_last_path(1).decode())
    keep = None
    if c.p > 0:
        Lk2 = (Lk + 1) // 2 * 2            # the kernels index dropout elements with the key count rounded up to even
        keep = ops.dropout_keep_mask(B * nh * Lq * Lk2, c.p, SEED, 0, DEV).view(B, nh, Lq, Lk2)[..., :Lk].cpu()
    torch.cuda.synchronize()
    got = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "dbias": dbias}
    return {n: (None if t is None else t.cpu()) for n, t in got.items()}, keep, paths


@pytest.mark.parametrize("c", ac.CASES, ids=ac.case_id)
def test_attention_kernel_against_fp64_at_its_tile_edges(ops, per_kernel, c, monkeypatch):
    _set_knobs(monkeypatch, c.knobs)
    q, k, v, do, km, bias = ac.make_inputs(c.B, c.nh, c.Lq, c.Lk, ac.TORCH_DTYPE[c.dtype], c.mask, c.bias, seed=ac.CASES.index(c))
    got, keep, paths = _run(ops, c, q, k, v, do, km, bias)
    assert paths == (c.fwd, c.bwd), paths
    ref = ac.reference(q, k, v, do, ac.SCALE, km, bias, keep, c.p)
    kind = ac.gate_kind(c)
    gate = ac.gates(ref, kind)
    where = f"{c.Lq}x{c.Lk} {c.mask} p={c.p}"
    # every element overwritten (a partial last tile skips no row) and finite
    for name, t in got.items():
        assert t is None or bool(torch.isfinite(t.float()).all()), (name, "elements left or not finite",
                                                                    int((~torch.isfinite(t.float())).sum()))
    if c.mask == "holes_inf":
        masked = torch.isinf(km)
        assert bool((got["dk"][masked] == 0).all()) and bool((got["dv"][masked] == 0).all())
    case_units = ac.units(got, ref, kind)
    print("attn-edge-errors: case", ac.case_id(c), " ".join(f"{n}={u:.3f}" for n, u in case_units.items()))
    failures = []
    for kernel, names in ((c.fwd, FWD_Q), (c.bwd, BWD_Q)):
        worst = per_kernel.setdefault(kernel, Worst(kernel))
        for name in names:
            if got[name] is None:
                continue
            if name != "lse":
                worst.note(name + " units", case_units[name], ac.C32 if kind != "bf16" else ac.C16, where)
            try:
                worst.bound(name, got[name], ref[name], gate[name], where)
            except AssertionError as e:             # every quantity of the case is measured before the case fails
                failures.append(e.args[0])
    assert not failures, failures


# ----------------------------------------------------------------------------- samples do not see each other
FAMILIES = [
    ac._c(80, 81, "holes_inf", 0.1, "short_fwd", "short_bwd", B=3),
    ac._c(97, 49, "holes", 0.1, "small_fwd", "small_bwd", ac.SMALL1, B=3),
    ac._c(49, 81, "holes_inf", 0.1, "mfma_fwd", "small_bwd2", ac.SHORT0, B=3),
    ac._c(129, 129, "holes", 0.1, "fwd2", "mfma_bwd1", bits="ready", B=3),
    ac._c(65, 320, "holes_inf", 0.1, "fwd2", "bwd3", B=3),
    ac._c(65, 320, "holes", 0.1, "fwd2", "bwd2", ac.BWD3_0, B=3),
    ac._c(449, 320, "holes_inf", 0.1, "fwd4", "bwd3", ac._fwd4(3), B=3),
    ac._c(64, 129, "holes", 0.1, "mfma_fwd", "mfma_bwd", bias=True, B=3),
    ac._c(65, 65, "holes_inf", 0.1, "mfma_fwd", "mfma_bwd1", bias=True, B=3),
    ac._c(33, 513, "holes", 0.0, "fwd2", "mfma_bwd", B=3),
    ac._c(65, 129, "holes_inf", 0.1, "f32_fwd", "f32_bwd", dtype="f32", impl=0, B=3),
    ac._c(65, 65, "holes", 0.1, "simple_fwd", "simple_bwd", ac.SIMPLE, dtype="f32", impl=0, B=3),
    ac._c(65, 65, "holes_inf", 0.1, "simple_fwd", "simple_bwd", impl=1, B=3),
]


@pytest.mark.parametrize("c", FAMILIES, ids=ac.case_id)
def test_attention_samples_do_not_see_each_other(ops, c, monkeypatch):
    """B = 3 with per-sample masks.  New k and v values at sample 1's masked keys change nothing anywhere but sample 1's dk
    and dv rows (a masked key has weight exactly 0, and key 0 is never masked, so no running maximum starts from one); a new
    mask pattern for sample 1 leaves every output of samples 0 and 2 bit-identical."""
    _set_knobs(monkeypatch, c.knobs)
    q, k, v, do, km, bias = ac.make_inputs(c.B, c.nh, c.Lq, c.Lk, ac.TORCH_DTYPE[c.dtype], c.mask, c.bias, seed=77)
    base, _, paths = _run(ops, c, q, k, v, do, km, bias)
    assert paths == (c.fwd, c.bwd), paths
    g = torch.Generator().manual_seed(5)
    masked = km[1] != 0
    assert 0 < int(masked.sum()) < c.Lk
    k2, v2 = k.clone(), v.clone()
    k2[1, masked] = (3.0 * torch.randn(int(masked.sum()), k.shape[-1], generator=g)).to(k.dtype)
    v2[1, masked] = (3.0 * torch.randn(int(masked.sum()), v.shape[-1], generator=g)).to(v.dtype)
    values, _, _ = _run(ops, c, q, k2, v2, do, km, bias)
    for name in ("o", "lse", "dq") + (("dbias",) if c.bias else ()):
        assert torch.equal(values[name], base[name]), name
    for name in ("dk", "dv"):
        assert torch.equal(values[name][[0, 2]], base[name][[0, 2]]), name
        assert torch.equal(values[name][1, ~masked], base[name][1, ~masked]), name
    km2 = km.clone()
    flip = torch.rand(c.Lk, generator=g) < 0.5
    flip[0] = False
    km2[1] = torch.where(flip, torch.where(masked, torch.zeros(()), km[km != 0][0]), km[1])
    assert not torch.equal(km2[1], km[1]) and km2[1, 0] == 0
    pattern, _, _ = _run(ops, c, q, k, v, do, km2, bias)
    for name, t in pattern.items():
        if t is not None:
            assert torch.equal(t[[0, 2]], base[name][[0, 2]]), name
            assert not torch.equal(t[1], base[name][1]), name
