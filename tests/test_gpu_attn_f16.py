"""csrc/attn_fwd2.hip with fp16 operands on the GPU: bevbert_attn_f16_fwd (through ops.attention_self / attention_cross / attention and
directly) per element against the fp64 softmax-attention of its fp16-rounded inputs, at every length where the kernel's tiling
turns over (tests/attn_f16_cases.py: inputs, bound and case list; tests/test_clip_vit_f16_host.py holds the bound against a
CPU emulation of the kernel's arithmetic and against one wrong key at a tile edge).

    |o - o64| <= C16 * 2^-11 * sum_j p_ij |v_jd| + half an fp16 ulp of o64,   C16 = 4

Every case also runs the entry with o as a strided view of a larger sentinel-filled buffer (rows beyond Lq, columns between
the rows, a batch gap): the bytes outside the view stay, the bytes inside repeat the first launch bit for bit.

Run with -s for one line per case ("attn-f16-edge-errors:"): the units of 2^-11 b_o the case needed, output rounding taken
off; the figures also go to the suite's error log (tests.test_gpu_model._record, kind "attn_f16_edge"), and
profiles/attn_f16_edge_errors.txt holds those lines from the MI355X."""
import ctypes
import math

import pytest
import torch

from tests import attn_f16_cases as AC
from tests.test_gpu_model import _record               # the suite's log of achieved errors
from vln_bevbert_amd import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAG = "attn-f16-edge-errors:"


def _log(line, what=None, units=None):
    print(TAG, line)
    if what is not None:
        _record("attn_f16_edge", what, units=units, c16=AC.C16)


@pytest.fixture(scope="module")
def worst():
    book = {}
    yield book
    if book:
        name = max(book, key=book.get)
        _log(f"worst of {len(book)} cases: {book[name]:.3f} of C16 = {AC.C16} units at {name}", f"worst:{name}", book[name])


_REF = {}


def _ref(Lq, Lk, nh):
    """(q, k, v, o64, b_o, floor) of a shape: computed once, shared by the packed and the separate case, never written to."""
    if (Lq, Lk, nh) not in _REF:
        q, k, v = AC.make_inputs(Lq, Lk, nh)
        _REF[(Lq, Lk, nh)] = (q, k, v) + AC.reference64(q, k, v)
    return _REF[(Lq, Lk, nh)]


def _strides(q, k, v, o):
    return (ctypes.c_int64 * 8)(q.stride(1), k.stride(1), v.stride(1), o.stride(1), q.stride(0), k.stride(0), v.stride(0),
                                o.stride(0))


def _entry(q, k, v, o, nh, head_dim=AC.D):
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    return lib.load().bevbert_attn_f16_fwd(lib.ptr(q), lib.ptr(k), lib.ptr(v), lib.ptr(o), _strides(q, k, v, o), B, nh, Lq, Lk,
                                           head_dim, AC.SCALE, lib.stream())


@pytest.mark.parametrize("case", AC.cases(), ids=AC.case_id)
def test_f16_attention_against_fp64_per_element(case, worst):
    Lq, Lk, nh, packed = case
    q, k, v, o64, b_o, floor = _ref(Lq, Lk, nh)
    assert floor >= AC.P_FLOOR, "the bound has no flush term: every probability must be a normal fp16 number"
    H = nh * AC.D
    if packed and Lq == Lk:
        qkv = torch.cat([q, k, v], -1).to(DEV)
        dq, dk, dv = qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:]
        o = ops.attention_self(qkv, None, None, nh)
    elif packed:
        dq, kv = q.to(DEV), torch.cat([k, v], -1).to(DEV)
        dk, dv = kv[..., :H], kv[..., H:]
        o = ops.attention_cross(dq, kv, None, nh)
    else:
        dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
        o = ops.attention(dq, dk, dv, nh=nh)
    assert o.dtype == torch.float16 and o.shape == (AC.B, Lq, H) and o.is_contiguous()
    got = o.cpu()
    need = AC.units(got, o64, b_o)
    _log(f"case {AC.case_id(case)} o={need:.3f}", AC.case_id(case), need)
    worst[AC.case_id(case)] = need
    assert bool(torch.isfinite(got).all())
    over = (got.double() - o64).abs() - AC.bound(o64, b_o)
    assert float(over.max()) <= 0.0, f"{AC.case_id(case)}: {int((over > 0).sum())} elements outside the bound, needs {need:.2f} units"
    # the entry itself, o a strided view inside a sentinel-filled buffer: two more rows per batch, 16 more columns per row
    pad_rows, pad_cols = 2, 16
    buf = torch.full((AC.B, Lq + pad_rows, H + pad_cols), -1234.0, dtype=torch.float16, device=DEV)
    view = buf[:, :Lq, :H]
    assert _entry(dq, dk, dv, view, nh) == 0, lib.load().bevbert_last_error().decode()
    assert torch.equal(view.view(torch.int16), o.view(torch.int16)), "two launches differ"
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[:, :Lq, :H] = False
    assert bool((buf[outside] == -1234.0).all()), "a store outside the rows and columns of o"


def test_entry_refuses_bad_arguments_before_any_launch():
    l = lib.load()
    q, k, v = (t.to(DEV) for t in AC.make_inputs(16, 16, 2))
    o = torch.full_like(q, -1234.0)
    st = _strides(q, k, v, o)

    def call(qp, kp, vp, op, sp, Lq=16, Lk=16, head_dim=64):
        return l.bevbert_attn_f16_fwd(qp, kp, vp, op, sp, 2, 2, Lq, Lk, head_dim, AC.SCALE, lib.stream())
    ptrs = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr())
    for bad, word in ((dict(head_dim=32), "head_dim"), (dict(head_dim=128), "head_dim"), (dict(Lq=0), "empty"),
                      (dict(Lk=0), "empty"), (dict(Lq=-3), "empty")):
        assert call(*ptrs, st, **bad) == -1 and word in l.bevbert_last_error().decode(), bad
    for i in range(4):
        assert call(*[None if j == i else p for j, p in enumerate(ptrs)], st) == -1
        assert "NULL" in l.bevbert_last_error().decode()
    assert call(*ptrs, None) == -1 and "NULL" in l.bevbert_last_error().decode()
    assert call(ptrs[0] + 2, *ptrs[1:], st) == -1 and "aligned" in l.bevbert_last_error().decode()
    odd = (ctypes.c_int64 * 8)(*[132 if i == 3 else x for i, x in enumerate(st)])
    assert call(*ptrs, odd) == -1 and "aligned" in l.bevbert_last_error().decode()
    torch.cuda.synchronize()
    assert bool((o == -1234.0).all()), "a refused call launched"
    assert call(*ptrs, st) == 0


def test_python_side_refuses_what_the_f16_kernel_does_not_do():
    """float16 goes to the inference kernel or nowhere: mask, bias, dropout, gradients and mixed dtypes raise in Python, and the
    general entries keep rejecting dtype 2."""
    q, k, v = (t.to(DEV) for t in AC.make_inputs(17, 17, 2))
    qkv = torch.cat([q, k, v], -1)
    mask = torch.zeros(AC.B, 17, device=DEV)
    with pytest.raises(ValueError, match="key mask"):
        ops.attention_self(qkv, mask, None, 2)
    with pytest.raises(ValueError, match="bias"):
        ops.attention(q, k, v, bias=torch.zeros(AC.B, 17, 17, device=DEV), nh=2)
    with pytest.raises(ValueError, match="dropout"):
        ops.attention_self(qkv, None, None, 2, drop_p=0.1, training=True)
    with pytest.raises(ValueError, match="backward"):
        ops.attention_self(qkv.clone().requires_grad_(True), None, None, 2)
    with pytest.raises(ValueError, match="float16"):
        ops.attention(q, k.bfloat16(), v, nh=2)
    with pytest.raises(ValueError, match="float16"):
        ops.attention_cross(q.float(), torch.cat([k, v], -1), None, 2)
    with pytest.raises(ValueError, match="nh"):
        ops.attention_self(qkv, None, None, 3)
    with torch.no_grad():                                      # what does work: eval-mode dropout, no_grad over a leaf
        a = ops.attention_self(qkv.clone().requires_grad_(True), None, None, 2, drop_p=0.1, training=False)
    assert a.dtype == torch.float16 and not a.requires_grad
    o = torch.empty_like(q)
    rc = lib.load().bevbert_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, None, None,
                                     _strides(q, k, v, o), AC.B, 2, 17, 17, 64, 1 / math.sqrt(64), lib.F16, 0, 0.0, 0, 0, None, 0,
                                     lib.stream())
    assert rc != 0 and "dtype 2 unsupported" in lib.load().bevbert_last_error().decode()
