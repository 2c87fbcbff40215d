"""ParamArena.clip_and_step on the MI355X against the float64 reference of tests/optimizer_ref.py: sumsq_kernel,
clip_coef_kernel and adamw_kernel (csrc/optimizer.hip) with the moments compared, not only the parameters.

The probe arena (optimizer_ref.PROBE, 2.12 M elements) has tensors on both sides of the 1024-element chunk edge, two
packed groups, the three no-decay name patterns, a tensor first touched at step 3, one touched once and then stepped on
zeros, one never touched, and a tensor that takes sumsq_kernel's grid into a ragged third pass.  Three scenarios of six
steps (optimizer_ref.SCENARIOS): S1 the workload's settings with a bf16 shadow and steps on both sides of the clip, S2
an fp32 arena with torch's default betas and a pre-scale, S3 the device-resident learning rate.

Gates (tests/test_optimizer_host.py shows that the inputs tell thirteen wrong variants from the right computation by
ten times these):

* norm: relative 1e-5 (a thread adds at most three float4 sums of squares, eight folding levels and a double-precision
  fold follow: about twenty roundings of 6e-8);
* multiplier: relative 2e-5 on a clipped step, exactly float32(pre_scale) on an unclipped one;
* moments (max error over the tensor's max magnitude) and displacement (relative L2 of p - p0): max(4 x e32, floor)
  per tensor and step, e32 being the distance of the fp32 CPU reference from the float64 one at that step or a later
  one; floors 5e-5 and 2e-4.  Per tensor because c.weight at a p0 scale of 2^-6 moves by lr * 3e-4 a step, less than
  the spacing of fp32 numbers at |p| (e32 0.25 at step 1, 0.05 at step 6), and head.bias is made to stand still (e32
  1: optimizer_ref.PROBE says what for); one gate per scenario would be that wide for every tensor.  Where the worst
  measured value lies more than ten times below the gate, the gate is TIGHT, four times the measured value;
* step counters, untouched tensors, padding and the bf16 shadow: exact.

Measured on the MI355X, worst over tensors and steps:

    quantity        S1                   S2                   S3                   gate
    norm            1.0e-7               5.9e-8               2.9e-8               1e-5
    multiplier      9.1e-8               (never clips)        5.8e-8               2e-5
    exp_avg         3.4e-7               3.3e-7               4.5e-7               5e-5 -> TIGHT
    exp_avg_sq      1.2e-6               1.3e-5               1.2e-6               5e-5 -> TIGHT in S1, S3
    displacement    7.0e-5 (b.weight)    7.4e-5 (bias_table)  8.4e-5 (enc.value)   2e-4 where e32 < 5e-5
      c.weight      0.245 .. 0.051       3.9e-4 .. 6.7e-5     0.222 .. 0.038       4 x e32 (step 1 .. step 6)
      head.bias     1.0 (stands still)   0.14 .. 9.0e-3       1.0 (stands still)   4 x e32
    norm at size    norm 1.9e-8, multiplier 4.2e-8, the same bits twice            1e-5, 2e-5

c.weight in S1 and S3 is at e32 itself, to four digits, at every step: there the kernel rounds p as the fp32 CPU
reference does.

S2's exp_avg_sq: the kernel forms 1 - beta2 in fp32 from float32(0.999), which is 1.3e-5 below the reference's
float32(1 - 0.999).  The same factor is in the kernel's bias correction, so the parameters do not see it.

Step size alone: step_size / lr recovered from one step of a zero parameter against sqrt(1 - beta2^t) / (1 - beta1^t)
in Python doubles, gate 1e-5.  Measured relative error:

    betas          t = 1     2         3         10        100       1000      100000
    (0.9, 0.98)    7.4e-7    8.3e-7    3.3e-7    5.2e-7    1.1e-7    7.0e-8    6.7e-8
    (0.9, 0.999)   6.65e-6   9.97e-6   3.35e-6   6.75e-6   6.16e-6   3.70e-6   5.5e-8

Inside the gate, at (0.9, 0.999) and t = 2 by 0.3 %.  Of these figures 6.5e-6 is not the kernel's power: float32(0.999)
is 1.3e-8 above 0.999, so 1 - beta2^t is 1.3e-5 smaller than in doubles while t (1 - beta2) << 1, and its root 6.5e-6.
A bias correction formed as -expm1f(t ln beta) measures 6.6e-6 at every t <= 100 (6.65, 6.58, 6.59, 6.55, 6.07e-6): the
rest, up to 3.4e-6, is the error of 1 - exp2(t log2 beta) on the transcendental unit, a tenth of what one ulp of the
power would give.  adamw_kernel is unchanged.
"""
import math

import pytest
import torch

from tests import optimizer_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

# 4 x the worst moment error measured on the device (see the table above), where that is more than ten times below the
# gate.  Not S2's exp_avg_sq: 1.3e-5 is a quarter of its gate (the kernel forms 1 - beta2 in fp32 from float32(0.999),
# 1.3e-5 below float32(1 - 0.999) of the reference; the same factor is in its bias correction, so p does not see it).
TIGHT = {("S1", "m"): 1.4e-6, ("S1", "v"): 4.9e-6, ("S2", "m"): 1.4e-6, ("S3", "m"): 1.8e-6, ("S3", "v"): 4.7e-6}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vln_bevbert_amd import lib, ops as _ops
    lib.load()          # raises (does not skip) when the HIP library is missing on a GPU box
    return _ops


def _arena(p0, shadow):
    from vln_bevbert_amd.arena import ParamArena
    module = O.build_probe(p0)
    arena = ParamArena(module, DEV, torch.bfloat16 if shadow else torch.float32, groups=O.GROUPS)
    return arena, dict(module.named_parameters())


def _chunks(arena, name):
    o, k = arena.slices[name]
    return slice(o // O.CHUNK, (o + k - 1) // O.CHUNK + 1)


def _padding_mask(arena):
    pad = torch.ones(arena.numel, dtype=torch.bool)
    for o, k in arena.slices.values():
        pad[o:o + k] = False
    return pad


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("scenario", list(O.SCENARIOS))
def test_clip_and_step_matches_float64_reference(ops, scenario):
    sc = O.SCENARIOS[scenario]
    p0, grads = O.make_inputs(scenario)
    arena, params = _arena(p0, sc["shadow"])
    assert (arena.shadow is not None) == sc["shadow"]
    gate = O.gates(scenario, arena.slices)
    pad = _padding_mask(arena)
    assert int(pad.sum()) > 0 and not bool(pad[-4:].any())
    start = {x: getattr(arena, x).cpu().clone() for x in (("params", "shadow") if sc["shadow"] else ("params",))}
    kw = dict(betas=sc["betas"], eps=sc["eps"], weight_decay=sc["wd"], max_norm=sc["max_norm"],
              grad_pre_scale=sc["pre_scale"])
    if sc["device_lr"]:
        with pytest.raises(RuntimeError, match="set_lr"):
            arena.clip_and_step(None, **kw)
    worst = {q: (0.0, 0.0, None) for q in ("m", "v", "disp", "norm", "mult")}     # (error / gate, error, where)
    worst_abs = {q: (0.0, None) for q in worst}
    failures, clipped = [], []

    def check(q, err, bound, where):
        if err > worst_abs[q][0]:
            worst_abs[q] = (err, where)
        if err / bound > worst[q][0]:
            worst[q] = (err / bound, err, where)
        if not err <= bound:
            failures.append(f"{where}: {q} error {err:.3e} > {bound:.3e}")

    for k, state, norm, mult in O.run(scenario, arena.slices):
        arena.zero_grad()
        assert int(torch.count_nonzero(arena.grads)) == 0 and float(arena.grads[-1]) == 0.0
        for n, g in grads[k].items():
            if g is not None:
                params[n].main_grad.copy_(g.to(DEV))
                arena.touch(params[n])
        if sc["device_lr"]:
            arena.set_lr(O.lr_at(scenario, k))
            arena.clip_and_step(None, **kw)
        else:
            arena.clip_and_step(O.lr_at(scenario, k), **kw)
        got = {x: getattr(arena, x).cpu() for x in ("params", "exp_avg", "exp_avg_sq")}
        steps = arena.chunk_steps.cpu()
        shadow = arena.shadow.cpu() if sc["shadow"] else None
        where = f"{scenario} step {k + 1}"
        # norm and multiplier
        check("norm", abs(float(arena.grad_norm()) - norm) / norm, O.NORM_GATE, where)
        got_mult = float(arena._scalars[1])
        clipped.append(mult < sc["pre_scale"])
        if clipped[-1]:
            check("mult", abs(got_mult - mult) / mult, O.MULT_GATE, where)
        else:
            assert got_mult == float(torch.tensor(sc["pre_scale"], dtype=torch.float32)), (where, got_mult)
        # padding between tensors stays 0
        for x in got:
            assert int(torch.count_nonzero(got[x][pad])) == 0, f"{where}: padding of {x} was written"
        for n in O.NAMES:
            o, cnt = arena.slices[n]
            ch = _chunks(arena, n)
            want = state[n]
            assert steps[ch].tolist() == [want["step"]] * (ch.stop - ch.start), (where, n, steps[ch].tolist())
            if want["step"] == 0:                                 # never touched (so far): bit for bit as built
                assert torch.equal(_bits(got["params"][o:o + cnt]), _bits(start["params"][o:o + cnt])), (where, n)
                assert int(torch.count_nonzero(got["exp_avg"][o:o + cnt])) == 0, (where, n)
                assert int(torch.count_nonzero(got["exp_avg_sq"][o:o + cnt])) == 0, (where, n)
                if shadow is not None:
                    assert torch.equal(_bits(shadow[o:o + cnt]), _bits(start["shadow"][o:o + cnt])), (where, n)
                continue
            err = O.tensor_errors({"p": got["params"][o:o + cnt], "m": got["exp_avg"][o:o + cnt],
                                   "v": got["exp_avg_sq"][o:o + cnt]}, want, p0[n])
            if n in ("c.weight", "head.bias"):
                print(f"MEASURED {where} {n} disp {err['disp']:.3e} (gate {gate[n][k]['disp']:.3e})")
            for q, e in err.items():
                check(q, e, min(gate[n][k][q], TIGHT.get((scenario, q), math.inf)), f"{where} {n}")
            if shadow is not None:                                # every touched chunk, its padding included
                a, b = ch.start * O.CHUNK, ch.stop * O.CHUNK
                assert torch.equal(_bits(shadow[a:b]), _bits(got["params"][a:b].to(torch.bfloat16))), (where, n)
    for q, (ratio, err, at) in worst.items():
        print(f"MEASURED {scenario} {q:5s} closest to its gate: error {err:.3e} = {ratio:.3f} x gate ({at}); "
              f"largest error {worst_abs[q][0]:.3e} ({worst_abs[q][1]})")
    if sc["max_norm"] is not None:
        assert any(clipped) and not all(clipped), clipped       # both branches of the clip were run
    assert not failures, failures


def test_grad_norm_at_size(ops):
    """The norm alone over the whole arena, padding included: magnitudes from 1e-4 to 1e2 and three dominant values
    where a short loop would miss them."""
    p0, _ = O.make_inputs("S2")
    arena, params = _arena(p0, False)
    n = arena.numel
    g = torch.Generator().manual_seed(7)
    vals = 10.0 ** (torch.rand(n, generator=g) * 6.0 - 4.0) * (torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0)
    o, cnt = arena.slices["enc.value.weight"]
    spots = {n - 2: 5e4, O.SUMSQ_PASS + 1: -4e4, o + cnt - 3: 3e4}
    for i, x in spots.items():
        vals[i] = x
    vals = vals.float()
    total = float((vals.double() ** 2).sum())
    for i, x in spots.items():                                   # each one alone moves the norm by far more than the gate
        assert x * x / total > 0.1
    arena.grads.copy_(vals.to(DEV))
    pre, max_norm = 0.25, 5.0
    norm = pre * math.sqrt(total)
    mult = pre * min(1.0, max_norm / (norm + 1e-6))
    before = arena.params.clone()
    out = []
    for _ in range(2):
        arena.clip_and_step(0.0, max_norm=max_norm, grad_pre_scale=pre)
        out.append(arena._scalars[:2].cpu().clone())
    e_norm, e_mult = abs(float(out[0][0]) - norm) / norm, abs(float(out[0][1]) - mult) / mult
    print(f"MEASURED norm at size: norm {e_norm:.3e} multiplier {e_mult:.3e}")
    assert e_norm <= O.NORM_GATE and e_mult <= O.MULT_GATE, (e_norm, e_mult)
    assert torch.equal(_bits(out[0]), _bits(out[1]))
    assert torch.equal(arena.params, before)                     # nothing was touched: lr = 0 and no flag set


STEP_TS = (1, 2, 3, 10, 100, 1000, 100000)


@pytest.mark.parametrize("t", STEP_TS)
@pytest.mark.parametrize("betas", [(0.9, 0.98), (0.9, 0.999)])
def test_step_size_bias_correction(ops, betas, t):
    """step_size / lr = sqrt(1 - beta2^t) / (1 - beta1^t), recovered from one step of a zero parameter.

    The margin at (0.9, 0.999), t = 2 is 3e-8 (9.97e-6 against 1e-5), and it is left so: the gate and the reference in
    doubles are what this test is for, and 6.5e-6 of the figure is the C ABI taking the betas as float (module
    docstring).  The kernel uses float32(beta) in the moments and in the bias correction alike, so the parameters do
    not carry that part.  Forming only the bias correction from the double betas would bring this figure down and make
    the step itself wrong by the same 6.5e-6; the remedy, if a toolchain change moves sqrtf or the division by an ulp
    and this case goes red, is to pass beta, 1 - beta and ln beta to the launcher as doubles, which also removes the
    1.3e-5 of S2's exp_avg_sq and changes low-order bits of every trained parameter."""
    from vln_bevbert_amd.arena import ParamArena
    module = torch.nn.Module()
    module.register_parameter("weight", torch.nn.Parameter(torch.zeros(1024)))
    arena = ParamArena(module, DEV, torch.float32)
    lr, eps = 1e-3, 1e-8
    arena.grads.copy_(torch.randn(1024, generator=torch.Generator().manual_seed(t)).to(DEV))
    arena.touch(module.weight)
    arena.exp_avg = torch.zeros_like(arena.params)
    arena.exp_avg_sq = torch.zeros_like(arena.params)
    arena.chunk_steps.fill_(t - 1)
    arena.clip_and_step(lr, betas, eps, 0.0, max_norm=None)
    assert arena.chunk_steps.tolist() == [t]
    p, m, v = (x.cpu().double() for x in (arena.params, arena.exp_avg, arena.exp_avg_sq))
    got = float((-p / (lr * m / (v.sqrt() + eps))).mean())
    want = math.sqrt(1.0 - betas[1] ** t) / (1.0 - betas[0] ** t)
    err = abs(got - want) / want
    print(f"MEASURED step size betas {betas} t {t}: relative error {err:.3e}")
    assert err <= 1e-5, (got, want, err)


def _cast_patterns():
    """Every bf16 bit pattern in the upper half of an fp32 word, with the lower halves that are the ties and their two
    sides; padded to whole chunks."""
    hi = torch.arange(1 << 16, dtype=torch.int64)
    lo = torch.tensor([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)
    bits = ((hi[:, None] << 16) | lo[None, :]).reshape(-1)
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    n = (bits.numel() + O.CHUNK - 1) // O.CHUNK * O.CHUNK
    return torch.cat([bits, torch.zeros(n - bits.numel(), dtype=torch.int32)])


def _assert_cast(shadow, masters, what):
    """``shadow`` (bf16) against torch's CPU cast of ``masters`` (fp32): the same bits wherever the cast is a number,
    NaN where it is NaN."""
    want = masters.to(torch.bfloat16)
    nan = want.isnan()
    assert torch.equal(shadow.isnan(), nan), f"{what}: NaN pattern differs"
    bad = (_bits(shadow) != _bits(want)) & ~nan
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} casts differ, first at fp32 bits "
                             f"{int(_bits(masters)[i]) & 0xFFFFFFFF:#010x}: got {int(_bits(shadow)[i]) & 0xFFFF:#06x} "
                             f"want {int(_bits(want)[i]) & 0xFFFF:#06x}")


def test_shadow_cast_matches_torch(ops):
    """The fp32 -> bf16 cast of the shadow, through sync_shadow and through the AdamW pass, on every rounding case.

    The AdamW pass runs with lr = 0, wd = 0 and zero gradients, so p - 0 * (0 / eps) - 0 * p leaves every finite master
    at its value (-0 comes back as +0, an infinity as NaN: IEEE arithmetic of x - 0 * x); the shadow is compared with
    the cast of the masters as that pass left them."""
    from vln_bevbert_amd.arena import ParamArena
    bits = _cast_patterns()
    module = torch.nn.Module()
    module.register_parameter("weight", torch.nn.Parameter(torch.zeros(bits.numel())))
    arena = ParamArena(module, DEV, torch.bfloat16)
    masters = bits.view(torch.float32)
    _bits(arena.params).copy_(bits.to(DEV))
    arena.sync_shadow()
    assert torch.equal(_bits(arena.params.cpu()), bits)
    _assert_cast(arena.shadow.cpu(), masters, "sync_shadow")

    arena.shadow.zero_()
    arena.zero_grad()
    arena.touch(module.weight)
    arena.clip_and_step(0.0, (0.9, 0.98), 1e-6, 0.0, max_norm=None)
    after = arena.params.cpu()
    finite = masters.isfinite()
    assert torch.equal(after[finite], masters[finite]), "the AdamW pass moved a finite master"
    _assert_cast(arena.shadow.cpu(), after, "AdamW pass")
