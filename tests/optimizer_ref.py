"""Plain float64 restatement of what ``ParamArena.clip_and_step`` has to compute, and the inputs the optimiser tests
share (tests/test_optimizer_host.py on the CPU, tests/test_gpu_optimizer_arena.py on the device).

``clip_and_step_ref`` restates, per call,

* ``torch.nn.utils.clip_grad_norm_``: norm of ``pre_scale * g`` over all tensors, ``coef = min(1, max_norm / (norm +
  1e-6))``, no clipping for ``max_norm=None``;
* ``oracle/bevbert_ref.py: adamw_step`` with the step count kept PER TENSOR;
* the reference's old-torch ``zero_grad`` semantics (tests/helpers.py: oracle_train): a tensor that has ever had a
  gradient is stepped on zeros afterwards, a never-touched tensor is skipped entirely;
* weight decay switched off by the substring rule of ``R.no_decay_key``.

``variant`` selects one deliberately wrong restatement (VARIANTS); only the host test uses it, to show that the shared
inputs tell every one of them from the right computation by ten times the gate of the quantity it moves.

``clip_and_step_f32`` is the reference in the precision it really runs in: ``R.adamw_step`` on float32 CPU tensors with
the norm as ``oracle_train`` forms it.  Its distance from the float64 run (``e32``) is the yardstick of the device gates.
"""
import functools
import math

import torch

from oracle import bevbert_ref as R

CHUNK = 1024
SUMSQ_PASS = 1024 * 256 * 4          # elements one pass of sumsq_kernel's grid covers
VARIANTS = ("eps_inside_sqrt", "no_sqrt_bc2", "global_step", "skip_when_no_grad", "decay_everywhere", "decay_nowhere",
            "coef_not_applied", "pre_scale_twice", "pre_scale_dropped", "no_clamp", "step_never_touched",
            "norm_first_pass_only", "norm_drops_last4")

# ---------------------------------------------------------------------------------------------- the probe module
# (name, shape, sigma of its gradients).  Names are chosen for their decay class; "late.weight" comes last so that the
# arena ends on real data (2048 elements: no padding behind it) and the norm's last float4 carries a gradient.
# c.weight at 1e-6: eps decides its update, and weight decay is half of its displacement.  head.bias at 1e-9: a tensor
# without decay that all but stands still (lr * 1.5e-7 a step after S1's clip, below what fp32 resolves at |p|: its
# displacement gate is 4 x e32 = 4), so that decay applied to it by mistake is thousands of times its displacement.
PROBE = [
    ("a.weight", (1,), 1.0), ("b.weight", (1023,), 1.0), ("c.weight", (1024,), 1e-6), ("d.weight", (1025,), 1e3),
    ("enc.query.weight", (32, 32), 1.0), ("enc.query.bias", (32,), 1.0),
    ("enc.key.weight", (32, 32), 1.0), ("enc.key.bias", (32,), 1.0),
    ("enc.value.weight", (32, 32), 1.0), ("enc.value.bias", (32,), 1.0),
    ("LayerNorm.weight", (768,), 1.0), ("head.bias", (5,), 1e-9), ("bias_table.weight", (300, 7), 1.0),
    ("once.weight", (1500,), 1.0), ("never.weight", (700,), 1.0), ("big.weight", (2_100_000,), 1.0),
    ("late.weight", (2048,), 1.0),
]
GROUPS = (["enc.query.weight", "enc.key.weight", "enc.value.weight"],
          ["enc.query.bias", "enc.key.bias", "enc.value.bias"])
NAMES = [n for n, _, _ in PROBE]
N_STEPS = 6
LATE_FIRST = 2                       # 0-based step of late.weight's first gradient (step 3)
LATE_SPIKE = 2e3                     # gradient of late.weight's last element: 4e-3 of the squared norm

# grad_scale: factor on every gradient of that step.  With d.weight at 1e3 * randn the norm is 3.2e4 * scale: a step at
# scale 1 clips, a step at 1e-4 (norm 3.2, or 0.4 after S3's pre_scale) does not.
SCENARIOS = {
    "S1": dict(shadow=True, betas=(0.9, 0.98), eps=1e-6, wd=0.01, lr=5e-5, max_norm=5.0, pre_scale=1.0,
               p0_scale=2.0 ** -6, device_lr=False, grad_scale=(1.0, 1e-4, 1.0, 1e-4, 1.0, 1.0), seed=101),
    "S2": dict(shadow=False, betas=(0.9, 0.999), eps=1e-8, wd=0.1, lr=1e-3, max_norm=None, pre_scale=0.5,
               p0_scale=1.0, device_lr=False, grad_scale=(1.0, 0.5, 2.0, 1.0, 0.25, 1.0), seed=202),
    "S3": dict(shadow=True, betas=(0.9, 0.98), eps=1e-6, wd=0.01, lr=5e-5, max_norm=1.0, pre_scale=0.125,
               p0_scale=2.0 ** -6, device_lr=True, grad_scale=(1.0, 1.0, 1e-4, 1.0, 1e-4, 1.0), seed=303),
}


def build_probe(p0):
    """torch module whose named_parameters() are PROBE, in that order, holding clones of ``p0`` (fp32)."""
    root = torch.nn.Module()
    for name in NAMES:
        *path, leaf = name.split(".")
        mod = root
        for part in path:
            if not hasattr(mod, part):
                mod.add_module(part, torch.nn.Module())
            mod = getattr(mod, part)
        mod.register_parameter(leaf, torch.nn.Parameter(p0[name].clone()))
    assert [n for n, _ in root.named_parameters()] == NAMES
    return root


@functools.lru_cache(maxsize=1)
def make_inputs(scenario):
    """(p0, grads): fp32 start values by name, and per step a dict name -> fp32 gradient or None."""
    sc = SCENARIOS[scenario]

    def randn(shape, *key):
        g = torch.Generator().manual_seed(sc["seed"] * 10007 + sum(k * 131 ** i for i, k in enumerate(key)))
        return torch.randn(shape, generator=g)

    p0 = {n: randn(shape, 99, i) * sc["p0_scale"] for i, (n, shape, _) in enumerate(PROBE)}
    grads = []
    for k in range(N_STEPS):
        gd = {}
        for i, (n, shape, sigma) in enumerate(PROBE):
            if n == "never.weight" or (n == "late.weight" and k < LATE_FIRST) or (n == "once.weight" and k > 0):
                gd[n] = None
                continue
            g = randn(shape, k, i) * (sigma * sc["grad_scale"][k])
            if n == "late.weight":
                g.view(-1)[-1] = LATE_SPIKE * sc["grad_scale"][k]
            gd[n] = g
        grads.append(gd)
    return p0, grads


def lr_at(scenario, k):
    return SCENARIOS[scenario]["lr"] * (k + 1) / N_STEPS


def new_state(p0, slices, dtype=torch.float64):
    """name -> {p, m, v, step, seen, offset}; ``slices`` is ParamArena.slices (the norm variants need arena order)."""
    return {n: dict(p=p0[n].to(dtype).clone(), m=torch.zeros(p0[n].shape, dtype=dtype),
                    v=torch.zeros(p0[n].shape, dtype=dtype), step=0, seen=False, offset=slices[n][0]) for n in p0}


def _sumsq(state, eff, variant):
    if variant not in ("norm_first_pass_only", "norm_drops_last4"):
        return sum(float((g.double() ** 2).sum()) for g in eff.values() if g is not None)
    end = max(s["offset"] + s["p"].numel() for s in state.values())
    end = (end + CHUNK - 1) // CHUNK * CHUNK
    hi = SUMSQ_PASS if variant == "norm_first_pass_only" else end - 4
    total = 0.0
    for n, g in eff.items():
        if g is not None:
            keep = max(0, min(g.numel(), hi - state[n]["offset"]))
            total += float((g.double().reshape(-1)[:keep] ** 2).sum())
    return total


def clip_and_step_ref(state, grads, lr, betas, eps, wd, max_norm, pre_scale, variant=None):
    """One clip_grad_norm_ + AdamW step, in place on ``state``.  Returns (norm, gradient multiplier)."""
    assert variant is None or variant in VARIANTS, variant
    beta1, beta2 = betas
    eff = {}
    for n, s in state.items():
        g = grads.get(n)
        if g is not None:
            s["seen"] = True
            g = g.to(s["p"].dtype)
        elif (s["seen"] and variant != "skip_when_no_grad") or variant == "step_never_touched":
            g = torch.zeros_like(s["p"])
        eff[n] = g
    norm = pre_scale * math.sqrt(_sumsq(state, eff, variant))
    coef = 1.0
    if max_norm is not None:
        coef = max_norm / norm if variant == "no_clamp" else min(1.0, max_norm / (norm + 1e-6))
    if variant == "coef_not_applied":
        coef = 1.0
    mult = {"pre_scale_twice": pre_scale * pre_scale, "pre_scale_dropped": 1.0}.get(variant, pre_scale) * coef
    for n, s in state.items():
        if eff[n] is not None:
            s["step"] += 1
    global_step = max(s["step"] for s in state.values())
    for n, s in state.items():
        if eff[n] is None:
            continue
        g = eff[n] * mult
        t = global_step if variant == "global_step" else s["step"]
        p, m, v = s["p"], s["m"], s["v"]
        m.mul_(beta1).add_(g, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
        denom = (v + eps).sqrt() if variant == "eps_inside_sqrt" else v.sqrt().add_(eps)
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        step_size = lr * (bc2 if variant == "no_sqrt_bc2" else math.sqrt(bc2)) / bc1
        p.addcdiv_(m, denom, value=-step_size)
        decayed = {"decay_everywhere": True, "decay_nowhere": False}.get(variant, not R.no_decay_key(n))
        if decayed and wd > 0.0:
            p.add_(p, alpha=-lr * wd)
    return norm, mult


def clip_and_step_f32(state, grads, lr, betas, eps, wd, max_norm, pre_scale):
    """The same step as the reference project runs it: fp32 tensors, ``R.adamw_step``, the norm of oracle_train."""
    eff = {}
    for n, s in state.items():
        g = grads.get(n)
        if g is not None:
            s["seen"] = True
            g = g.float() * pre_scale
        elif s["seen"]:
            g = torch.zeros_like(s["p"])
        eff[n] = g
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in eff.values() if g is not None)).float()
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (float(total) + 1e-6))
    for n, s in state.items():
        if eff[n] is None:
            continue
        s["step"] += 1
        R.adamw_step(s["p"], eff[n] * coef, s["m"], s["v"], s["step"], lr, 0.0 if R.no_decay_key(n) else wd,
                     betas[0], betas[1], eps)
    return float(total), pre_scale * coef


def run(scenario, slices, variant=None, f32=False):
    """Generator over the six steps of a scenario: yields (k, live state, norm, multiplier) after step k."""
    sc = SCENARIOS[scenario]
    p0, grads = make_inputs(scenario)
    state = new_state(p0, slices, torch.float32 if f32 else torch.float64)
    for k in range(N_STEPS):
        args = (state, grads[k], lr_at(scenario, k), sc["betas"], sc["eps"], sc["wd"], sc["max_norm"], sc["pre_scale"])
        norm, mult = clip_and_step_f32(*args) if f32 else clip_and_step_ref(*args, variant=variant)
        yield k, state, norm, mult


# ---------------------------------------------------------------------------------------------- the compared quantities
FLOORS = {"m": 5e-5, "v": 5e-5, "disp": 2e-4}
NORM_GATE, MULT_GATE = 1e-5, 2e-5


def _rel_max(got, want):
    """max |got - want| over max |want| (0 / 0 = 0, x / 0 = inf)."""
    err, mag = float((got.double() - want).abs().max()), float(want.abs().max())
    return 0.0 if err == 0.0 else (err / mag if mag > 0.0 else math.inf)


def tensor_errors(got, want, p0):
    """{m, v, disp}: moments as max error over the tensor's max magnitude, displacement as relative L2 of p - p0.
    ``got`` holds p, m, v in any float dtype, ``want`` the float64 reference, ``p0`` the fp32 start values."""
    p0 = p0.double().reshape(-1)
    dg, dw = got["p"].double().reshape(-1) - p0, want["p"].reshape(-1) - p0
    err, mag = float((dg - dw).norm()), float(dw.norm())
    return {"m": _rel_max(got["m"].reshape(-1), want["m"].reshape(-1)),
            "v": _rel_max(got["v"].reshape(-1), want["v"].reshape(-1)),
            "disp": 0.0 if err == 0.0 else (err / mag if mag > 0.0 else math.inf)}


@functools.lru_cache(maxsize=None)
def e32(scenario, slices_key):
    """name -> per step {m, v, disp}: distance of the fp32 reference from the float64 one after that step or a later
    one, whichever is larger.  The relative error of a displacement falls as the displacement grows (c.weight in S1:
    one spacing of fp32 numbers against one step's decay at step 1, a twentieth of six steps' decay at step 6), so the
    first step must not set the figure for the last; a later step's lucky draw must not tighten an earlier one."""
    slices = dict(slices_key)
    p0, _ = make_inputs(scenario)
    per_step = {n: [] for n in NAMES}
    for (_, s32, _, _), (_, s64, _, _) in zip(run(scenario, slices, f32=True), run(scenario, slices)):
        for n in NAMES:
            touched = s64[n]["step"] > 0
            per_step[n].append(tensor_errors(s32[n], s64[n], p0[n]) if touched else {q: 0.0 for q in FLOORS})
    for n in NAMES:
        for k in range(N_STEPS - 2, -1, -1):
            per_step[n][k] = {q: max(per_step[n][k][q], per_step[n][k + 1][q]) for q in FLOORS}
    return per_step


def gates(scenario, slices):
    """name -> per step {m, v, disp}: max(4 x e32, floor) of that tensor, step and quantity; the factor 4 covers the
    kernel's different but fixed summation and fused-multiply order against torch's CPU kernels.  Taken per tensor, not
    as one figure per scenario: where an update is smaller than the spacing of fp32 numbers at |p| (c.weight and
    head.bias at a p0 scale of 2^-6), e32 of the displacement is 0.05 .. 1, and one gate for the whole scenario would let
    every other tensor pass with a displacement that is wrong by as much."""
    e = e32(scenario, tuple(sorted(slices.items())))
    return {n: [{q: max(4.0 * ek[q], FLOORS[q]) for q in FLOORS} for ek in e[n]] for n in NAMES}
