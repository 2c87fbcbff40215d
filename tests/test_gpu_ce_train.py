"""csrc/ce_train.hip + vln_bevbert_amd/ce_train.py on the GPU.

The adjoint of the map's embedding path against the fp64 live-tensor restatement of the reference (tests/ce_train_ref.py)
on its scripted walk, bit for bit -- every upstream gradient is 12 k, so every quotient and sum is an integer exact in
fp32 and bf16, and each mistake listed in tests/test_ce_train_host.py changes a compared value; the write / read ordering
through one backward call; determinism, no synchronisation, a second episode on the same tape; the action draw against
its restatement; one training rollout end to end against a torch-glue run of the same device modules that keeps the
map's embeddings as live tensors in Python dicts.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from tests import ce_train_ref as T
from tests import rng_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-3          # tests/test_gpu_model.py


@functools.lru_cache(maxsize=None)
def _ref(H):
    steps, w = T.walk(H), T.upstream(H)
    d_avg, d_pano, fts, record = T.run_reference(steps, w)
    return {"steps": steps, "w": w, "d_avg": d_avg, "d_pano": d_pano, "record": record, "a": T.action_rows(record, steps)}


def _map(H, dtype):
    from vln_bevbert_amd.ce_map import CEGraphMap
    return CEGraphMap(T.WALK_B, H, DEV, dtype=dtype, loc_noise=T.LOC_NOISE, node_capacity=T.WALK_N, ghost_capacity=T.WALK_GH)


def _tape(H, dtype):
    from vln_bevbert_amd.ce_train import CEMapTape
    return CEMapTape(_map(H, dtype), T.WALK_T, T.WALK_C, T.WALK_L)


def _device_inputs(ref, dtype):
    out = []
    for s in ref["steps"]:
        d = {k: torch.from_numpy(s[k]).to(DEV) for k in ("cand_count", "cand_angles", "cand_distances", "nav_types")}
        d["avg"], d["pano"] = (torch.from_numpy(s[k]).to(DEV, dtype) for k in ("avg", "pano"))
        out.append(d)
    return out, torch.from_numpy(ref["a"]).to(DEV)


def _walk(obj, ref, inputs, a, grad):
    """The scripted walk through a CEMapTape or a plain CEGraphMap: per step the leaves, the listing and cand_slot."""
    m = getattr(obj, "map", obj)
    out = []
    for t, (s, d) in enumerate(zip(ref["steps"], inputs)):
        avg, pano = d["avg"].clone().requires_grad_(grad), d["pano"].clone().requires_grad_(grad)
        slot = obj.update(t + 1, d["cand_count"], d["cand_angles"], d["cand_distances"], avg, pano, d["nav_types"],
                          cur_pos=s["cur_pos"], heading=s["heading"], live=s["live"])
        nav = obj.nav_gmap_variable()
        m.act(a[t], last_step=t == T.WALK_T - 1, gmap_ids=nav["gmap_ids"])
        out.append({"avg": avg, "pano": pano, "slot": slot, "nav": nav})
    return out


def _grads(run):
    z = torch.zeros_like
    return (torch.stack([z(o["avg"]) if o["avg"].grad is None else o["avg"].grad for o in run]),
            torch.stack([z(o["pano"]) if o["pano"].grad is None else o["pano"].grad for o in run]))


def _want(ref, dtype, use=None):
    if use is None:
        d_avg, d_pano = ref["d_avg"], ref["d_pano"]
    else:
        d_avg, d_pano = T.closed_form(ref["record"], ref["w"], T.WALK_L, use)
    return torch.from_numpy(d_avg).to(DEV, dtype), torch.from_numpy(d_pano).to(DEV, dtype)


def _loss(run, w, dtype, use=None):
    return sum((o["nav"]["gmap_img_fts"].float() * w[t]).sum() for t, o in enumerate(run) if use is None or use[t])


# ------------------------------------------------------------------------------------------- the kernel, bit for bit
@pytest.mark.parametrize("H", [48, 768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_adjoint_kernel_equals_the_live_tensor_restatement_bit_for_bit(dtype, H):
    ref = _ref(H)
    inputs, a = _device_inputs(ref, dtype)
    tape, plain = _tape(H, dtype), _map(H, dtype)
    with torch.no_grad():
        run, base = _walk(tape, ref, inputs, a, False), _walk(plain, ref, inputs, a, False)
    # the forward is the tape-less map's, bit for bit
    for t, (o, p) in enumerate(zip(run, base)):
        assert torch.equal(o["slot"], p["slot"]), t
        for k in p["nav"]:
            assert torch.equal(o["nav"][k], p["nav"][k]), (t, k)
    for k in plain.t:
        assert torch.equal(tape.map.t[k], plain.t[k]), k
    assert tape.map.check_overflow() == 0
    # the tape is the restatement's record
    h = {k: getattr(tape, k).cpu() for k in ("live", "cur", "slot", "row", "ids", "cnt")}
    for t, rs in enumerate(ref["record"]):
        for b, r in enumerate(rs):
            assert int(h["live"][t, b]) == (r is not None) and int(h["cur"][t, b]) == (-1 if r is None else r["cur"])
            if r is not None:
                want = [(e, row) if e >= T.WALK_N else (-1, -1) for e, row in r["cands"]]
                got = list(zip(h["slot"][t, b].tolist(), h["row"][t, b].tolist()))
                assert got[:len(want)] == want and all(x == (-1, -1) for x in got[len(want):]), (t, b, got, want)
                assert h["ids"][t, b, :len(r["ids"])].tolist() == r["ids"]
                assert all(int(h["cnt"][t, b, g]) == c for g, c in r["cnt"].items())
    # the kernel, consumer steps in backward's order
    w = torch.from_numpy(ref["w"]).to(DEV, dtype)
    for t in reversed(range(T.WALK_T)):
        tape.embeds_bwd(t, w[t])
    want_avg, want_pano = _want(ref, torch.float32)
    nz = int((want_pano != 0).sum()), int((want_avg != 0).sum())
    print(f"{dtype} H={H}: {nz[0]} non-zero d_pano and {nz[1]} non-zero d_avg values; max |value| "
          f"{float(want_pano.abs().max()):.0f}; differing: d_avg {int((tape.d_avg != want_avg).sum())}, "
          f"d_pano {int((tape.d_pano != want_pano).sum())}")
    assert nz[0] > 0 and nz[1] > 0
    assert torch.equal(tape.d_avg, want_avg) and torch.equal(tape.d_pano, want_pano)


# ------------------------------------------------------------------------------------------- ordering through autograd
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_backward_call_gives_the_same_result_and_a_step_left_out_removes_only_its_own_term(dtype):
    H = 48
    ref = _ref(H)
    inputs, a = _device_inputs(ref, dtype)
    w = torch.from_numpy(ref["w"]).to(DEV)
    for use in [None] + [[int(u != t) for u in range(T.WALK_T)] for t in range(T.WALK_T)]:
        run = _walk(_tape(H, dtype), ref, inputs, a, True)
        _loss(run, w, dtype, use).backward()
        got, want = _grads(run), _want(ref, dtype, use)
        assert got[0].dtype == dtype and got[1].dtype == dtype
        print(f"{dtype} steps in the loss {use}: differing d_avg {int((got[0] != want[0]).sum())}, d_pano {int((got[1] != want[1]).sum())}")
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), use
        if use is None:
            full = got
    got = full
    # rows that must receive nothing are exactly zero (the restatement has them at zero; stated once more from the record)
    for t, rs in enumerate(ref["record"]):
        for b, r in enumerate(rs):
            rows = set() if r is None else {row for e, row in r["cands"] if e >= T.WALK_N}
            for row in range(T.WALK_L):
                if row not in rows:
                    assert not bool(got[1][t, b, row].any()), (t, b, row)
            if r is None:
                assert not bool(got[0][t, b].any())


def test_backward_is_deterministic_does_not_synchronise_and_a_second_episode_starts_clean():
    H, dtype = 48, torch.float32
    ref = _ref(H)
    inputs, a = _device_inputs(ref, dtype)
    w = torch.from_numpy(ref["w"]).to(DEV)
    results = []
    tape = _tape(H, dtype)
    for episode in range(3):                                           # two fresh tapes, then the second one again
        if episode == 1:
            tape = _tape(H, dtype)
        elif episode == 2:
            tape.begin_episode()
        run = _walk(tape, ref, inputs, a, True)
        loss = _loss(run, w, dtype)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        results.append(_grads(run))
    want = _want(ref, dtype)
    for g in results:
        assert torch.equal(g[0], want[0]) and torch.equal(g[1], want[1])
    # a backward of the episode before begin_episode() is refused instead of adding into the new record
    from vln_bevbert_amd.lib import BevBertHipError
    tape.begin_episode()
    run = _walk(tape, ref, inputs, a, True)
    loss = _loss(run, w, dtype)
    tape.begin_episode()
    with pytest.raises(BevBertHipError):
        loss.backward()


# ------------------------------------------------------------------------------------------------------------ the draw
def _sampler_case(dtype, t, seed, salt, B=8, G=23):
    """Logits with -inf masks and one row with a single open slot, chosen (on the CPU) so that no cumulative probability
    lies within 1e-4 of u0."""
    u0, u1 = T.ce_action_uniforms(B, seed, t, salt)
    for k in range(64):
        g = torch.Generator().manual_seed(100 * t + k)
        x = torch.randn(B, G, generator=g) * 2
        x[torch.rand(B, G, generator=g) < 0.3] = -float("inf")
        x[:, 0] = torch.randn(B, generator=g)                          # [stop] is always open
        x[5] = -float("inf")
        x[5, 11] = 0.7
        x = x.to(dtype)
        _, cum = T.sample_action(x.float().numpy(), np.zeros(B, np.int64), -1.0, u0, u1)
        if np.abs(cum - u0[:, None]).min() > 1e-4:
            return x, u0, u1
    raise AssertionError("no logits with a margin found")


@pytest.mark.parametrize("t", [0, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_action_draw_equals_its_restatement(dtype, t):
    from vln_bevbert_amd import ops
    from vln_bevbert_amd.ce_train import sample_action
    seed, step_seed, ratio = 0x5EED, 7, 0.5
    ops.RT.new_step(step_seed)
    salt = R.salt_word(step_seed)
    x, u0, u1 = _sampler_case(dtype, t, seed, salt)
    B = x.shape[0]
    over = u1 <= np.float32(ratio)
    assert over.any() and not over.all()
    teacher = np.arange(B, dtype=np.int64) % 3
    teacher[np.nonzero(over)[0][0]] = -100
    for r in (ratio, 0.0, 1.0):
        want, _ = T.sample_action(x.float().numpy(), teacher, r, u0, u1)
        a, g0, g1 = sample_action(x.to(DEV), torch.from_numpy(teacher).to(DEV), r, seed, t)
        assert np.array_equal(g0.cpu().numpy(), u0) and np.array_equal(g1.cpu().numpy(), u1)
        print(f"{dtype} t={t} ratio {r}: a_t {a.tolist()} want {want.tolist()}")
        assert a.tolist() == want.tolist()
        assert (a.cpu().numpy()[u1 <= np.float32(r)] == teacher[u1 <= np.float32(r)]).all()
    assert want.tolist() == teacher.tolist() and -100 in want           # ratio 1: the teacher everywhere, -100 included
    assert int(sample_action(x.to(DEV), torch.from_numpy(teacher).to(DEV), 0.0, seed, t)[0][5]) == 11


# ------------------------------------------------------------------------------------------ one rollout, end to end
class _GlueMap:
    """The torch glue the tape replaces: the device map for everything but the embeddings, which stay live tensors in
    Python dicts as in the reference's GraphMap and are stacked in the device listing's order."""

    def __init__(self, m):
        self.map = m
        # tensor / tensor is a true division, as in the map's kernel (tensor / Python number multiplies by a reciprocal)
        self.counts = [torch.tensor(float(c), device=DEV) for c in range(17)]
        self.begin_episode()

    def begin_episode(self):
        self.map.reset()
        self.nodes, self.ghosts = [{} for _ in range(self.map.B)], [{} for _ in range(self.map.B)]

    def update(self, step_id, cand_count, cand_angles, cand_distances, avg, pano, nav_types, cur_pos=None, heading=None,
               live=None):
        m = self.map
        slot = m.update(step_id, cand_count, cand_angles, cand_distances, avg, pano, nav_types, cur_pos=cur_pos,
                        heading=heading, live=live)
        cur, sl, nt = m.t["cur_vp"].tolist(), slot.tolist(), nav_types.cpu().numpy()
        for b in range(m.B):
            if not live[b]:
                continue
            self.nodes[b][cur[b]] = avg[b]
            rows = np.nonzero(nt[b] == 1)[0]
            for j, e in enumerate(sl[b]):
                if e >= m.N:
                    g = self.ghosts[b]
                    g[e] = [pano[b, int(rows[j])], 1] if e not in g else [g[e][0] + pano[b, int(rows[j])], g[e][1] + 1]
        return slot

    def nav_gmap_variable(self):
        m = self.map
        o = m.nav_gmap_variable()
        zero = o["gmap_img_fts"].new_zeros(m.H)
        rows = []
        for b, ids in enumerate(o["gmap_ids"].tolist()):
            for e in ids:
                rows.append(zero if e < 0 else (self.nodes[b][e] if e < m.N else self.ghosts[b][e][0] / self.counts[self.ghosts[b][e][1]]))
        live = torch.stack(rows).view(m.B, m.G, m.H)
        assert torch.equal(live.detach(), o["gmap_img_fts"])
        o["gmap_img_fts"] = live
        return o


def _rollout(model, pred, mapper, terms=(0, 1, 2), pano_grad=(True, True, True)):
    """3 steps of ce_train.train_step with a scripted simulator: the agent moves to the ghost it chose; goal distances
    are fixed numbers.  Returns (loss, per-step fused logits, step-0 outputs)."""
    from vln_bevbert_amd import ce_train, ops
    from tests import waypoint_ref as WR
    m = mapper.map
    B = m.B
    ops.RT.new_step(5)
    mapper.begin_episode()
    gen = torch.Generator().manual_seed(4)
    txt_ids = torch.randint(1, 1000, (B, 20), generator=gen).to(DEV)
    txt_masks = torch.ones(B, 20, dtype=torch.bool, device=DEV)
    txt = model("language", {"txt_ids": txt_ids, "txt_masks": txt_masks})
    pos, live = np.array([[0.0, 0.0, 0.0], [5.0, 1.0, -2.0]]), np.ones(B, bool)
    ghost_dist = torch.from_numpy(3.0 + np.abs(WR.synthetic(33, (B, m.Gh))).astype(np.float64)).to(DEV)
    loss, logits = None, []
    for t in range(3):
        o = ce_train.train_step(
            model, pred, mapper, t + 1, txt, txt_masks, torch.from_numpy(WR.synthetic(60 + t, (B * 12, 512))).to(DEV),
            torch.from_numpy(WR.synthetic(70 + t, (B * 12, 128, 4, 4))).to(DEV),
            torch.from_numpy(WR.synthetic(80 + t, (B, 12, 196, 768))).to(DEV),
            torch.from_numpy(np.abs(WR.synthetic(90 + t, (B, 12, 14, 14))) * 0.4).to(DEV), pos, np.array([0.4, 2.0]) + t, live,
            torch.full((B,), 6.0 - 2 * t, dtype=torch.float64, device=DEV), ghost_dist,
            loss_sum=loss if t in terms else None, sample_ratio=0.5, seed=3, last_step=t == 2, pano_grad=pano_grad[t])
        if t in terms:
            loss = o["loss_sum"]
        logits.append(o["fused_logits"].detach())
        for b, act in enumerate(m.to_reference(o["rec"])):                 # the caller's one read-back of a step
            if act is not None and act["action"]["act"] == 4:
                pos[b] = act["action"]["ghost_pos"]
    return ce_train.finish(loss, 3 * B, 1.0), logits


def _param_grads(arena, rollout):
    arena.zero_grad()
    loss, logits = rollout()
    loss.backward()
    arena.sync()
    return {n: p.main_grad.clone() for n, p in arena.named}, loss.detach(), logits


def test_one_training_rollout_end_to_end_against_live_tensors_in_python_dicts(monkeypatch):
    from vln_bevbert_amd import waypoint as W, weights
    from vln_bevbert_amd.ce_map import CEGraphMap
    from vln_bevbert_amd.ce_train import CEMapTape
    from vln_bevbert_amd.config import BevBertConfig
    from vln_bevbert_amd.nav_model import GlocalTextPathNavCMT
    from tests.helpers import rule_state_dict
    from vln_bevbert_amd import ops
    # weight gradients in line on the one stream: this test compares numbers, and it must not be the place where the
    # process picks its weight-gradient side streams (tests that capture steps later depend on where that happens)
    monkeypatch.setattr(ops.WgradStream, "enabled", False)
    B = 2
    cfg = BevBertConfig.ce(num_l_layers=2, num_x_layers=2, num_pano_layers=1, vocab_size=1200, max_position_embeddings=128)
    model = GlocalTextPathNavCMT(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    arena = model.finalize(DEV, torch.float32)
    model.eval()                                                          # no dropout: the two runs must see the same numbers
    pred = W.WaypointPredictor()
    pred.load_state_dict(rule_state_dict("waypoint_keys.txt"), strict=True)
    pred.finalize(DEV, torch.float32)

    class _Plain:                                                         # today's map: embeddings enter as constants
        def __init__(self, m):
            self.map, self.update, self.nav_gmap_variable, self.begin_episode = m, m.update, m.nav_gmap_variable, m.reset

    def new_map():
        return CEGraphMap(B, cfg.hidden_size, DEV, loc_noise=0.5)
    tape = CEMapTape(new_map(), 3, 5, 17)
    g_tape, loss_t, logits_t = _param_grads(arena, lambda: _rollout(model, pred, tape))
    glue = _GlueMap(new_map())
    g_glue, loss_g, logits_g = _param_grads(arena, lambda: _rollout(model, pred, glue))
    for t in range(3):
        assert torch.equal(logits_t[t], logits_g[t]), t
        assert int(torch.isfinite(logits_t[t]).sum()) >= 2 * B
    print(f"loss: tape {float(loss_t):.9g}, live tensors {float(loss_g):.9g}")
    assert float(loss_t) == float(loss_g) and np.isfinite(float(loss_t))
    worst = ("", 0.0)
    for n, g in g_glue.items():
        scale = float(g.abs().max())
        if scale == 0.0:
            assert not bool(g_tape[n].any()), n
            continue
        d = float((g_tape[n] - g).abs().max()) / scale
        if d > worst[1]:
            worst = (n, d)
    print(f"worst parameter-gradient distance (max-abs / absmax) over {len(g_glue)} parameters: {worst[1]:.3e} at {worst[0]}")
    assert worst[1] <= FP32_TOL
    # without the tape the panorama side gets nothing at all; with it, it does
    plain = _Plain(new_map())
    g_plain, loss_p, logits_p = _param_grads(arena, lambda: _rollout(model, pred, plain))
    assert all(torch.equal(a, b) for a, b in zip(logits_p, logits_t))
    pano_side = [n for n in g_plain if n.startswith("img_embeddings.")]
    assert len(pano_side) >= 8 and any("pano_encoder" in n for n in pano_side)
    assert all(not bool(g_plain[n].any()) for n in pano_side)
    assert all(bool(g_tape[n].any()) for n in pano_side if "obj_" not in n), [n for n in pano_side if not bool(g_tape[n].any())]
    # the cross-step flow: with only step 0's panorama pass in the graph, dropping step 2's loss term changes its gradient
    only0 = (True, False, False)
    g_full = _param_grads(arena, lambda: _rollout(model, pred, tape, (0, 1, 2), only0))[0]
    g_01 = _param_grads(arena, lambda: _rollout(model, pred, tape, (0, 1), only0))[0]
    n = "img_embeddings.img_linear.weight"
    d = float((g_full[n] - g_01[n]).abs().max())
    print(f"step-0 panorama pass, {n}: |grad| max {float(g_full[n].abs().max()):.3e}; changed by step 2's loss term: {d:.3e}")
    assert d > 0 and bool(g_01[n].any())
    assert tape.map.check_overflow() == 0 and glue.map.check_overflow() == 0
