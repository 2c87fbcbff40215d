"""CPU tests of the restatements behind vln_bevbert_amd/ce_train.py (tests/ce_train_ref.py): the reference's live-tensor
GraphMap under autograd against the closed-form adjoint on a scripted walk, that every mistake a kernel could make
changes a compared value, the action draw's stream, and the C-ABI surface."""
import numpy as np
import pytest

from tests import ce_train_ref as T
from tests import rng_ref as R

H = 48


@pytest.fixture(scope="module")
def ref():
    steps, w = T.walk(H), T.upstream(H)
    d_avg, d_pano, fts, record = T.run_reference(steps, w)
    return {"steps": steps, "w": w, "d_avg": d_avg, "d_pano": d_pano, "fts": fts, "record": record}


def test_walk_contains_every_case_the_adjoint_distinguishes(ref):
    rec, N = ref["record"], T.WALK_N
    assert (T.WALK_B, T.WALK_T, T.WALK_N, T.WALK_C, T.WALK_L) == (3, 5, 6, 5, 7)
    obs = {}                                                            # (b, ghost) -> steps of its observations
    for t, rs in enumerate(rec):
        for b, r in enumerate(rs):
            if r is not None:
                for e, _ in r["cands"]:
                    if e >= N:
                        obs.setdefault((b, e - N), []).append(t)
    assert any(len(set(s)) >= 2 for s in obs.values()), "a ghost merged from two different steps"
    assert any(len(s) != len(set(s)) for s in obs.values()), "two candidates of one step merged into one ghost"
    assert any(e < N for rs in rec for r in rs if r is not None for e, _ in r["cands"]), "a candidate localised to a node"
    absent = 0
    for t, rs in enumerate(rec):
        for b, r in enumerate(rs):
            if r is not None and r["consumed"] >= 0:
                later = [rec[u][b] for u in range(t + 1, T.WALK_T) if rec[u][b] is not None]
                assert all(N + r["consumed"] not in x["ids"] for x in later)
                absent += len(later) > 0 and len(obs[b, r["consumed"]]) > 1
    assert absent >= 1, "a consumed ghost with several observations, absent from later listings"
    live = np.array([[r is not None for r in rs] for rs in rec])
    assert any(live[:3, b].all() and not live[3:, b].any() for b in range(T.WALK_B)), "a map not live from step 3 on"
    counts = [c for rs in rec for r in rs if r is not None for c in r["cnt"].values()]
    assert max(counts) == 4 and max(len(s) for s in obs.values()) <= 4
    rows = [row for rs in rec for r in rs if r is not None for j, (_, row) in enumerate(r["cands"]) if row != j]
    assert rows, "a candidate whose panorama row is not its own index"


def test_autograd_through_the_live_tensor_map_equals_the_closed_form_exactly(ref):
    d_avg, d_pano = T.closed_form(ref["record"], ref["w"], T.WALK_L)
    assert np.abs(ref["w"]).max() == 24 and max(np.abs(d_avg).max(), np.abs(d_pano).max()) <= 120
    assert np.array_equal(d_avg, np.rint(d_avg)) and np.array_equal(d_pano, np.rint(d_pano))
    assert np.array_equal(ref["d_avg"], d_avg) and np.array_equal(ref["d_pano"], d_pano)
    assert np.abs(d_pano).sum() > 0 and np.abs(d_avg).sum() > 0
    # every value is exact in the formats the device uses
    import torch
    for x in (d_avg, d_pano):
        assert np.array_equal(torch.from_numpy(x).to(torch.bfloat16).double().numpy(), x)
    # rows that must receive nothing
    for t, rs in enumerate(ref["record"]):
        for b, r in enumerate(rs):
            if r is None:
                assert not ref["d_avg"][t, b].any() and not ref["d_pano"][t, b].any()
                continue
            ghost_rows = {row for e, row in r["cands"] if e >= T.WALK_N}
            for row in range(T.WALK_L):
                if row not in ghost_rows:
                    assert not ref["d_pano"][t, b, row].any(), (t, b, row)


def test_leaving_a_step_out_of_the_loss_removes_that_steps_contribution_only(ref):
    full = T.closed_form(ref["record"], ref["w"], T.WALK_L)
    for t in range(T.WALK_T):
        use = [int(u != t) for u in range(T.WALK_T)]
        only = [int(u == t) for u in range(T.WALK_T)]
        got = T.run_reference(ref["steps"], ref["w"], use)[:2]
        part, one = T.closed_form(ref["record"], ref["w"], T.WALK_L, use), T.closed_form(ref["record"], ref["w"], T.WALK_L, only)
        for g, p, o, f in zip(got, part, one, full):
            assert np.array_equal(g, p) and np.array_equal(p + o, f)


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_every_wrong_variant_changes_a_compared_value(ref, variant):
    d_avg, d_pano = T.closed_form(ref["record"], ref["w"], T.WALK_L, variant=variant)
    n = int((d_avg != ref["d_avg"]).sum() + (d_pano != ref["d_pano"]).sum())
    print(variant, "differs in", n, "values")
    assert n > 0


# ------------------------------------------------------------------------------------------------------------ the draw
def test_teacher_keep_rate_is_binomial():
    u1 = np.concatenate([T.ce_action_uniforms(64, 0, t, R.salt_word(11))[1] for t in range(64)])
    keep = int((u1 <= np.float32(0.25)).sum())
    sigma = np.sqrt(4096 * 0.25 * 0.75)
    print(f"{keep} of {u1.size} draws keep the teacher (expected 1024, sigma {sigma:.1f})")
    assert u1.size == 4096 and abs(keep - 1024) <= 3 * sigma


@pytest.mark.parametrize("step_seed", [None, 11, 2 ** 32 + 3])
@pytest.mark.parametrize("seed", [0, 0x5EED])
def test_action_draw_hashes_words_of_its_own(step_seed, seed):
    salt = None if step_seed is None else R.salt_word(step_seed)
    for t in range(16):
        ce = set(int(x) for x in T.ce_action_inputs(64, seed, t, salt).reshape(-1))
        assert len(ce) == 128
        ghost = R.ghost_chain(4, 16, seed, t + 1, salt)
        others = {"nav": R.nav_inputs(64, seed, t, salt), "waypoint": R.waypoint_inputs(64, seed, t, salt),
                  "ghost": np.concatenate([v.reshape(-1) for v in ghost.values()])}
        for name, v in others.items():
            assert not (ce & set(int(x) for x in np.asarray(v).reshape(-1))), (name, t)
    assert T.ce_action_key(seed, 0, salt) != R.nav_key(seed, 0, salt)


def test_sampler_restatement_rule():
    logits = np.array([[0.0, -np.inf, 0.0, -np.inf], [-np.inf, 2.0, -np.inf, -np.inf]], np.float32)
    teacher = np.array([3, -100])
    for u0, want in ((0.25, 0), (0.75, 2), (0.999999, 2)):
        a, cum = T.sample_action(logits, teacher, 0.5, np.float32([u0, u0]), np.float32([0.9, 0.9]))
        assert a.tolist() == [want, 1] and cum[0].tolist() == [0.5, 0.5, 1.0, 1.0]
    a, _ = T.sample_action(logits, teacher, 0.5, np.float32([0.1, 0.1]), np.float32([0.5, 0.5000001]))
    assert a.tolist() == [3, 1]                                          # <=, as the reference
    a, _ = T.sample_action(logits, teacher, 0.5, np.float32([0.1, 0.1]), np.float32([0.7, 0.2]))
    assert a.tolist() == [0, -100]                                       # -100 passes through


# --------------------------------------------------------------------------------------------------------- the surface
def test_new_entry_points_are_declared_and_typed():
    from vln_bevbert_amd import lib
    names = {"bevbert_ce_tape_record", "bevbert_ce_embeds_bwd", "bevbert_ce_sample_action"}
    assert names <= set(lib.prototypes())
    assert "ce_train.hip" in lib.SOURCES
