"""Every random stream of the device against the host restatement of its specification (tests/rng_ref.py, which calls
nothing in the package): the dropout keep mask bit for bit (the hook every "matches exported mask" test compares with),
one dropout consumer and the attention keep bits without the hook, the uniform draws of bevbert_nav_action and
bevbert_wp_candidates bit for bit and the decisions taken from them, the ghost noise of bevbert_ce_update, the
separation of the nav and waypoint draws of one step, and the offsets a real training step hands to its dropout sites."""
import math

import numpy as np
import pytest
import torch

from tests import rng_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from vln_bevbert_amd import lib, ops
    lib.load()
    return ops


def _salt(ops, step_seed):
    """Start a step on the device and return its salt word as the restatement computes it."""
    ops.RT.new_step(step_seed)
    return R.salt_word(step_seed)


# -------------------------------------------------------------------------------------------------- keep mask, bit-exact
SIZES = (1, 2, 3, 255, 4097, 2 ** 20 + 1)
PS = (0.1, 0.3, 0.5, 1e-5, 0.99999)           # thresholds 6554, 19661, 32768, 1 and the clamp 65535
SEEDS = (0, 0x5EED, 2 ** 32 + 5, 2 ** 63 + 7)
OFFSETS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3)
STEP_SEEDS = (3, 2 ** 32 + 3)
KEEP_CASES = [(STEP_SEEDS[(i // 2) % 2], SIZES[i % 6], PS[i % 5], SEEDS[(i + i // 4) % 4], OFFSETS[(i + i // 5) % 5])
              for i in range(40)]


def test_keep_mask_cases_cover_every_value_of_every_axis(ops):
    assert SEEDS[1] == ops.RT.SEED
    for axis, values in enumerate((STEP_SEEDS, SIZES, PS, SEEDS, OFFSETS)):
        assert {c[axis] for c in KEEP_CASES} == set(values)
    assert {(c[1], c[2]) for c in KEEP_CASES} == {(n, p) for n in SIZES for p in PS}
    assert [R.drop_threshold(p) for p in PS] == [6554, 19661, 32768, 1, 65535]


@pytest.mark.parametrize("step_seed,n,p,seed,offset", KEEP_CASES)
def test_exported_keep_mask_equals_the_restatement_bit_for_bit(ops, step_seed, n, p, seed, offset):
    salt = _salt(ops, step_seed)
    got = ops.dropout_keep_mask(n, p, seed, offset, DEV).cpu().numpy()
    want = R.keep_mask(n, p, seed, offset, salt)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------------------- consumers, without the hook
@pytest.mark.parametrize("p", [0.1, 0.3])
def test_dropout_add_of_ones_is_the_restated_mask_over_one_minus_p(ops, p):
    salt = _salt(ops, 2 ** 32 + 3)
    x = torch.ones(4, 1031, device=DEV)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for offset in (0, x.numel()):                        # the step's first two sites
        assert ops.RT.offset == offset
        y = ops.dropout(x, p, True).cpu().numpy().reshape(-1)
        want = np.where(R.keep_mask(x.numel(), p, ops.RT.seed, offset, salt), scale, np.float32(0.0))
        assert y.dtype == np.float32 and np.array_equal(y, want), int((y != want).sum())


def test_attention_keep_bit_words_decode_to_the_restated_mask(ops):
    """Forward layout as test_attention_keep_bit_workspace_holds_the_exported_mask_in_both_layouts documents it: bit l of
    word (bh, q16, k64, t, r) = query 16 q16 + (l & 15), key 64 k64 + 16 t + 4 (l >> 4) + r; element index
    (bh Lq + q) Lk2 + key with Lk2 = Lk rounded up to even."""
    B, nh, Lq, Lk, p, offset = 1, 12, 33, 441, 0.1, 5
    salt = _salt(ops, 77)
    bits = ops.attn_drop_bits(B, nh, Lq, Lk, p, ops.RT.seed, offset, DEV).cpu().numpy().view(np.uint64)
    Lk2 = (Lk + 1) // 2 * 2
    keep = R.keep_mask(B * nh * Lq * Lk2, p, ops.RT.seed, offset, salt).reshape(B * nh, Lq, Lk2)
    nq16, nk64 = (Lq + 127) // 128 * 8, (Lk + 63) // 64
    half = B * nh * nq16 * nk64 * 16
    assert bits.shape[0] == 3 * half
    lanes = np.arange(64)
    f = bits[:half].reshape(B * nh, nq16, nk64, 4, 4)
    q = np.arange(nq16)[:, None, None, None, None] * 16 + (lanes & 15)
    k = (np.arange(nk64)[None, :, None, None, None] * 64 + np.arange(4)[None, None, :, None, None] * 16
         + (lanes >> 4) * 4 + np.arange(4)[None, None, None, :, None])
    got = ((f[..., None] >> lanes.astype(np.uint64)) & np.uint64(1)).astype(bool)         # (bh, q16, k64, t, r, lane)
    ok = (q < Lq) & (k < Lk)
    qq, kk = np.broadcast_arrays(np.minimum(q, Lq - 1), np.minimum(k, Lk - 1))
    assert ok.sum() == Lq * Lk
    assert np.array_equal(got[:, ok], keep[:, qq, kk][:, ok])


# ------------------------------------------------------------------------------------------------------------ nav draws
def _nav_state(B, N=4):
    return dict(ended=torch.zeros(B, dtype=torch.uint8, device=DEV), stop_scores=torch.zeros(B, N, device=DEV),
                stop_order=torch.full((B, N), -1, dtype=torch.int32, device=DEV),
                n_stop=torch.zeros(B, dtype=torch.int32, device=DEV))


def _nav_inputs(B, C):
    return dict(cand=torch.zeros(B, C, dtype=torch.int32, device=DEV), cur=torch.zeros(B, dtype=torch.int32, device=DEV),
                goal=torch.ones(B, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("step_seed,seed,t", [(11, 0, 0), (2 ** 32 + 3, 7, 5)])
def test_sample_draw_is_the_restated_uniform_and_its_fp64_inverse_cdf(ops, step_seed, seed, t):
    from vln_bevbert_amd import nav_expert as NE
    B, C = 4096, 7
    g = torch.Generator().manual_seed(1)
    row = torch.tensor([[0.3, -1.0, 1.2, -math.inf, 0.0, 2.0, -0.5]])
    x = row + 0.3 * torch.randn(B, C, generator=g)
    salt = _salt(ops, step_seed)
    o = NE.action_step(x.to(DEV), "sample", t, 15, seed=seed, **_nav_inputs(B, C), **_nav_state(B))
    u0, _ = R.nav_uniforms(B, seed, t, salt)
    rand = o["rand"].cpu().numpy()
    assert rand.dtype == np.float32 and np.array_equal(rand, u0), int((rand != u0).sum())
    cdf = torch.softmax(x.double(), 1).cumsum(1).numpy()
    gap = np.abs(cdf - u0.astype(np.float64)[:, None]).min(1)
    want = (u0.astype(np.float64)[:, None] >= cdf).sum(1)          # first slot whose cdf exceeds u0 (p = 0 slots never do)
    checked = gap >= 1e-5
    left_out = int((~checked).sum())
    print(f"nav sample: {B - left_out} of {B} rows checked (left out: {left_out})")
    assert left_out <= 0.01 * B
    assert (want[checked] < C).all() and (want[checked] != 3).all()
    assert np.array_equal(o["a_t"].cpu().numpy()[checked], want[checked])


def test_expl_sample_explores_where_u0_says_and_picks_the_slot_u1_says(ops):
    from vln_bevbert_amd import nav_expert as NE
    B, C, t, seed, ratio = 4096, 9, 2, 3, 0.6
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, generator=g) * 2
    masks = (torch.rand(B, C, generator=g) < 0.5).to(torch.uint8)
    masks[:, 1] = 1
    salt = _salt(ops, 5)
    o = NE.action_step(x.to(DEV), "expl_sample", t, 15, seed=seed, masks=masks.to(DEV), expl_max_ratio=ratio,
                       **_nav_inputs(B, C), **_nav_state(B))
    u0, u1 = R.nav_uniforms(B, seed, t, salt)
    assert np.array_equal(o["rand"].cpu().numpy(), u0)
    explore = u0 > np.float32(ratio)
    assert 0.3 < explore.mean() < 0.5
    mk = masks.numpy() != 0
    cnt = mk.sum(1)
    slot = np.minimum((u1 * cnt.astype(np.float32)).astype(np.int32), cnt - 1)        # the product in float32
    rank = np.cumsum(mk, 1) - 1                                                       # rank of a set slot among the set ones
    want = np.where(explore, (mk & (rank == slot[:, None])).argmax(1), x.max(1)[1].numpy())
    assert len(set(slot[explore])) > 4
    assert np.array_equal(o["a_t"].cpu().numpy(), want)


# -------------------------------------------------------------------------------------------------------- waypoint draw
@pytest.mark.parametrize("step_seed", [11, 2 ** 32 + 3])
@pytest.mark.parametrize("seed,t", [(5, 3), (2 ** 31 + 1, 0)])
def test_waypoint_draw_is_the_restated_uniform(ops, step_seed, seed, t):
    from vln_bevbert_amd import waypoint as W
    B = 37
    logits = torch.randn(B, 12, 120, generator=torch.Generator().manual_seed(2)).to(DEV)
    salt = _salt(ops, step_seed)
    rand = W.waypoint_candidates(logits, True, seed=seed, t=t)["rand"].cpu().numpy()
    want = R.waypoint_uniforms(B, seed, t, salt)
    assert rand.shape == (B, 5) and rand.dtype == np.float32 and np.array_equal(rand, want)


# ---------------------------------------------------------------------------------------------------------- ghost noise
@pytest.mark.parametrize("step_seed,seed", [(9, 7), (2 ** 32 + 3, 0)])
def test_ghost_noise_is_the_restated_box_muller_draw(ops, step_seed, seed):
    from tests import test_gpu_ce_map as M
    from vln_bevbert_amd.ce_map import CEGraphMap
    gold = np.load(M.GOLDEN)
    T, B = gold["in_live"].shape
    a = 0.3
    salt = _salt(ops, step_seed)
    m = CEGraphMap(B, 32, DEV, seed=seed, loc_noise=float(gold["loc_noise"]), merge_ghost=gold["merge_ghost"].tolist(),
                   ghost_aug=a)
    drawn, worst = 0, 0.0
    for t, o in enumerate(M._drive(gold, m)):
        s = o["state"]
        nx, nz = R.ghost_noise(B, m.Gh, seed, t + 1, salt, a)
        want = np.stack([nx, np.zeros_like(nx), nz], axis=-1)
        al = s["ghost_alive"]
        drawn += int(al.sum())
        if al.any():
            worst = max(worst, float(np.abs((s["ghost_aug"] - s["ghost_mean"])[al] - want[al]).max()))
    print(f"ghost noise: {drawn} draws, worst difference from the restatement {worst:.2e}")
    assert drawn > 20 and worst <= M.F64_TOL


# ------------------------------------------------------------------------------------------------------------- coupling
def test_waypoint_and_nav_draws_of_one_step_share_no_value(ops):
    """Default seeds, one t, one step: before the domain constants waypoint [b, 0] was nav [2 b], [b, 1] nav u1 of 2 b and
    [b, 4] nav [2 b + 1] (the device-side twin of test_consumers_of_one_step_hash_disjoint_words)."""
    from vln_bevbert_amd import nav_expert as NE
    from vln_bevbert_amd import waypoint as W
    B, C, t = 64, 7, 3
    ops.RT.new_step(11)
    g = torch.Generator().manual_seed(3)
    wp = W.waypoint_candidates(torch.randn(B, 12, 120, generator=g).to(DEV), True, t=t)["rand"].cpu().numpy()
    nav = NE.action_step(torch.randn(2 * B, C, generator=g).to(DEV), "sample", t, 15, **_nav_inputs(2 * B, C),
                         **_nav_state(2 * B))["rand"].cpu().numpy()
    assert not (wp[:, 0] == nav[0::2]).any() and not (wp[:, 4] == nav[1::2]).any()
    assert not set(wp[:, [0, 4]].reshape(-1).tolist()) & set(nav.tolist())


# ------------------------------------------------------------------------------------ stream bookkeeping of a real step
def test_dropout_sites_of_a_training_step_advance_the_offset_by_their_size_and_get_distinct_keys(ops, monkeypatch):
    from vln_bevbert_amd import synthetic, weights
    from vln_bevbert_amd.config import BevBertConfig
    from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining
    cfg = BevBertConfig.tiny(num_l_layers=1, num_x_layers=1)
    model = GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(weights.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model.tie_weights()
    arena = model.finalize(DEV, torch.float32)
    model.train()
    assert cfg.hidden_dropout_prob > 0 and cfg.attention_probs_dropout_prob > 0
    sites = []
    inner = ops.RT.next_offset

    def recording(n):
        off = inner(n)
        sites.append((off, int(n)))
        return off
    monkeypatch.setattr(ops.RT, "next_offset", recording)
    step_seed = 2 ** 32 + 3
    for task in ("mlm", "sap", "masksem"):
        del sites[:]
        ops.RT.new_step(step_seed)
        arena.zero_grad()
        batch = synthetic.batch_to(synthetic.make_batch(cfg, task, 2, seed=5, ragged=True), DEV)
        loss = model(batch, task).mean()
        loss.backward()
        arena.sync()
        assert torch.isfinite(loss).item()
        assert len(sites) > 4, task
        assert sites[0][0] == 0
        for (off, n), (nxt, _) in zip(sites, sites[1:]):
            assert n > 0 and nxt == off + n, (task, off, n, nxt)
        assert all(n < 2 ** 32 for _, n in sites)
        keys = [R.dropout_key(ops.RT.seed, off, R.salt_word(step_seed)) for off, _ in sites]
        nxt_keys = [R.dropout_key(ops.RT.seed, off, R.salt_word(step_seed + 1)) for off, _ in sites]
        print(f"{task}: {len(sites)} dropout sites, {sites[-1][0] + sites[-1][1]} elements")
        assert len(set(keys)) == len(keys), task
        assert all(k != k2 for k, k2 in zip(keys, nxt_keys)) and not set(keys) & set(nxt_keys), task
    torch.cuda.synchronize()
