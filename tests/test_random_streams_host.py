"""The specification of the device random streams, checked on the host (tests/rng_ref.py; no GPU).

* the salt word the runtime writes for a step equals the restatement;
* the keep mask of the specification has the keep rate of its 16-bit threshold, independent halves of a pair, and no
  correlation with itself at the lags the kernels stride by, with another site of the step, with the same site under
  another step seed, or with the same site on the other rank;
* the words the nav, waypoint, ghost and dropout consumers hash under one (seed, t, step seed) are pairwise disjoint.

Sites of 2^22 elements, p in {0.1, 0.3, 0.5}, 4 step seeds x 3 offsets (i * 2^22) = 12 sites per p, seed = _Runtime.SEED.
Sampling noise of a correlation at this size is 2^-11 = 4.9e-4.  Measured worst values of the restatement (the bound of
every correlation is 1e-2, about twice the worst; a shared or repeated mask, halves cut from overlapping bits, or a
site / step / rank that ignores its key give 0.1 or more):

    statistic                                    worst over the 12 sites at p = 0.1 / 0.3 / 0.5     bound
    keep rate, |z|                               1.65 / 2.61 / 1.91 sigma                           6 sigma
    both halves of a pair dropped, |z|           2.21 / 2.18 / 1.44 sigma                           6 sigma
    |corr| at lags 1, 2, 3, 4                    1.5e-3 / 1.2e-3 / 1.7e-3                           1e-2
    |corr| at lag 64                             1.4e-3 / 9.4e-4 / 1.4e-3                           1e-2
    |corr| at lag 448                            7.9e-4 / 8.3e-4 / 1.0e-3                           1e-2
    |corr| at lag 768                            2.6e-3 / 3.2e-3 / 3.0e-3                           1e-2
    |corr| at the other multiples of 128         3.8e-3 (lag 1536) / 3.1e-3 (1536) / 3.5e-3 (256)   1e-2
    |corr| two sites of one step                 9.4e-4 / 1.2e-3 / 1.1e-3                           1e-2
    |corr| same site, two step seeds             5.8e-4 / 6.4e-4 / 7.7e-4                           1e-2
    |corr| same site, the two ranks' step seeds  4.6e-4 / 1.1e-3 / 1.8e-4                           1e-2

The worst of all, 3.8e-3, is below 5e-3, so the bound 1e-2 is at least twice the reference's worst value.

The lags that are multiples of 128 carry a small systematic correlation (up to 8 standard errors): a property of the
mix on strided counters, noted next to bb_hash32 in csrc/common.h.  Far too small to matter for dropout; recorded, not
fixed."""
import types

import numpy as np
import pytest

from tests import rng_ref as R

STEP_SEEDS = [0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 12345]
N = 1 << 22
PS = (0.1, 0.3, 0.5)
LAGS = (1, 2, 3, 4, 64, 128, 256, 384, 448, 512, 768, 1024, 1536, 3072)
SITE_STEP_SEEDS = (3, 1000003 + 3, 2 ** 32 + 3, 2 ** 63 + 12345)
CORR_BOUND = 1e-2


def _rank_step_seeds(global_step=17, seed=0):
    from vln_bevbert_amd.train import PretrainTrainer
    return [PretrainTrainer._step_seed(types.SimpleNamespace(seed=seed, rank=r, global_step=global_step)) for r in (0, 1)]


# ------------------------------------------------------------------------------------------------------------ salt word
def test_runtime_salt_word_equals_the_restatement():
    from vln_bevbert_amd.ops_core import RT
    seeds = STEP_SEEDS + _rank_step_seeds()
    assert _rank_step_seeds()[0] != _rank_step_seeds()[1]
    for s in seeds:
        got = RT.salt_word(s)
        assert -(1 << 31) <= got < (1 << 31)                 # the int32 bit pattern of the fill
        assert got & 0xFFFFFFFF == R.salt_word(s), hex(s)
    # the high half of the step seed reaches the word
    assert len({R.salt_word(s) for s in seeds}) == len(seeds)


def test_threshold_is_the_rounded_16_bit_fraction_with_both_clamps():
    assert [R.drop_threshold(p) for p in (0.0, 1e-5, 0.1, 0.3, 0.5, 0.99999, 1.0)] == [0, 1, 6554, 19661, 32768, 65535, 65535]


# ------------------------------------------------------------------------------------------------------------ statistics
def _corr(a, b):
    """Pearson correlation of two boolean arrays, from exact counts."""
    n = a.size
    na, nb, nab = int(np.count_nonzero(a)), int(np.count_nonzero(b)), int(np.count_nonzero(a & b))
    return (n * nab - na * nb) / np.sqrt(float(na) * (n - na) * nb * (n - nb))


@pytest.fixture(scope="module")
def seed():
    from vln_bevbert_amd.ops_core import _Runtime
    return _Runtime.SEED


@pytest.fixture(scope="module")
def halves(seed):
    """The 16 random bits of every element of the 12 sites (step seed, offset index) -> uint16 (N)."""
    out = {}
    for s in SITE_STEP_SEEDS:
        for i in range(3):
            bits = R.hash32(R.dropout_pair_inputs(N // 2, seed, i * N, R.salt_word(s)))
            out[s, i] = np.stack([bits & np.uint32(0xFFFF), bits >> np.uint32(16)], axis=1).reshape(-1).astype(np.uint16)
    return out


def test_halves_fixture_is_the_keep_mask_of_the_restatement(halves, seed):
    s, i = SITE_STEP_SEEDS[1], 2
    for p in PS:
        assert np.array_equal(halves[s, i][:4097] >= R.drop_threshold(p), R.keep_mask(4097, p, seed, i * N, R.salt_word(s)))


@pytest.mark.parametrize("p", PS)
def test_keep_rate_and_pair_independence(halves, p):
    thr = R.drop_threshold(p)
    q = thr / 65536.0
    worst = [0.0, 0.0]
    for key, h in halves.items():
        keep = h >= thr
        z_keep = (keep.mean() - (1 - q)) / np.sqrt(q * (1 - q) / N)
        both = ~keep[0::2] & ~keep[1::2]
        z_both = (both.mean() - q * q) / np.sqrt(q * q * (1 - q * q) / (N // 2))
        worst = [max(worst[0], abs(z_keep)), max(worst[1], abs(z_both))]
        assert abs(z_keep) < 6 and abs(z_both) < 6, (key, z_keep, z_both)
    print(f"p={p}: worst |z| keep rate {worst[0]:.2f}, both halves dropped {worst[1]:.2f}")


@pytest.mark.parametrize("p", PS)
def test_mask_has_no_autocorrelation_at_the_strides_of_the_kernels(halves, p):
    thr = R.drop_threshold(p)
    worst = dict.fromkeys(LAGS, 0.0)
    for key, h in halves.items():
        keep = h >= thr
        for lag in LAGS:
            c = _corr(keep[:-lag], keep[lag:])
            worst[lag] = max(worst[lag], abs(c))
            assert abs(c) < CORR_BOUND, (key, lag, c)
    print(f"p={p}: worst |corr| per lag " + " ".join(f"{k}:{v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("p", PS)
def test_sites_steps_and_ranks_draw_uncorrelated_masks(halves, seed, p):
    thr = R.drop_threshold(p)
    worst = {"sites": 0.0, "steps": 0.0, "ranks": 0.0}
    for s in SITE_STEP_SEEDS:
        for i, j in ((0, 1), (0, 2), (1, 2)):
            worst["sites"] = max(worst["sites"], abs(_corr(halves[s, i] >= thr, halves[s, j] >= thr)))
    for i in range(3):
        for a in range(len(SITE_STEP_SEEDS)):
            for b in range(a + 1, len(SITE_STEP_SEEDS)):
                c = _corr(halves[SITE_STEP_SEEDS[a], i] >= thr, halves[SITE_STEP_SEEDS[b], i] >= thr)
                worst["steps"] = max(worst["steps"], abs(c))
    r0, r1 = _rank_step_seeds()
    for i in range(3):
        m0, m1 = (R.keep_mask(N, p, seed, i * N, R.salt_word(r)) for r in (r0, r1))
        worst["ranks"] = max(worst["ranks"], abs(_corr(m0, m1)))
    print(f"p={p}: worst |corr| " + " ".join(f"{k}:{v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) < CORR_BOUND, worst


def test_the_statistics_would_catch_a_repeated_or_shared_mask(halves):
    """The gates above against the failures they are there for (each gives |corr| >= 0.1)."""
    h = halves[SITE_STEP_SEEDS[0], 0]
    keep = h >= R.drop_threshold(0.1)
    rows = np.tile(keep[:768], N // 768)                                   # one row's mask in every row
    assert abs(_corr(rows[:-768], rows[768:])) > 0.9
    assert abs(_corr(keep, keep.copy())) > 0.9                             # a site / step / rank that ignores its key
    same = np.repeat(h[0::2], 2) >= R.drop_threshold(0.5)                  # both halves of a pair from the same 16 bits
    assert abs(_corr(same[:-1], same[1:])) > 0.1
    windows = h.copy()                                                     # ... or from windows sharing their top 4 bits
    windows[1::2] = (h[0::2] & 0xF000) | (h[1::2] & 0x0FFF)
    windows = windows >= R.drop_threshold(0.3)
    assert abs(_corr(windows[:-1], windows[1:])) > 0.1
    trunc = h >= (R.drop_threshold(0.1) >> 8 << 8)                         # an 8-bit threshold: 26/256 for p = 0.1
    q = R.drop_threshold(0.1) / 65536.0
    assert abs(trunc.mean() - (1 - q)) / np.sqrt(q * (1 - q) / N) > 6


# ------------------------------------------------------------------------------------------------- consumer separation
@pytest.mark.parametrize("step_seed", [11, 2 ** 32 + 3])
@pytest.mark.parametrize("t", [0, 3])
def test_consumers_of_one_step_hash_disjoint_words(step_seed, t):
    """nav (B = 64), waypoint (B = 64 x 5), the ghost chain (B = 4 x 16 ghosts) and the first 1024 pair words of the
    dropout site at offset 0 -- all with the entry points' default seed 0, the same t and one step salt.  Before the
    domain constants the nav and waypoint sets overlapped (waypoint (b, 0) = nav u0 of sample 2 b), and both overlapped
    the dropout site whose offset equals t."""
    seed, salt = 0, R.salt_word(step_seed)
    ghost = R.ghost_chain(4, 16, seed, t + 1, salt)
    sets = {"nav": R.nav_inputs(64, seed, t, salt), "waypoint": R.waypoint_inputs(64, seed, t, salt),
            "ghost": np.concatenate([v.reshape(-1) for v in ghost.values()]),
            "dropout": R.dropout_pair_inputs(1024, seed, 0, salt),
            "dropout@t": R.dropout_pair_inputs(1024, seed, t, salt)}
    sets = {k: set(int(x) for x in np.asarray(v).reshape(-1)) for k, v in sets.items()}
    assert len(sets["nav"]) == 128 and len(sets["waypoint"]) == 320 and len(sets["dropout"]) == 1024
    assert len(sets["ghost"]) == 1 + 4 + 3 * 64
    names = list(sets)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if {a, b} == {"dropout", "dropout@t"}:
                continue                                  # one consumer (and the same site for t = 0)
            assert not (sets[a] & sets[b]), (a, b, len(sets[a] & sets[b]))
