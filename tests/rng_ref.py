"""Host restatement of the device random streams (csrc/common.h "counter-based dropout RNG" and the draws of
bevbert_nav_action, bevbert_wp_candidates and bevbert_ce_update), in vectorised numpy uint32.  Written from the comments
of common.h, include/bevbert_hip.h and the kernels; it imports nothing from the package, so a test that compares a kernel
with it compares the kernel with the specification and not with the library's own helpers.

One 32-bit mix serves everything:

    hash32(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          ("lowbias32")

Keys.  ``salt`` below is the step's salt word (``salt_word(step_seed)``), or None when no salt is registered.

    site_key(seed, offset) = hash(hash(hash(hash(lo(seed) ^ 0x9e3779b9) ^ hi(seed)) ^ lo(offset)) ^ hi(offset))
    salted(key)            = hash(key ^ salt)                (key itself without a salt)
    dropout site           k = salted(site_key(seed, offset))
    nav action draws       k = salted(hash(site_key(seed, t) ^ STREAM_NAV))
    waypoint draws         k = salted(hash(site_key(seed, t) ^ STREAM_WAYPOINT))
    ghost noise            k = salted(hash(hash(seed ^ 0x9e3779b9) ^ STREAM_GHOST))

Draws.

    dropout   element j: bits = hash(k ^ (j >> 1)); its 16 bits are the low half for even j, the high half for odd j;
              keep iff bits16 >= drop_threshold(p)
    nav       u0(b) = uniform24(hash(k ^ 4 b)), u1(b) = uniform24(hash(k ^ (4 b + 1)))
    waypoint  u(b, c) = uniform24(hash(k ^ (8 b + c))), c < 5
    ghost     kb = hash(hash(k ^ step_id) ^ b); kg = hash(kb ^ g); u1 = ((hash(kg ^ 1) >> 8) + 1) / 2^24 in (0, 1],
              u2 = (hash(kg ^ 2) >> 8) / 2^24 in [0, 1); r = sqrt(-2 ln u1) aug; (nx, nz) = clip(r (cos, sin)(2 pi u2), +-aug)
"""
import numpy as np

GOLDEN_RATIO = 0x9E3779B9
STREAM_NAV = 0x6E617631
STREAM_WAYPOINT = 0x77617970
STREAM_GHOST = 0x67687374
WP_KMAX = 5
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def hash32(x):
    """lowbias32 of a uint32 array (or a Python int: returned as a uint32 scalar array)."""
    x = np.array(x, dtype=np.uint64).astype(np.uint32) if not isinstance(x, np.ndarray) else x.astype(np.uint32)
    with np.errstate(over="ignore"):                     # the products wrap modulo 2^32, as on the device
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        return x ^ (x >> np.uint32(16))


def _h(x):
    return int(hash32(int(x) & _M32))


def site_key(seed64, offset64):
    seed64, offset64 = int(seed64) & _M64, int(offset64) & _M64
    k = _h((seed64 & _M32) ^ GOLDEN_RATIO)
    k = _h(k ^ (seed64 >> 32))
    k = _h(k ^ (offset64 & _M32))
    return _h(k ^ (offset64 >> 32))


def drop_threshold(p):
    """round(p * 2^16) in float32 arithmetic, clamped to [0, 65535]."""
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    if t <= np.float32(0.0):
        return 0
    return 65535 if t >= np.float32(65535.0) else int(t)


def salt_word(step_seed):
    """The 32-bit word the host writes for a step: hash(hash(lo(step_seed)) ^ hi(step_seed))."""
    step_seed = int(step_seed) & _M64
    return _h(_h(step_seed & _M32) ^ (step_seed >> 32))


def salted(key, salt):
    return int(key) & _M32 if salt is None else _h((int(key) ^ (int(salt) & _M32)) & _M32)


def stream_key(key, domain):
    return _h(int(key) ^ domain)


def dropout_key(seed, offset, salt):
    return salted(site_key(seed, offset), salt)


def dropout_pair_inputs(n_pairs, seed, offset, salt):
    """The words the dropout site hashes for its first ``n_pairs`` element pairs."""
    return np.arange(n_pairs, dtype=np.uint32) ^ np.uint32(dropout_key(seed, offset, salt))


def keep_mask(n, p, seed, offset, salt):
    """Keep mask (bool, n) of a dropout site; element indices are below 2^32."""
    bits = hash32(dropout_pair_inputs((int(n) + 1) // 2, seed, offset, salt))
    halves = np.stack([bits & np.uint32(0xFFFF), bits >> np.uint32(16)], axis=1).reshape(-1)[:int(n)]
    return halves >= np.uint32(drop_threshold(p))


def uniform24(word):
    """(h >> 8) * 2^-24 as float32: the top 24 bits of a hashed word, in [0, 1)."""
    return (np.asarray(word, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---------------------------------------------------------------------------------------------------------- nav action
def nav_key(seed, t, salt):
    return salted(stream_key(site_key(int(seed) & _M32, t), STREAM_NAV), salt)


def nav_inputs(B, seed, t, salt):
    """(B, 2) words hashed for u0 and u1."""
    b = np.arange(B, dtype=np.uint32) * np.uint32(4)
    return np.stack([b, b + np.uint32(1)], axis=1) ^ np.uint32(nav_key(seed, t, salt))


def nav_uniforms(B, seed, t, salt):
    u = uniform24(hash32(nav_inputs(B, seed, t, salt)))
    return u[:, 0], u[:, 1]


# ------------------------------------------------------------------------------------------------------------ waypoint
def waypoint_key(seed, t, salt):
    return salted(stream_key(site_key(int(seed) & _M32, t), STREAM_WAYPOINT), salt)


def waypoint_inputs(B, seed, t, salt):
    """(B, 5) words hashed for u(b, c)."""
    w = np.arange(B, dtype=np.uint32)[:, None] * np.uint32(8) + np.arange(WP_KMAX, dtype=np.uint32)[None]
    return w ^ np.uint32(waypoint_key(seed, t, salt))


def waypoint_uniforms(B, seed, t, salt):
    return uniform24(hash32(waypoint_inputs(B, seed, t, salt)))


# --------------------------------------------------------------------------------------------------------- ghost noise
def ghost_key(seed, salt):
    return salted(stream_key(_h((int(seed) & _M32) ^ GOLDEN_RATIO), STREAM_GHOST), salt)


def ghost_chain(B, G, seed, step_id, salt):
    """Every word the ghost noise of maps 0..B-1, ghosts 0..G-1 hashes at one step: dict of uint32 arrays
    "step" (1), "map" (B), "ghost" (B, G), "u1" (B, G), "u2" (B, G)."""
    w_step = np.array([ghost_key(seed, salt) ^ (int(step_id) & _M32)], dtype=np.uint32)
    w_map = hash32(w_step) ^ np.arange(B, dtype=np.uint32)
    w_ghost = hash32(w_map)[:, None] ^ np.arange(G, dtype=np.uint32)[None]
    kg = hash32(w_ghost)
    return {"step": w_step, "map": w_map, "ghost": w_ghost, "u1": kg ^ np.uint32(1), "u2": kg ^ np.uint32(2)}


def ghost_noise(B, G, seed, step_id, salt, aug):
    """(nx, nz), each (B, G) float64: Box-Muller in fp64 scaled by ``aug`` and clipped to +-aug."""
    c = ghost_chain(B, G, seed, step_id, salt)
    u1 = ((hash32(c["u1"]) >> np.uint32(8)).astype(np.float64) + 1.0) * (1.0 / 16777216.0)
    u2 = (hash32(c["u2"]) >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)
    r = np.sqrt(-2.0 * np.log(u1)) * aug
    two_pi = 6.283185307179586
    return np.clip(r * np.cos(two_pi * u2), -aug, aug), np.clip(r * np.sin(two_pi * u2), -aug, aug)
