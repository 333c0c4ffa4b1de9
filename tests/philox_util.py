"""A host restatement of the in-kernel Philox draws that the step's C oracle does not cover: the actor's exploration normals and
categorical uniforms (csrc/bsx_actor_core.h: normals4 / uniforms4), the continuous scripted opponent's draws (csrc/bsx_instinct.h:
instinct_continuous_draws) and the replay sampler's indices (csrc/bsx_replay.hip).  Vectorised numpy, so the GPU tests can compare
the kernels with it exactly where the arithmetic allows (integer words, float32 uniforms, the opponent's binary64 values) and against
float64 where it does not (Box-Muller, Gumbel).  Used by tests/test_hip_rng_restated.py (GPU) and tests/test_philox_restated_cpu.py (CPU)."""
import functools

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SALT_OU = 0x00000000                 # normals4: the OU increment, or the Gaussian term on its own
SALT_GAUSS_WITH_OU = 0x80000000      # normals4: the Gaussian term when the OU process is on too
SALT_CATEGORICAL = 0x40000000        # uniforms4: the Gumbel draws of the categorical policy head
ACTOR_KEY_XOR = 0xA5A5A5A5
OPPONENT_CTR_XOR = 0x10000000
SAMPLER_KEY_XOR = 0x5EED5A3C


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """bsx_actor::philox4x32_10 on arrays (broadcast): four uint32 counter words and two key words in, the four uint32 output words out.
    Each round: (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)), then the key moves by the Weyl constants."""
    c = [np.asarray(x, np.uint64) & MASK for x in (c0, c1, c2, c3)]
    c = np.broadcast_arrays(*c)
    c0, c1, c2, c3 = (x.copy() for x in c)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def _split(x):
    x = np.asarray(x, np.uint64)
    return x & MASK, x >> np.uint64(32)


def actor_words(seed, seq, grow, salt):
    """The actor's block for job-wide rows `grow` = (env_offset + e) * A + a at sequence number `seq` (the call's seq + *seq_base):
    counter (grow, grow >> 32, seq, (seq >> 32) ^ salt), key (seed, (seed >> 32) ^ 0xA5A5A5A5)."""
    g_lo, g_hi = _split(grow)
    seq, seed = int(seq), int(seed)
    return philox4x32_10(g_lo, g_hi, seq & 0xFFFFFFFF, (seq >> 32) ^ salt, seed & 0xFFFFFFFF, (seed >> 32) ^ ACTOR_KEY_XOR)


def opponent_words(seed, seq, g):
    """instinct_continuous_draws' block for job-wide row g: counter (g, (g >> 32) ^ 0x10000000, seq, seq >> 32), key (seed, seed >> 32)."""
    g_lo, g_hi = _split(g)
    seq, seed = int(seq), int(seed)
    return philox4x32_10(g_lo, g_hi ^ np.uint64(OPPONENT_CTR_XOR), seq & 0xFFFFFFFF, seq >> 32, seed & 0xFFFFFFFF, seed >> 32)


def sampler_words(seed, seq, b):
    """The replay sampler's block for batch position b: counter (b, b >> 32, seq, seq >> 32), key (seed, (seed >> 32) ^ 0x5EED5A3C)."""
    b_lo, b_hi = _split(b)
    seq, seed = int(seq), int(seed)
    return philox4x32_10(b_lo, b_hi, seq & 0xFFFFFFFF, seq >> 32, seed & 0xFFFFFFFF, (seed >> 32) ^ SAMPLER_KEY_XOR)


def uniform23(r):
    """uniforms4's mapping of one word, in float32 as the kernel computes it: (float(r >> 9) + 0.5f) * 2^-23.  Every step is exact,
    so the values are the odd multiples of 2^-24, strictly inside (0, 1) and strictly increasing with the code r >> 9."""
    code = (np.asarray(r, np.uint32) >> np.uint32(9)).astype(np.float32)
    return (code + np.float32(0.5)) * np.float32(2.0 ** -23)


def uniforms4(seed, seq, grow, salt=SALT_CATEGORICAL):
    """The categorical head's four uniforms per row: float32 [..., 4], bit for bit."""
    return np.stack([uniform23(w) for w in actor_words(seed, seq, grow, salt)], -1)


def normals4(seed, seq, grow, salt):
    """normals4 restated: the float32 uniforms exactly as the kernel forms them, then Box-Muller in float64 (the kernel's __logf /
    __sincosf are approximations, so this is the value it approximates).  float64 [..., 4]."""
    r = actor_words(seed, seq, grow, salt)
    k = np.float32(2.0 ** -24)
    u0 = ((r[0] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * k
    u1 = (r[1] >> np.uint32(8)).astype(np.float32) * k
    u2 = ((r[2] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * k
    u3 = (r[3] >> np.uint32(8)).astype(np.float32) * k
    m0, m1 = np.sqrt(-2.0 * np.log(u0.astype(np.float64))), np.sqrt(-2.0 * np.log(u2.astype(np.float64)))
    t1 = np.float32(6.2831853071795864) * u1                     # the kernel's float32 product (exact to a rounding), then exact sin / cos
    t3 = np.float32(6.2831853071795864) * u3
    t1, t3 = t1.astype(np.float64), t3.astype(np.float64)
    return np.stack([m0 * np.cos(t1), m0 * np.sin(t1), m1 * np.cos(t3), m1 * np.sin(t3)], -1)


def opponent_draws(seed, seq, g):
    """(r0, n0, n1, n2) float64 [..., 4] for job-wide rows g, in the kernel's order of operations: bit for bit."""
    r = opponent_words(seed, seq, g)
    s = 1.0 / 4294967296.0
    r0 = r[0].astype(np.float64) * s
    n = [-0.15 + 0.3 * (w.astype(np.float64) * s) for w in r[1:]]
    return np.stack([r0, *n], -1)


def sampler_indices(seed, seq, B, M, counter):
    """The rows sample() draws: idx[b] = (w.x * max_mem) >> 32, max_mem = clamp(counter, 0, M).  int64 [B]."""
    max_mem = np.uint64(min(max(int(counter), 0), int(M)))
    w = sampler_words(seed, seq, np.arange(B, dtype=np.uint64))[0].astype(np.uint64)
    return ((w * max_mem) >> np.uint64(32)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def edge_rows(seed, seq, salt, g0, count, chunk=1 << 21):
    """Scan job-wide rows [g0, g0 + count) of the actor's stream (seed, seq, salt) for words at the ends of the 24-bit code:
    returns (top, bottom), each a tuple of (grow, component) with r >> 8 == 0xFFFFFF (top; then also r >> 9 == 0x7FFFFF, the
    top code of uniforms4) and r >> 8 == 0 (bottom).  About two of each per 2^23 rows; deterministic for fixed arguments."""
    top, bottom = [], []
    for s in range(g0, g0 + count, chunk):
        g = np.arange(s, min(s + chunk, g0 + count), dtype=np.uint64)
        for comp, w in enumerate(actor_words(seed, seq, g, salt)):
            code = w >> np.uint32(8)
            top += [(int(x), comp) for x in g[code == 0xFFFFFF]]
            bottom += [(int(x), comp) for x in g[code == 0]]
    return tuple(sorted(top)), tuple(sorted(bottom))
