"""A host restatement of the epsilon-greedy row finish (csrc/bsx_actor_core.h, finish_row with BsxActorNoise.epsilon) and of the linear
annealing schedule (csrc/bsx_explore.hip), in numpy, on tests/philox_util.uniforms4 with the rule's own salt.  The GPU is held to it bit
for bit (tests/test_hip_epsilon.py); tests/test_epsilon_cpu.py checks its statistics once."""
import numpy as np

import philox_util as P

EPS_SALT = 0x20000000
ONE_HOT = np.where(np.eye(4, dtype=bool), np.float32(1.0), np.float32(-1.0))       # bsx_instinct.h one_hot_scores, row = action


def draws(seed, seq, grow, u=None):
    """(explore-deciding uniform u.x, random action int(u.y * 4.0f)) for job-wide rows `grow` at sequence number `seq`; u: injected
    uniforms float32 [..., 4] instead of the Philox block."""
    if u is None:
        u = P.uniforms4(seed, seq, grow, EPS_SALT)
    u = np.asarray(u, np.float32)
    return u[..., 0], (u[..., 1] * np.float32(4.0)).astype(np.int32)


def apply(greedy, epsilon, seed, seq, env_offset=0, u=None):
    """The rule on greedy score rows float32 [E, A, 4] with per-plane rates epsilon float32 [A]: -> (scores [E, A, 4], explored uint8
    [E, A]).  A row explores iff u.x < epsilon[a] in float32 (a NaN compares false); an exploring row becomes the one-hot +-1 row of its
    random action, every other row stays as it is, bit for bit."""
    greedy = np.asarray(greedy, np.float32)
    E, A = greedy.shape[:2]
    grow = (np.uint64(env_offset) + np.arange(E, dtype=np.uint64))[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]
    ux, act = draws(seed, seq, grow, u)
    with np.errstate(invalid="ignore"):
        explored = ux < np.asarray(epsilon, np.float32)[None, :]
    out = np.where(explored[..., None], ONE_HOT[act], greedy)
    return out, explored.astype(np.uint8)


def schedule(count, start, end, steps, kind="linear"):
    """bsx_epsilon_advance's value at the (new) count, float32: binary64 operations each rounded on their own, one rounding to float32.
    The linear kind is what the kernel computes bit for bit; the exponential kind is numpy's exp, which the device's is measured against."""
    x = float(count) / float(steps)
    f = max(0.0, 1.0 - x) if kind == "linear" else float(np.exp(-x))
    return np.float32(end + (start - end) * f)
