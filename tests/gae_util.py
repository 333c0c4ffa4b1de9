"""numpy restatement of bsx_gae (include/battlespace_hip.h; csrc/bsx_advantage.hip): GAE(gamma, lambda) over a rollout's records,
column-vectorised, float32 operation for operation (each rounded on its own, as the kernel is built with -ffp-contract=off), the
normalisation in float64."""
import numpy as np


def gae_ref(rew, value, last_value, done, env_done, done_prev, gamma, lam, normalize=False):
    """rew, value f32 [T, E, A]; done [T, E, A] and env_done [T(+1), E] flags; last_value f32 [E, A]; done_prev flags [E, A].
    -> (adv f32, ret f32, mask bool [T, E, A], done_prev' uint8 [E, A], stats f64 [3] or None)."""
    rew, value = np.asarray(rew, np.float32), np.asarray(value, np.float32)
    T, E, A = rew.shape
    done = np.asarray(done).astype(bool)
    env_done = np.asarray(env_done).astype(bool)[:T]
    prev = np.asarray(done_prev).astype(bool)
    lv = np.asarray(last_value, np.float32)
    g, gl = np.float32(gamma), np.float32(np.float32(gamma) * np.float32(lam))
    zero = np.zeros((E, A), np.float32)
    adv = np.zeros((T, E, A), np.float32)
    ret = np.zeros((T, E, A), np.float32)
    mask = np.zeros((T, E, A), bool)
    for t in range(T - 1, -1, -1):
        before = prev if t == 0 else done[t - 1]
        m = ~env_done[t][:, None] & ~before
        term = done[t]
        nv = np.where(term, zero, lv if t == T - 1 else value[t + 1])
        an = np.where(term, zero, zero if t == T - 1 else adv[t + 1])
        delta = (rew[t] + g * nv) - value[t]
        a = delta + gl * an
        adv[t] = np.where(m, a, zero)
        ret[t] = np.where(m, a + value[t], zero)
        mask[t] = m
    stats = None
    if normalize:
        x = adv[mask].astype(np.float64)
        n = x.size
        mean = float(x.mean()) if n else 0.0
        std = float(x.std(ddof=1)) if n >= 2 else 0.0
        if n:
            adv = adv.copy()
            adv[mask] = ((x - mean) / (std + 1e-8)).astype(np.float32)
        stats = np.array([n, mean, std], np.float64)
    return adv, ret, mask, done[T - 1].astype(np.uint8), stats


def textbook_gae(rew, value, last_value, dones, gamma, lam):
    """The usual float64 loop over one agent's episode (no mask): dones[t] = the episode ended at tick t."""
    T = len(rew)
    adv = np.zeros(T)
    last = 0.0
    for t in range(T - 1, -1, -1):
        nonterminal = 1.0 - float(dones[t])
        nv = last_value if t == T - 1 else value[t + 1]
        delta = rew[t] + gamma * nv * nonterminal - value[t]
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
    return adv, adv + np.asarray(value, np.float64)


def random_case(rng, T, E, A, p_done=0.1, p_env=0.1, p_prev=0.2):
    """Random records with random done, env_done and done_prev patterns (not game-consistent: the contract covers any input)."""
    rew = rng.standard_normal((T, E, A)).astype(np.float32)
    value = rng.standard_normal((T, E, A)).astype(np.float32)
    last_value = rng.standard_normal((E, A)).astype(np.float32)
    done = (rng.random((T, E, A)) < p_done).astype(np.uint8)
    env_done = (rng.random((T + 1, E)) < p_env).astype(np.uint8)
    done_prev = (rng.random((E, A)) < p_prev).astype(np.uint8)
    return rew, value, last_value, done, env_done, done_prev
