"""numpy restatement of bsx_gae (include/battlespace_hip.h; csrc/bsx_advantage.hip): GAE(gamma, lambda) over a rollout's records,
column-vectorised, float32 operation for operation (each rounded on its own, as the kernel is built with -ffp-contract=off), the
normalisation in float64 -- numpy's own mean / std, or (kernel_order=True) the kernel's moments merged in the kernel's order, to the bit.
`agents` restates bsx_gae_agents: an agent that is flagged off has no decisions."""
import numpy as np

# csrc/bsx_advantage.hip: lanes per tile, ticks per chunk, threads of the merge workgroup (tests/test_advantage_cpu.py reads the file and
# compares).  stats_in_kernel_order follows the kernel's structure, so it is no independent reference: what makes it one is that the same
# CPU test holds it to numpy's own mean / std within 1e-12 -- it may differ from them by summation order only.
WAVE, U, MERGE_TPB = 64, 8, 256


def _chan(n, mean, m2, nb, mb, m2b):
    """chan_merge of the kernel on float64 arrays: (n, mean, M2) merged with (nb, mb, m2b); an empty side leaves the other unchanged."""
    with np.errstate(all="ignore"):
        nn, d = n + nb, mb - mean
        mean2 = mean + d * (nb / nn)
        m22 = (m2 + m2b) + (d * d) * ((n * nb) / nn)
    keep, take = nb == 0.0, (n == 0.0) & (nb != 0.0)
    return (np.where(keep, n, np.where(take, nb, nn)), np.where(keep, mean, np.where(take, mb, mean2)),
            np.where(keep, m2, np.where(take, m2b, m22)))


def _tree(n, mean, m2, width):
    """The halving tree over the last axis (lane i takes lane i + off, off = width / 2 .. 1): element 0 holds the result."""
    off = width // 2
    while off > 0:
        a = _chan(n[..., :off], mean[..., :off], m2[..., :off], n[..., off:2 * off], mean[..., off:2 * off], m2[..., off:2 * off])
        n, mean, m2 = (np.concatenate([x, y[..., off:]], -1) for x, y in zip(a, (n, mean, m2)))
        off //= 2
    return n[..., 0], mean[..., 0], m2[..., 0]


def stats_in_kernel_order(adv, mask):
    """(n, mean, unbiased std) of the masked advantages as bsx_gae's three kernels compute them: per lane (4 adjacent columns, 2 where
    E*A is no multiple of 4) chunks of 8 ticks from T-1 down -- count, sum, then squares around the chunk's mean, ticks descending and
    columns ascending -- merged by Chan's formula; the 64 lanes of a tile by a halving tree; the tiles by thread (tile i to thread
    i mod 256, in order) and another halving tree.  Every operation is float64, rounded on its own."""
    T = adv.shape[0]
    C = int(np.prod(adv.shape[1:]))
    W = 4 if C % 4 == 0 else 2
    NW = C // W
    x, m = np.asarray(adv, np.float32).reshape(T, NW, W).astype(np.float64), np.asarray(mask).astype(bool).reshape(T, NW, W)
    sn, sm, s2 = np.zeros(NW), np.zeros(NW), np.zeros(NW)
    for t0 in range(T - 1, -1, -U):
        ticks = range(t0, max(t0 - U, -1), -1)
        cn, cs = np.zeros(NW), np.zeros(NW)
        for t in ticks:
            for j in range(W):
                cn = cn + m[t, :, j]
                cs = cs + np.where(m[t, :, j], x[t, :, j], 0.0)
        with np.errstate(all="ignore"):
            cm = cs / cn
        c2 = np.zeros(NW)
        for t in ticks:
            for j in range(W):
                d = x[t, :, j] - cm
                c2 = c2 + np.where(m[t, :, j], d * d, 0.0)
        sn, sm, s2 = _chan(sn, sm, s2, cn, np.where(cn > 0, cm, 0.0), c2)
    tiles = -(-NW // WAVE)
    pad = lambda v: np.concatenate([v, np.zeros(tiles * WAVE - NW)]).reshape(tiles, WAVE)   # noqa: E731
    tn, tm, t2 = _tree(pad(sn), pad(sm), pad(s2), WAVE)
    rounds = -(-tiles // MERGE_TPB)
    pad = lambda v: np.concatenate([v, np.zeros(rounds * MERGE_TPB - tiles)]).reshape(rounds, MERGE_TPB)   # noqa: E731
    tn, tm, t2 = pad(tn), pad(tm), pad(t2)
    n, mean, m2 = np.zeros(MERGE_TPB), np.zeros(MERGE_TPB), np.zeros(MERGE_TPB)
    for r in range(rounds):
        n, mean, m2 = _chan(n, mean, m2, tn[r], tm[r], t2[r])
    n, mean, m2 = (float(v) for v in _tree(n, mean, m2, MERGE_TPB))
    return n, mean, (float(np.sqrt(np.float64(m2) / np.float64(n - 1.0))) if n >= 2.0 else 0.0)


def gae_ref(rew, value, last_value, done, env_done, done_prev, gamma, lam, normalize=False, agents=None, kernel_order=False):
    """rew, value f32 [T, E, A]; done [T, E, A] and env_done [T(+1), E] flags; last_value f32 [E, A]; done_prev flags [E, A].
    agents: flags [A] or None -- a column whose flag is 0 has no decisions (mask 0, adv = ret = +0, out of the statistics); its carry is
    still updated.  kernel_order: the normalisation's statistics in the kernel's own summation order (stats_in_kernel_order).
    -> (adv f32, ret f32, mask bool [T, E, A], done_prev' uint8 [E, A], stats f64 [3] or None)."""
    rew, value = np.asarray(rew, np.float32), np.asarray(value, np.float32)
    T, E, A = rew.shape
    done = np.asarray(done).astype(bool)
    env_done = np.asarray(env_done).astype(bool)[:T]
    prev = np.asarray(done_prev).astype(bool)
    lv = np.asarray(last_value, np.float32)
    g, gl = np.float32(gamma), np.float32(np.float32(gamma) * np.float32(lam))
    on = np.ones(A, bool) if agents is None else np.asarray(agents).astype(bool).reshape(A)
    zero = np.zeros((E, A), np.float32)
    adv = np.zeros((T, E, A), np.float32)
    ret = np.zeros((T, E, A), np.float32)
    mask = np.zeros((T, E, A), bool)
    for t in range(T - 1, -1, -1):
        before = prev if t == 0 else done[t - 1]
        m = ~env_done[t][:, None] & ~before & on
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
        if kernel_order:
            n, mean, std = stats_in_kernel_order(adv, mask)
            assert n == x.size
        else:
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
