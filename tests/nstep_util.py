"""The n-step fold of csrc/bsx_replay_nstep.hip (include/battlespace_hip.h at BsxNstepCarry) restated in numpy, the ring it feeds, and
hand-made records that place every boundary case on purpose.

  fmaf32          float32 fmaf: through float64, where the product is exact, with the one double rounding that can happen (the float64
                  sum landing exactly between two float32 values) undone by the sum's exact residual
  gamma_chain     g_0 .. g_n of the kernel's chain of float32 products (g_n is NStepAppender.bootstrap_gamma)
  NStepRef        the fold and the carry on a team's own columns, in float32 (bit for bit the kernel's) or in float64
  RingRef         the ring's append: counter, wrap, only the newest M survive, stored
  make_run        a run of L ticks over E games whose games follow SCENARIOS; chunks() cuts it into rollout-shaped records
  guard_appender  re-homes an NStepAppender's staging and carry in guard slabs"""
import numpy as np

F32, F64 = np.float32, np.float64


def fmaf32(a, b, c):
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    p = a * b                                             # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                       # TwoSum: p + c = s + err exactly
    r = s.astype(F32)
    d = s - r.astype(F64)                                 # exact
    other = np.nextafter(r, np.where(d > 0, np.inf, -np.inf).astype(F32))
    with np.errstate(invalid="ignore", over="ignore"):
        tie = (d != 0) & (np.abs(d) == np.abs(other.astype(F64) - s))
    return np.where(tie & (np.sign(err) == np.sign(d)), other, r).astype(F32)


def gamma_chain(gamma, n, dtype=F32):
    g = [dtype(1.0)]
    for _ in range(n):
        g.append(dtype(g[-1] * dtype(gamma)))
    return g


class NStepRef:
    """State: the carry (n - 1 ticks, dense) and carry_valid.  fold() takes a team's own columns: obs [T + 1, E, nA, D], act [T, E, nA, k],
    rew [T, E, nA], done [T, E, nA], env_done [T + 1, E] -> dict of the T * E folded rows in (u, e) order (obs, obs_next, act, rew, done,
    skip, m) and moves the carry on.  dtype=float64: the same operations in float64 (a * b + c for the fmaf), for the recursion check."""

    def __init__(self, n, gamma, E, nA, D, k, dtype=F32):
        self.n, self.gamma, self.E, self.dtype = int(n), gamma, E, dtype
        c = self.n - 1
        self.c_obs, self.c_act = np.zeros((c, E, nA, D), F32), np.zeros((c, E, nA, k), F32)
        self.c_rew, self.c_done, self.c_ed = np.zeros((c, E, nA), F32), np.zeros((c, E, nA), np.uint8), np.zeros((c, E), np.uint8)
        self.valid = np.zeros(E, np.uint8)

    def reset_carry(self, mask=None):
        self.valid[slice(None) if mask is None else np.asarray(mask, bool)] = 0

    def fold(self, obs, act, rew, done, env_done):
        n, E, dt = self.n, self.E, self.dtype
        T = rew.shape[0]
        assert n <= T and obs.shape[0] == T + 1 and env_done.shape == (T + 1, E)
        obs_tl, act_tl = np.concatenate([self.c_obs, obs]), np.concatenate([self.c_act, act])
        rew_tl, done_tl = np.concatenate([self.c_rew, rew]), np.concatenate([self.c_done, np.asarray(done, np.uint8)]) != 0
        ed_tl = np.concatenate([self.c_ed, np.asarray(env_done, np.uint8)]) != 0
        g = gamma_chain(self.gamma, n, dt)
        out = dict(obs=obs_tl[:T].copy(), act=act_tl[:T].copy(), obs_next=np.empty_like(obs_tl[:T]), rew=np.empty((T, E, rew.shape[2]), dt),
                   done=np.empty(rew.shape, np.uint8), skip=np.empty((T, E), np.uint8), m=np.empty((T, E), np.int64))
        games = np.arange(E)
        for u in range(T):
            out["skip"][u] = ed_tl[u] | ((self.valid == 0) if u < n - 1 else False)
            m = np.full(E, n)
            for j in range(n - 1, -1, -1):
                m = np.where(ed_tl[u + j + 1], j + 1, m)
            R, dead = rew_tl[u].astype(dt), done_tl[u].copy()
            for j in range(1, n):
                inside = (j < m)[:, None]
                term = fmaf32(g[j], rew_tl[u + j], R) if dt is F32 else g[j] * rew_tl[u + j].astype(dt) + R
                R = np.where(inside & ~dead, term, R)
                dead = dead | (inside & done_tl[u + j])
            out["rew"][u], out["done"][u], out["m"][u] = R, dead | (m < n)[:, None], m
            out["obs_next"][u] = obs_tl[u + m, games]
        c = n - 1
        self.c_obs, self.c_act, self.c_rew = obs[T - c:T].copy(), act[T - c:T].copy(), rew[T - c:T].copy()
        self.c_done, self.c_ed = (np.asarray(done[T - c:T], np.uint8) != 0).astype(np.uint8), (np.asarray(env_done[T - c:T], np.uint8) != 0).astype(np.uint8)
        self.valid[:] = 1
        return {key: v.reshape(T * E, *v.shape[2:]) for key, v in out.items()}


RING_FIELDS = ("obs", "obs_next", "act", "rew", "done")


class RingRef:
    """M rows of (obs, obs_next [nA, D], act [nA, k], rew [nA], done [nA]); append(rows dict, skip) as bsx_replay_append: kept rows in
    order take ranks 0 .. R-1, rank j goes to row (counter + j) % M, only the newest M are written, counter += R; returns R."""

    def __init__(self, M, nA, D, k):
        self.M, self.counter = M, 0
        self.obs, self.obs_next = np.zeros((M, nA, D), F32), np.zeros((M, nA, D), F32)
        self.act, self.rew, self.done = np.zeros((M, nA, k), F32), np.zeros((M, nA), F32), np.zeros((M, nA), np.uint8)

    def append(self, rows, skip):
        keep = np.flatnonzero(np.asarray(skip) == 0)
        R = len(keep)
        for j in range(max(0, R - self.M), R):
            for f in RING_FIELDS:
                getattr(self, f)[(self.counter + j) % self.M] = rows[f][keep[j]]
        self.counter += R
        return R


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == F32 else a.astype(np.uint8)


def assert_ring_equal(buf, ring, what=""):
    """A DeviceReplayBuffer's five memories and counter against a RingRef, bit for bit."""
    got = dict(obs=buf.actor_states, obs_next=buf.actor_new_states, act=buf.action_mem, rew=buf.rew_mem, done=buf.done_mem)
    for f in RING_FIELDS:
        g = got[f].cpu().numpy()
        assert np.array_equal(bits(g), bits(getattr(ring, f))), (what, f, np.argwhere(bits(g) != bits(getattr(ring, f)))[:4])
    assert buf.mem_cntr == ring.counter, (what, buf.mem_cntr, ring.counter)


# What a game does over a run cut into rollouts of T ticks, by scenario -> (flag before tick 0, [ticks the game ends on], stays finished,
# (agent, tick) of an agent going down early or None).  A game that ends on tick g and does not stay finished re-spawns on tick g + 1: that
# tick starts on a finished game, so it is no transition (the auto-reset re-spawn right after an end).
SCENARIOS = ("ends on the carry's last tick", "ends on the rollout's first tick", "ends inside windows, at every j", "ends on the rollout's last tick",
             "inert: stays finished to the end", "an agent goes down ticks before its game ends", "finished before tick 0", "never ends")


def scenario(s, T, n, L, down=0):
    mid = [g for g in (T + max(1, T // 2), 2 * T + 1, 2 * T + 3) if g < L]            # the ticks before each are windows it ends at j = 1 .. n-1
    return {0: (0, [T - 1], False, None), 1: (0, [T], False, None), 2: (0, mid, False, None), 3: (0, [2 * T - 1], False, None),
            4: (0, [T // 2], True, None), 5: (0, [min(L - 1, T + 1)], False, (down, max(0, T - 2))), 6: (1, [T + 2] if T + 2 < L else [], False, None),
            7: (0, [], False, None)}[s]


def make_run(E, T, n, A, D, Ka=4, calls=3, shift=0, seed=0, down=0):
    """A run of L = calls * T ticks: obs [L + 1, E, A, D], act [L, E, A, Ka], rew [L, E, A] (never zero), done [L, E, A], env_done
    [L + 1, E] (the flag before each tick), game e following SCENARIOS[(e + shift) % 8].  Every agent's done is set on the tick its game
    ends (as the env does); agent `down` of scenario 5 goes down early, stays down until then, and rewards go on being recorded for it."""
    rng = np.random.default_rng([seed, E, T, n, A, D])
    L = calls * T
    obs, act = rng.standard_normal((L + 1, E, A, D)).astype(F32), rng.standard_normal((L, E, A, Ka)).astype(F32)
    rew = (rng.choice([-1.0, 1.0], (L, E, A)) * rng.uniform(0.25, 4.0, (L, E, A))).astype(F32)
    done, ed = np.zeros((L, E, A), np.uint8), np.zeros((L + 1, E), np.uint8)
    for e in range(E):
        before, ends, inert, early = scenario((e + shift) % len(SCENARIOS), T, n, L, down)
        over, dead = bool(before), np.zeros(A, bool)
        for g in range(L):
            ed[g, e] = over
            if over:                                       # the inert call, or the re-spawn: flags of a tick that is no transition
                over, dead[:] = inert, False
                done[g, e] = inert
            else:
                if early is not None and g >= early[1]:
                    dead[early[0]] = True
                if g in ends:
                    over, dead[:] = True, True
                done[g, e] = dead
        ed[L, e] = over
    return dict(obs=obs, act=act, rew=rew, done=done, env_done=ed)


def chunks(run, T):
    """The run as rollout-shaped records of T ticks: record c's obs and env_done carry one more row, the next record's first."""
    L = run["rew"].shape[0]
    return [dict(obs=run["obs"][t:t + T + 1], act=run["act"][t:t + T], rew=run["rew"][t:t + T], done=run["done"][t:t + T],
                 env_done=run["env_done"][t:t + T + 1]) for t in range(0, L, T)]


def team(rec, c0, nA, k):
    """The reference's view of a record: the team's columns, the first k action words."""
    return (rec["obs"][:, :, c0:c0 + nA], rec["act"][:, :, c0:c0 + nA, :k], rec["rew"][:, :, c0:c0 + nA], rec["done"][:, :, c0:c0 + nA], rec["env_done"])


def guard_appender(app, bufs):
    """Move an NStepAppender's staging buffer and carry into guard slabs (bufs: a guarded guard_util.Buffers); bufs.stray() names the ones
    whose surroundings a call wrote to."""
    import torch
    app._staging = bufs("staging", tuple(app._staging.shape), torch.int32)
    for name in ("_c_obs", "_c_act", "_c_rew", "_c_done", "_c_env_done", "carry_valid"):
        t = getattr(app, name)
        setattr(app, name, bufs(name, tuple(t.shape), t.dtype) if t.numel() else t)
    app._bind()
    return app
