"""The in-kernel draws the C oracle does not restate -- the actor's categorical uniforms and exploration normals, the continuous
scripted opponent's noise, the replay sampler's indices -- against the host restatement in tests/philox_util.py: bit for bit where
the arithmetic allows (words, float32 uniforms, the opponent's binary64 values, sampler indices), against float64 where it does not
(Gumbel, Box-Muller).  Statistics cannot see a keying mistake or an event of probability 2^-24; these comparisons do.  Rows at the
ends of the uniform code are reached by scanning the job-wide row space on the host (philox_util.edge_rows) and launching a small
call whose env_offset puts one of its games on the found row.  The measured errors are printed (run with -s to see them)."""
import numpy as np
import pytest
import torch

import philox_util as pu

pytestmark = pytest.mark.gpu

SEED = (1 << 32) + 0x2468ACE         # >= 2^32: the key's high word is in play
SEQ, SEQ_BASE = 5, (1 << 33) + 12345  # the call's seq and the device word added to it: the key's seq is their sum
SCAN = (1 << 20, 1 << 24)            # job-wide rows scanned for edge codes (first row, count)
GUMBEL_ATOL = 1e-4
NORMAL_TOL = 1e-5                    # |z - z64| <= NORMAL_TOL * (1 + |z64|)


def _env(**kw):
    import deep_rl_battlespace_amd as bsx
    return bsx.parallel_env(**kw)


def _actor(n, n_out=4, zero=False, seed=31):
    from deep_rl_battlespace_amd.rollout import StackedActor
    torch.manual_seed(seed)
    actor = StackedActor(2 * n, 3 * n + 2, n_out, device="cuda")
    with torch.no_grad():
        if zero:
            for p in (actor.w1, actor.b1, actor.w2, actor.b2, actor.w3, actor.b3):
                p.zero_()                                    # tanh(0) = 0: the score rows are the noise alone
        else:
            actor.w3.mul_(60.0)                              # spread the fresh heads so that rows differ
    return actor


def _grows(E, A, off):
    """Job-wide rows (env_offset + e) * A + a, [E, A] uint64."""
    return (np.arange(off, off + E, dtype=np.uint64)[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :])


def _seq_base():
    return torch.tensor([SEQ_BASE], dtype=torch.int64, device="cuda")


def _at(grow, A, k=5):
    """(env_offset, e, a) of a launch whose game e = k holds job-wide row `grow` in column a."""
    e0, a = divmod(int(grow), A)
    return e0 - k, k, a


# ---------------------------------------------------------------------------------------------------- categorical uniforms
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("off", [0, 100_003])
@pytest.mark.parametrize("noise_std", [0.0, 0.3])
def test_categorical_uniforms_are_the_restated_ones_bit_for_bit(n, off, noise_std):
    """The categorical head with its own Philox uniforms equals the same call fed the host-restated uniforms (u_inject): scores
    (the perturbed rows) and log-probabilities bit for bit.  Ragged E, a seed above 2^32, nonzero seq and seq_base, and a shard's
    env_offset: a wrong salt, key word or row would change every row."""
    from deep_rl_battlespace_amd.rollout import FusedActor
    E, A, D, tau = 1037, 2 * n, 3 * n + 2, 0.7
    actor = _actor(n)
    fa = FusedActor(actor, n, seed=SEED, env_offset=off)
    obs = (torch.rand((E, A, D), device="cuda") * 2 - 1).contiguous()
    sb = _seq_base()
    got, lp = torch.empty((E, A, 4), device="cuda"), torch.full((E, A), 7.0, device="cuda")
    fa.forward_into(obs, got, noise_std, seq=SEQ, seq_base=sb, sample=dict(temperature=tau, logp=lp))
    u = torch.from_numpy(pu.uniforms4(SEED, SEQ + SEQ_BASE, _grows(E, A, off))).cuda().contiguous()
    want, lp2 = torch.empty_like(got), torch.full_like(lp, 7.0)
    fa.forward_into(obs, want, noise_std, seq=SEQ, seq_base=sb, sample=dict(temperature=tau, logp=lp2, u=u))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(lp, lp2)
    assert bool(torch.isfinite(got).all()) and float(lp.max()) <= 0.0
    # the restatement is not trivially right: the neighbouring shard's uniforms give other rows
    u_wrong = torch.from_numpy(pu.uniforms4(SEED, SEQ + SEQ_BASE, _grows(E, A, off + E))).cuda().contiguous()
    fa.forward_into(obs, want, noise_std, seq=SEQ, seq_base=sb, sample=dict(temperature=tau, u=u_wrong))
    assert float((want != got).float().mean()) > 0.99


# ---------------------------------------------------------------------------------------------------- Gumbel against float64
def _gumbel_check(n, E, off, tau, obs, fa, what):
    """Run the head at (E, off); compare every perturbed score with float64 z / tau - log(-log u) (u restated, z the unperturbed
    forward's float32 scores); the drawn action with the float64 arg-max where the margin is clear; logp with float64 log-softmax.
    Returns the largest score error and how many rows had a clear margin, of how many."""
    A = 2 * n
    sb = _seq_base()
    z = torch.empty((E, A, 4), device="cuda")
    fa.forward_into(obs, z, 0.0, seq=SEQ, seq_base=sb)
    got, lp = torch.empty_like(z), torch.zeros((E, A), device="cuda")
    fa.forward_into(obs, got, 0.0, seq=SEQ, seq_base=sb, sample=dict(temperature=tau, logp=lp))
    torch.cuda.synchronize()
    u = pu.uniforms4(SEED, SEQ + SEQ_BASE, _grows(E, A, off)).astype(np.float64)
    z64 = z.double().cpu().numpy() / tau
    want = z64 - np.log(-np.log(u))
    g = got.double().cpu().numpy()
    assert np.isfinite(g).all(), (what, "non-finite perturbed score", np.argwhere(~np.isfinite(g))[:8].tolist())
    err = float(np.abs(g - want).max())
    assert err <= GUMBEL_ATOL, (what, err)
    top2 = np.sort(want, -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 10 * GUMBEL_ATOL
    drawn = g.argmax(-1)
    assert np.array_equal(drawn[clear], want.argmax(-1)[clear]), what
    m = z64.max(-1, keepdims=True)
    lsm = z64 - (m + np.log(np.exp(z64 - m).sum(-1, keepdims=True)))
    want_lp = np.take_along_axis(lsm, drawn[..., None], -1)[..., 0]
    lp_err = float(np.abs(lp.double().cpu().numpy() - want_lp).max())
    assert lp_err <= 2e-4, (what, lp_err)
    return err, int(clear.sum()), clear.size


@pytest.mark.parametrize("n", [1, 2])
def test_gumbel_scores_at_the_edge_codes_and_over_a_large_batch_against_float64(n):
    """Rows whose uniform word has the top code (r >> 8 == 0xFFFFFF: u was exactly 1.0 before uniforms4 kept 23 bits, and the
    perturbed score +inf) or the bottom code: every score finite and within GUMBEL_ATOL of float64; then the same over 65 536 games.
    Near u -> 1, -log u ~ 6e-8 and the Gumbel error IS __logf's relative error there: this bounds it."""
    from deep_rl_battlespace_amd.rollout import FusedActor
    A, D, tau = 2 * n, 3 * n + 2, 0.5
    actor = _actor(n)
    top, bottom = pu.edge_rows(SEED, SEQ + SEQ_BASE, pu.SALT_CATEGORICAL, *SCAN)
    assert top and bottom, "the fixed scan must reach both ends of the code"
    worst = 0.0
    for grow, comp in top + bottom:
        off, E = _at(grow, A)[0], 16
        fa = FusedActor(actor, n, seed=SEED, env_offset=off)
        obs = (torch.rand((E, A, D), device="cuda") * 2 - 1).contiguous()
        code = int(pu.actor_words(SEED, SEQ + SEQ_BASE, np.array([grow], np.uint64), pu.SALT_CATEGORICAL)[comp][0]) >> 8
        assert code in (0, 0xFFFFFF)
        err, _, _ = _gumbel_check(n, E, off, tau, obs, fa, f"edge row {grow} comp {comp} code {code:#x}")
        worst = max(worst, err)
    E, off = 65536, 100_003
    fa = FusedActor(actor, n, seed=SEED, env_offset=off)
    obs = (torch.rand((E, A, D), device="cuda") * 2 - 1).contiguous()
    err, n_clear, n_rows = _gumbel_check(n, E, off, tau, obs, fa, "large batch")
    assert n_clear > 0.99 * n_rows
    print(f"\n[gumbel n={n}] max |score - float64| at {len(top)} top / {len(bottom)} bottom edge rows: {worst:.3e}; "
          f"over {E * A * 4} components: {err:.3e} (tolerance {GUMBEL_ATOL:g})")


# ---------------------------------------------------------------------------------------------------- normals by key and salt
def _normals_from_kernel(mode, n, E, off):
    """z as the kernel drew it, read where no clamp interferes: an all-zero actor (scores are the noise alone), sigma = 1/8 (exact
    scaling).  Returns {salt: z [E, A, 4] float64}."""
    from deep_rl_battlespace_amd.rollout import FusedActor
    A, D = 2 * n, 3 * n + 2
    fa = FusedActor(_actor(n, zero=True), n, seed=SEED, env_offset=off)
    obs = torch.rand((E, A, D), device="cuda").contiguous()
    out = torch.empty((E, A, 4), device="cuda")
    st = torch.zeros((E, A, 4), device="cuda")
    sb, s = _seq_base(), 0.125
    if mode == "gauss":                                  # scores = fmaf(1/8, z, 0) = z / 8 exactly, |z| < 6: never clamped
        fa.forward_into(obs, out, s, seq=SEQ, seq_base=sb)
        torch.cuda.synchronize()
        assert float(out.abs().max()) < 1.0
        return {pu.SALT_OU: out.double().cpu().numpy() / s}
    scale = 2.0 ** -10
    # OU from x = 0, mu = 0: x = 0 + fmaf(theta, 0, sigma * z) = z / 8 exactly, stored
    fa.forward_into(obs, out, s if mode == "ou+gauss" else 0.0, seq=SEQ, seq_base=sb, ou=dict(scale=scale, state=st, sigma=s, mu=0.0))
    torch.cuda.synchronize()
    x = st.double().cpu().numpy()
    res = {pu.SALT_OU: x / s}
    if mode == "ou+gauss":                               # scores = fmaf(1/8, zg, scale * x): zg to within half an ulp of the score, times 8
        o = out.double().cpu().numpy()
        assert np.abs(o).max() < 1.0
        res[pu.SALT_GAUSS_WITH_OU] = (o - scale * x) / s
    return res


@pytest.mark.parametrize("mode", ["gauss", "ou", "ou+gauss"])
@pytest.mark.parametrize("n", [1, 3])
def test_exploration_normals_are_the_restated_box_muller_at_the_expected_salt(mode, n):
    """Gaussian noise alone and the OU increment draw normals4 at salt 0; with both on, the Gaussian term draws at salt 0x80000000.
    Each against the host Box-Muller (float32 uniforms as the kernel forms them, float64 log / sin / cos) at a shard's env_offset,
    and at found rows where the radius word u0 / u2 takes its top code (u = 1.0, radius 0) or its bottom code (radius 5.9).
    A wrong salt, key or row gives O(1) differences."""
    A = 2 * n
    worst, rows = {}, []
    E, off = 4133, 100_003
    rows.append((E, off))
    edge = {}
    for salt in ((pu.SALT_OU,) if mode != "ou+gauss" else (pu.SALT_OU, pu.SALT_GAUSS_WITH_OU)):
        top, bottom = pu.edge_rows(SEED, SEQ + SEQ_BASE, salt, *SCAN)
        edge[salt] = [(g, c) for g, c in top + bottom if c in (0, 2)]       # the radius words
        rows += [(16, _at(g, A)[0]) for g, _ in edge[salt]]
    assert sum(len(v) for v in edge.values()) > 0, "the fixed scan must reach an edge code of a radius word"
    for E, off in rows:
        got = _normals_from_kernel(mode, n, E, off)
        for salt, z in got.items():
            want = pu.normals4(SEED, SEQ + SEQ_BASE, _grows(E, A, off), salt)
            err = float((np.abs(z - want) / (1.0 + np.abs(want))).max())
            assert err <= NORMAL_TOL, (mode, salt, E, off, err)
            worst[salt] = max(worst.get(salt, 0.0), err)
            other = pu.SALT_GAUSS_WITH_OU if salt == pu.SALT_OU else pu.SALT_OU
            if E > 16:                                   # the other salt's normals are other numbers
                assert np.abs(z - pu.normals4(SEED, SEQ + SEQ_BASE, _grows(E, A, off), other)).mean() > 0.5
    for salt, hits in edge.items():                      # the edge rows themselves: radius 0 at the top code
        for g, c in hits:
            w = pu.normals4(SEED, SEQ + SEQ_BASE, np.array([g], np.uint64), salt)[0]
            top = (int(pu.actor_words(SEED, SEQ + SEQ_BASE, np.array([g], np.uint64), salt)[c][0]) >> 8) == 0xFFFFFF
            assert (abs(w[c]) + abs(w[c + 1]) == 0.0) if top else (abs(w[c]) + abs(w[c + 1]) > 4.0)
    print(f"\n[normals {mode} n={n}] max |z - z64| / (1 + |z64|) by salt: " + ", ".join(f"{s:#x}: {v:.3e}" for s, v in worst.items())
          + f"; edge rows {dict((hex(s), len(v)) for s, v in edge.items())} (tolerance {NORMAL_TOL:g})")


# ---------------------------------------------------------------------------------------------------- scripted opponent
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("off", [0, 5000])
@pytest.mark.parametrize("with_base", [False, True])
def test_continuous_opponent_draws_are_keyed_by_the_job_wide_row(n, off, with_base):
    """instinct.Team.write_actions in production mode (in-kernel Philox) equals the same call fed the host draws of the job-wide row
    (env_offset + e) * A + a (rnd), float64 actions bit for bit; the draws of the launch's own row e * A + a are other actions."""
    from deep_rl_battlespace_amd import instinct
    E, A = 1037, 2 * n
    env = _env(n_agents=n, n_envs=E, seed=23, continuous_actions=True, env_offset=off, device="cuda")
    env.reset()
    for team in (instinct.Team(env.possible_blue, env.possible_red, env, seed=SEED),
                 instinct.Team(env.possible_red, env.possible_blue, env, seed=SEED + 1)):
        sb = _seq_base() if with_base else None
        key_seq = SEQ + (SEQ_BASE if with_base else 0)
        got = torch.zeros((E, A, 3), dtype=torch.float64, device="cuda")
        team.write_actions(out=got, seq=SEQ, seq_base=sb)
        want = torch.zeros_like(got)
        team.write_actions(out=want, seq=SEQ, seq_base=sb, rnd=pu.opponent_draws(team.seed, key_seq, _grows(E, A, off)))
        torch.cuda.synchronize()
        assert torch.equal(got, want), (n, off, team.team)
        cols = team._cols
        assert float(got[:, cols].abs().sum()) > 0 and float(got[:, [c for c in range(A) if c not in cols]].abs().sum()) == 0.0
        if off:
            launch_rows = team.write_actions(out=torch.zeros_like(got), seq=SEQ, seq_base=sb,
                                             rnd=pu.opponent_draws(team.seed, key_seq, _grows(E, A, 0)))
            assert float((launch_rows[:, cols] != got[:, cols]).float().mean()) > 0.5


@pytest.mark.parametrize("one_launch", [False, True])
def test_scripted_opponent_noise_does_not_depend_on_the_sharding(one_launch):
    """A job with a continuous scripted opponent split over ranks (env_offset) plays exactly the unsplit job: the opponent's draws
    are keyed by the global row, like the actor's and the env's own.  The whole job and 4 pieces: equal observations, scores,
    rewards and flags, in the per-tick graph and the one-launch rollout."""
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout
    E, n, T, parts = 2048, 2, 24, 4
    actor = _actor(n, n_out=3, seed=2)

    def play(E_, off):
        env = _env(n_agents=n, n_envs=E_, seed=11, auto_reset=True, env_offset=off, continuous_actions=True); env.reset()
        opp = instinct.Team(env.possible_blue, env.possible_red, env, seed=91)
        ro = PolicyRollout(env, actor, T, noise_std=0.2, seed=9, one_launch=one_launch, opponent=opp); ro.start()
        for _ in range(6):
            ro.run()
        torch.cuda.synchronize()
        return ro
    whole = play(E, 0)
    q = E // parts
    pieces = [play(q, i * q) for i in range(parts)]
    for name in ("obs", "scores", "rew", "done", "env_done"):
        assert torch.equal(getattr(whole, name), torch.cat([getattr(p, name) for p in pieces], dim=1)), name
    assert int(whole.env.counters()[:, 0].sum()) > 0
    cols = whole.opponent._cols
    assert 0.02 < float((whole.scores[..., cols, 2] > 0).float().mean()) < 0.9     # the script fires sometimes: its draws are in play


# ---------------------------------------------------------------------------------------------------- replay sampler
@pytest.mark.parametrize("M", [1, 777, 999_983])
def test_replay_sampler_indices_are_the_restated_ones(M):
    """DeviceReplayBuffer.sample(): last_idx equals the host indices (w.x * clamp(counter, 0, M)) >> 32 for the draw word's value
    before the call -- counters 0, 1, M - 1, M, M + 1, 5M + 17 and a negative one written into the device word (all zeros), batch
    sizes across the 32-draw workgroup boundary, a seed above 2^32, and three replays of a captured sample()."""
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    seed = (1 << 32) + 77
    for B in (1, 31, 33, 4097):
        buf = DeviceReplayBuffer(M, B, ["plane0"], 2, 2, 4, device="cuda", seed=seed)
        for cnt in (0, 1, M - 1, M, M + 1, 5 * M + 17, -3):
            if cnt < 0:
                buf._counter.fill_(cnt)                  # only a raw write can make it negative (mem_cntr refuses)
            else:
                buf.mem_cntr = cnt
            draw = int(buf._draws.item())
            buf.sample()
            torch.cuda.synchronize()
            want = pu.sampler_indices(seed, draw, B, M, cnt)
            assert np.array_equal(buf.last_idx.cpu().numpy(), want), (M, B, cnt)
            assert int(buf._draws.item()) == draw + 1
    # a captured sample(): each replay draws with the word's value at that replay
    buf = DeviceReplayBuffer(M, 4097, ["plane0"], 2, 2, 4, device="cuda", seed=seed)
    buf.mem_cntr = 5 * M + 17
    buf._draws.fill_(1 << 33)                            # the sequence number's high word is in play too
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.sample()
    for _ in range(3):
        draw = int(buf._draws.item())
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(buf.last_idx.cpu().numpy(), pu.sampler_indices(seed, draw, 4097, M, 5 * M + 17)), draw
        assert int(buf._draws.item()) == draw + 1
