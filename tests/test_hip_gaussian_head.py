"""The Gaussian policy head on the MI355X (bsx_actor_forward_gaussian, bsx_rollout_continuous_gaussian, PolicyRollout(sample="gaussian")):
the head against torch with injected normals; the kernel's own normals against the host Philox restatement at their salt; the one-launch
rollout against the graph of (actor -> step) pairs bit for bit; a closed loop against the C oracle on the recorded, unclipped rows; GAE on
the head's records; an in-place update of log_std seen by a captured graph."""
import math

import numpy as np
import pytest
import torch

import philox_util as pu
from gae_util import gae_ref
from guard_util import SENTINEL

pytestmark = pytest.mark.gpu

SALT = 0xC0000000                 # normals4 under the Gaussian policy head (bsx_actor_core.h: GAUSS_SALT)
SEED, SEQ, SEQ_BASE = 0x1234ABCD5678, 7, 1000
NORMAL_TOL = 1e-5                 # |z - z64| <= NORMAL_TOL * (1 + |z64|), as tests/test_hip_rng_restated.py


def _actor(n, scale=1.0, seed=5, outputs=3):
    from deep_rl_battlespace_amd.rollout import StackedActor
    torch.manual_seed(seed)
    a = StackedActor(2 * n, 3 * n + 2, outputs, device="cuda")
    with torch.no_grad():
        a.w3.mul_(scale)
    return a


def _obs(E, n, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((E, 2 * n, 3 * n + 2), device="cuda", generator=g) * 2 - 1


# ---------------------------------------------------------------------------------------------------- 1. exact, against torch
@pytest.mark.parametrize("precision", ["f32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_head_with_injected_normals_equals_torch(n, precision):
    from deep_rl_battlespace_amd.rollout import FusedActor, gaussian_log_prob
    E, A = 300, 2 * n
    actor = _actor(n, scale=10.0)
    obs = _obs(E, n)
    z = torch.randn((E, A, 4), device="cuda")
    ls = (0.4 * torch.randn((A, 3), device="cuda")).contiguous()
    fa = FusedActor(actor, n, precision=precision)
    scores = torch.full((E, A, 4), 7.0, device="cuda")
    logp = torch.full((E, A), 7.0, device="cuda")
    fa.forward_into(obs, scores, seq=3, z=z, gaussian=dict(log_std=ls, logp=logp))
    torch.cuda.synchronize()
    with torch.no_grad():
        mu = actor(obs)
        want = mu + torch.exp(ls) * z[..., :3]
        want_lp, _ = gaussian_log_prob(actor, ls, obs, scores)
        dist_lp = torch.distributions.Normal(mu, torch.exp(ls)).log_prob(scores[..., :3]).sum(-1)
    # bf16x3: ~1e-5 on a tanh score AT THIS (fresh) WEIGHT SCALE (test_hip_rollout_oracle.py scales the same way); the budgets that follow
    # from a float64 reference, at trained-weight scale too, are in tests/test_hip_actor_float64.py
    tol = 1.0 if precision != "bf16x3" else 40.0
    torch.testing.assert_close(scores[..., :3], want, rtol=0, atol=2e-5 * tol)
    assert bool((scores[..., 3] == 0).all())
    assert float(scores[..., :3].abs().max()) > 1.0                                # unclipped
    torch.testing.assert_close(logp, want_lp, rtol=0, atol=1e-4 * tol)
    torch.testing.assert_close(logp, dist_lp, rtol=0, atol=1e-4 * tol)
    # logp is a function of z and log_std alone: the kernel's value against the normals it was given
    want_z = (-0.5 * z[..., :3] ** 2 - ls).sum(-1) - 1.5 * math.log(2 * math.pi)
    torch.testing.assert_close(logp, want_z, rtol=0, atol=2e-5)
    # without a logp tensor the head still draws the same rows
    s2 = torch.zeros_like(scores)
    fa.forward_into(obs, s2, seq=3, z=z, gaussian=dict(log_std=ls))
    assert torch.equal(s2, scores)


# ---------------------------------------------------------------------------------------------------- 2. the kernel's own draws
def _draw(n, E, off, ls, seq=SEQ, games=None, logp=None):
    from deep_rl_battlespace_amd.rollout import FusedActor
    actor = _actor(n, scale=30.0)
    fa = FusedActor(actor, n, seed=SEED, env_offset=off)
    obs = _obs(E, n, seed=2)
    sb = torch.tensor([SEQ_BASE], dtype=torch.int64, device="cuda")
    mu, a = torch.empty((E, 2 * n, 4), device="cuda"), torch.empty((E, 2 * n, 4), device="cuda")
    fa.forward_into(obs, mu, 0.0, seq=seq, seq_base=sb)                              # the plain kernel: the tanh row = mu, same bits
    if games is None:
        fa.forward_into(obs, a, seq=seq, seq_base=sb, gaussian=dict(log_std=ls, logp=logp))
    else:
        for g in games:
            fa.forward_into(obs, a, seq=seq, seq_base=sb, gaussian=dict(log_std=ls, logp=logp), games=g)
    torch.cuda.synchronize()
    return mu, a


@pytest.mark.parametrize("n", [1, 3])
def test_head_normals_are_the_restated_box_muller_at_their_salt(n):
    A, E, off = 2 * n, 4133, 100_003
    ls = torch.zeros((A, 3), device="cuda")
    mu, a = _draw(n, E, off, ls)
    z = (a[..., :3] - mu[..., :3]).double().cpu().numpy()                           # sigma = 1: a - mu = z to a rounding of a
    grows = np.uint64(off) * np.uint64(A) + np.arange(E * A, dtype=np.uint64)
    want = pu.normals4(SEED, SEQ + SEQ_BASE, grows, SALT).reshape(E, A, 4)[..., :3]
    err = np.abs(z - want) / (1.0 + np.abs(want))
    assert float(err.max()) <= NORMAL_TOL + 2.0 ** -22, float(err.max())
    for other in (pu.SALT_OU, pu.SALT_GAUSS_WITH_OU):                               # the other salts' normals are other numbers
        assert np.abs(z - pu.normals4(SEED, SEQ + SEQ_BASE, grows, other).reshape(E, A, 4)[..., :3]).mean() > 0.5
    # a different sigma per plane and column scales the same normals
    ls2 = torch.linspace(-1.0, 0.7, A * 3, device="cuda").reshape(A, 3).contiguous()
    mu2, a2 = _draw(n, E, off, ls2)
    assert torch.equal(mu2, mu)
    z2 = ((a2[..., :3] - mu2[..., :3]) / torch.exp(ls2)).double().cpu().numpy()
    assert float((np.abs(z2 - want) / (1.0 + np.abs(want))).max()) <= 1e-4


def test_head_normals_are_standard_keyed_by_seq_and_by_the_job_wide_row():
    n, E, off = 1, 65536, 12_288
    A = 2 * n
    ls = torch.zeros((A, 3), device="cuda")
    lp = torch.zeros((E, A), device="cuda")
    mu, a = _draw(n, E, off, ls, logp=lp)
    z = (a[..., :3] - mu[..., :3]).double().reshape(-1, 3)
    N = z.shape[0]
    m, v = z.mean(0), z.var(0)
    assert bool((m.abs() < 5.0 / math.sqrt(N)).all()), m
    assert bool(((v - 1.0).abs() < 5.0 * math.sqrt(2.0 / N)).all()), v
    # another sequence number draws other normals
    mu_s, a_s = _draw(n, E, off, ls, seq=SEQ + 1)
    assert torch.equal(mu_s, mu)
    assert float((a_s - a)[..., :3].abs().mean()) > 0.5
    # the job split in two ranks (env_offset) draws what the unsplit job draws (the shards' own observations differ: compare a - mu = z);
    # so do the games= ranges of one call, bit for bit
    k = 25_600
    mu_lo, lo = _draw(n, k, off, ls)
    mu_hi, hi = _draw(n, E - k, off + k, ls)
    z_split = torch.cat([lo - mu_lo, hi - mu_hi])[..., :3].double().reshape(-1, 3)
    torch.testing.assert_close(z_split, z, rtol=0, atol=2e-6)
    lp_r = torch.zeros((E, A), device="cuda")
    _, a_r = _draw(n, E, off, ls, games=[(0, k), (k, E - k)], logp=lp_r)
    assert torch.equal(a_r, a) and torch.equal(lp_r, lp)


# ---------------------------------------------------------------------------------------------------- 3. one launch == the graph
def _play(n, E, T, one_launch, log_std, value=False, opponent=None, chains=1, gae=None, guard=False, seed=41):
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, continuous_actions=True, device="cuda")
    env.reset()
    actor = _actor(n, scale=60.0)                                                   # decisive policies: planes die, games end
    critic = _actor(n, scale=100.0, seed=9, outputs=1) if value else None
    opp = None
    if opponent is not None:
        mine, theirs = (env.possible_red, env.possible_blue) if opponent == "red" else (env.possible_blue, env.possible_red)
        opp = instinct.Team(mine, theirs, env)
    ro = PolicyRollout(env, actor, T, seed=3, one_launch=one_launch, sample="gaussian", log_std=log_std, value_actor=critic, opponent=opp,
                       chains=chains, gae=gae)
    slabs = None
    if guard:                                                                        # the head's record with sentinel bytes behind it
        nb = ro.logp.numel() * 4
        s = torch.full((nb + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
        ro.logp = s[:nb].view(torch.float32).view(ro.logp.shape)
        ro.logp.zero_()
        slabs = (s, nb)
    ro.start(); ro.capture()
    return env, ro, slabs


FIELDS = ("obs", "scores", "logp", "rew", "_done", "env_done")


@pytest.mark.parametrize("n,E,value,opponent", [(1, 300, True, None), (2, 256, False, None), (3, 96, False, None), (4, 64, False, None),
                                                (1, 1, True, None), (4, 5, False, None), (3, 7, False, None), (3, 33, False, None),
                                                (1, 160, True, "red"), (2, 96, False, "blue")])
def test_one_launch_equals_the_graph_bit_for_bit(n, E, value, opponent):
    T = 64                                                                           # 3 runs = 192 ticks: past every time-limit tie up to 4v4
    A = 2 * n
    ls = (0.3 * torch.randn((A, 3), generator=torch.Generator().manual_seed(n))).to("cuda").contiguous()
    env_g, g, _ = _play(n, E, T, False, ls, value, opponent)
    env_o, o, slabs = _play(n, E, T, True, ls, value, opponent, guard=True)
    ended = 0
    for k in range(3):
        g.run(); o.run()
        torch.cuda.synchronize()
        for f in FIELDS + (("value",) if value else ()):
            assert torch.equal(getattr(g, f), getattr(o, f)), (k, f)
        ended += int((o.env_done[1:] != 0).sum())
        assert float(o.scores[..., :3].abs().max()) > 1.0 and bool((o.scores[..., 3] == 0).all())
        if opponent is not None:
            cols = slice(0, n) if opponent == "red" else slice(n, A)
            assert bool((o.logp[:, :, cols] == 0).all()) and bool((g.logp[:, :, cols] == 0).all())
            learned = slice(n, A) if opponent == "red" else slice(0, n)
            assert bool((o.logp[:, :, learned] != 0).all())
        else:
            assert bool((o.logp != 0).all())
    sg, so = env_g.export_state(), env_o.export_state()
    for f in sg:
        assert torch.equal(sg[f], so[f]), f
    s, nb = slabs
    assert bool((s[nb:] == SENTINEL).all()), "the one-launch form wrote past logp"
    if E >= 64:
        assert ended > 0


# ---------------------------------------------------------------------------------------------------- 4. against the C oracle
@pytest.mark.parametrize("n", [1, 2])
def test_recorded_unclipped_rows_replay_on_the_c_oracle(n):
    from oracle import cref
    E, T, runs, seed = 64, 40, 2, 77
    kw = dict(n_agents=n, seed=seed, auto_reset=True, continuous_actions=True)
    c = cref.CRefBatch(E, **kw)
    o_c = c.reset().copy()
    env, ro, _ = _play(n, E, T, n == 1, torch.zeros((2 * n, 3), device="cuda"), seed=seed)
    outside = 0
    for run in range(runs):
        ro.run()
        torch.cuda.synchronize()
        obs, sc, rew, done, edone = (x.cpu().numpy() for x in (ro.obs, ro.scores, ro.rew, ro._done, ro.env_done))
        if run == 0:
            np.testing.assert_allclose(obs[0], o_c, rtol=1e-5, atol=1e-7)
        outside += int((np.abs(sc[..., :3]) > 1.0).sum())
        for t in range(T):
            assert np.array_equal(edone[t], c.env_done), (run, t)
            co, cr, cd = c.step(np.ascontiguousarray(sc[t][..., :3]))
            assert np.array_equal(done[t].astype(bool), cd), (run, t)
            assert np.array_equal(rew[t].astype(np.float64), cr), (run, t)
            diff = np.abs(obs[t + 1].astype(np.float64) - co)
            assert not ((diff > 1e-7) & (diff / np.maximum(np.abs(co), 1e-30) > 1e-5)).any(), (run, t)
    assert outside > 0, "no recorded row left [-1, 1]: the clip was not exercised"


# ---------------------------------------------------------------------------------------------------- 5. GAE
@pytest.mark.parametrize("n,E,one_launch,chains", [(1, 301, True, 1), (2, 512, False, 2)])
def test_gae_on_the_gaussian_rollout_equals_the_restatement_of_its_records(n, E, one_launch, chains):
    T, runs, gamma, lam = 32, 5, 0.99, 0.95
    ls = torch.full((2 * n, 3), -0.5, device="cuda")
    _, ro, _ = _play(n, E, T, one_launch, ls, value=True, chains=chains, gae=dict(gamma=gamma, lam=lam))
    assert ro.chains == chains
    prev = ro._done_prev.clone()
    ends = 0
    for k in range(runs):
        ro.run()
        torch.cuda.synchronize()
        rec = [x.cpu().numpy() for x in (ro.rew, ro.value, ro.last_value, ro._done, ro.env_done, prev)]
        wa, wr, wm, wc = gae_ref(*rec, gamma, lam)[:4]
        a, r, m, c = (x.cpu().numpy() for x in (ro.adv, ro.ret, ro.mask, ro._done_prev))
        assert np.array_equal(m, wm), k
        assert np.array_equal(a.view(np.int32), wa.view(np.int32)), k
        assert np.array_equal(r.view(np.int32), wr.view(np.int32)), k
        assert np.array_equal(c, wc), k
        ends += int((ro.env_done[1:] != 0).sum())
        prev = ro._done_prev.clone()
    assert ends > 0


# ---------------------------------------------------------------------------------------------------- 6. in-place updates
@pytest.mark.parametrize("one_launch", [False, True])
def test_a_captured_graph_sees_an_in_place_log_std_update(one_launch):
    from deep_rl_battlespace_amd.rollout import FusedActor
    n, E, T = 1, 512, 8
    ls = torch.zeros((2, 3), device="cuda")
    env, ro, _ = _play(n, E, T, one_launch, ls)
    ro.run(); torch.cuda.synchronize()                                              # leave the start: tick 0 of the next run reads obs[T]
    keep = (ro.obs[T].clone(), ro.env_done[T].clone(), ro._seq_base.clone())
    ro.run(); torch.cuda.synchronize()
    a1, lp1, obs0 = ro.scores[0].clone(), ro.logp[0].clone(), ro.obs[0].clone()
    ro.obs[T].copy_(keep[0]); ro.env_done[T].copy_(keep[1]); ro._seq_base.copy_(keep[2])
    ls.add_(0.5)                                                                     # the learner's in-place update; no re-capture
    ro.run(); torch.cuda.synchronize()
    assert torch.equal(ro.obs[0], obs0)
    mu = torch.empty_like(a1)
    FusedActor(ro.actor, n).forward_into(obs0, mu, 0.0, seq=0)
    d1, d2 = (a1 - mu)[..., :3], (ro.scores[0] - mu)[..., :3]
    torch.testing.assert_close(d2, d1 * math.exp(0.5), rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(ro.logp[0], lp1 - 1.5, rtol=0, atol=2e-5)             # log N: -sum(log_std) moves by 3 * 0.5, z unchanged
