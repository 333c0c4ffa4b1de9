"""The n-step fold in front of the device ring (csrc/bsx_replay_nstep.hip, replay.NStepAppender) on the MI355X, held bit for bit to its
numpy restatement (tests/nstep_util.py) on hand-made records that place every boundary case, at the smallest shapes that can go wrong: a
lone game, a ragged wave, a ragged 256-row tile; T = n, n + 1 and 7; team columns at an offset inside wider records; rings smaller than
one call's rows and rings that wrap; both rings; and one real rollout, eager and captured with a learner behind it."""
import types

import numpy as np
import pytest
import torch

import ddpg_util as D
import nstep_util as U
from guard_util import Buffers
from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, NStepAppender, PrioritizedReplayBuffer

pytestmark = pytest.mark.gpu

GAMMA = 0.95
#         E    T  n  nA  D  k  c0  A    M   shift      (c0: the team's first column of the A recorded ones; shift: nstep_util.make_run's)
CASES = [(257, 7, 3, 2,  8, 4, 1,  4, 4000, 0),
         (257, 5, 5, 3, 11, 3, 2,  6, 1000, 0),      # T = n; the ring is smaller than one call's rows
         (257, 6, 5, 1,  5, 4, 0,  2, 3000, 0),      # T = n + 1; wraps on the third call
         (257, 2, 1, 1,  5, 3, 1,  2,  300, 0),      # n = 1, T = n + 1, M < rows
         (5,   7, 5, 2,  8, 3, 1,  4,   64, 0),      # wraps
         (5,   2, 2, 3, 11, 4, 0,  3,    7, 3),      # T = n, M < rows
         (5,   3, 2, 1,  5, 3, 1,  2,  100, 5),      # T = n + 1
         (5,   3, 3, 2,  8, 4, 2,  4,   23, 0),      # T = n, wraps
         (5,   4, 3, 3, 11, 3, 3,  6,  100, 4),      # T = n + 1
         (5,   1, 1, 2,  8, 4, 0,  4,  100, 0),      # n = 1 = T
         (5,   7, 1, 3, 11, 4, 0,  6,  100, 0),
         (5,   7, 2, 2,  8, 4, 2,  4,  100, 0),
         (1,   5, 5, 1,  5, 3, 0,  2,    5, 2),      # a lone game, T = n
         (1,   6, 5, 3, 11, 4, 1,  6,   50, 5),
         (1,   1, 1, 1,  5, 3, 0,  1,    2, 1),
         (1,   3, 2, 2,  8, 4, 0,  2,    4, 4)]
CASES += [(1, 7, 3, 2, 8, 4, 1, 4, 16, s) for s in range(len(U.SCENARIOS))]         # a lone game through every scenario


def _ring(M, nA, D, k, cls=DeviceReplayBuffer, B=4):
    return cls(M, B, [f"plane{i}" for i in range(nA)], D, D * nA, k, device="cuda", seed=1)


def _upload(rec):
    return {key: torch.from_numpy(np.ascontiguousarray(v)).cuda() for key, v in rec.items()}


def _append(app, rec, cols):
    d = _upload(rec)
    return app.append(d["obs"], d["act"], d["rew"], d["done"], d["env_done"], cols), d


@pytest.mark.parametrize("E,T,n,nA,D,k,c0,A,M,shift", CASES)
def test_three_calls_match_the_reference_bit_for_bit_inside_guards(E, T, n, nA, D, k, c0, A, M, shift):
    run = U.make_run(E, T, n, A, D, shift=shift, down=c0)
    buf, bufs = _ring(M, nA, D, k), Buffers(True)
    app = U.guard_appender(NStepAppender(buf, n, GAMMA, T, E), bufs)
    ref, ring = U.NStepRef(n, GAMMA, E, nA, D, k), U.RingRef(M, nA, D, k)
    assert not app.carry_valid.any()
    kept = []
    for c, rec in enumerate(U.chunks(run, T)):
        stored, held = _append(app, rec, range(c0, c0 + nA))
        out = ref.fold(*U.team(rec, c0, nA, k))
        kept.append(ring.append(out, out["skip"]))
        assert int(stored) == kept[-1] and stored is buf._stored, (c, int(stored), kept[-1])
        U.assert_ring_equal(buf, ring, c)
        assert np.array_equal(app.carry_valid.cpu().numpy(), ref.valid) and app.carry_valid.all(), c
        for mine, want in ((app._c_obs, ref.c_obs), (app._c_act, ref.c_act), (app._c_rew, ref.c_rew), (app._c_done, ref.c_done),
                           (app._c_env_done, ref.c_ed)):
            assert np.array_equal(U.bits(mine.cpu().numpy()), U.bits(want)), c
        del held
    assert bufs.stray() == []
    # carry_valid starts at 0: the first call stores the T - n + 1 complete windows of its record, those that start on a running game
    assert kept[0] == int((run["env_done"][:T - n + 1] == 0).sum()) and sum(kept) > 0


@pytest.mark.parametrize("E,T,nA,D,k,c0,A,M", [(257, 7, 2, 8, 4, 1, 4, 2500), (5, 3, 3, 11, 3, 0, 3, 12), (1, 1, 1, 5, 3, 1, 2, 1)])
def test_one_step_stores_what_append_rollout_stores(E, T, nA, D, k, c0, A, M):
    run = U.make_run(E, T, 1, A, D, down=c0)
    buf, plain = _ring(M, nA, D, k), _ring(M, nA, D, k)
    app = NStepAppender(buf, 1, GAMMA, T, E)
    for c, rec in enumerate(U.chunks(run, T)):
        stored, d = _append(app, rec, range(c0, c0 + nA))
        ro = types.SimpleNamespace(T=T, obs=d["obs"], scores=d["act"], rew=d["rew"], _done=d["done"], env_done=d["env_done"])
        want = plain.append_rollout(ro, range(c0, c0 + nA))
        assert int(stored) == int(want), c
        for f in ("actor_states", "actor_new_states", "action_mem", "rew_mem"):
            assert torch.equal(getattr(buf, f).view(torch.int32), getattr(plain, f).view(torch.int32)), (c, f)
        assert torch.equal(buf.done_mem, plain.done_mem) and buf.mem_cntr == plain.mem_cntr, c
    assert buf.mem_cntr > M                                    # the rings wrapped


@pytest.mark.parametrize("E,T,n,nA,D,k", [(257, 5, 5, 2, 8, 4), (5, 3, 2, 3, 11, 3), (5, 7, 3, 1, 5, 4)])
def test_one_rollout_of_2T_ticks_equals_two_of_T_ticks(E, T, n, nA, D, k):
    run = U.make_run(E, T, n, nA + 1, D, calls=2, down=1)
    M = 2 * T * E + 3
    whole, halves = _ring(M, nA, D, k), _ring(M, nA, D, k)
    one, two = NStepAppender(whole, n, GAMMA, 2 * T, E), NStepAppender(halves, n, GAMMA, T, E)
    _append(one, U.chunks(run, 2 * T)[0], range(1, 1 + nA))
    for rec in U.chunks(run, T):
        _append(two, rec, range(1, 1 + nA))
    for f in ("actor_states", "actor_new_states", "action_mem", "rew_mem"):
        assert torch.equal(getattr(whole, f).view(torch.int32), getattr(halves, f).view(torch.int32)), f
    assert torch.equal(whole.done_mem, halves.done_mem) and 0 < whole.mem_cntr == halves.mem_cntr < M
    for f in ("_c_obs", "_c_act", "_c_rew"):
        assert torch.equal(getattr(one, f).view(torch.int32), getattr(two, f).view(torch.int32)), f
    assert torch.equal(one._c_done, two._c_done) and torch.equal(one._c_env_done, two._c_env_done) and torch.equal(one.carry_valid, two.carry_valid)


@pytest.mark.parametrize("E,T,n", [(257, 4, 3), (5, 7, 5), (1, 2, 2)])
def test_reset_carry_drops_the_masked_games_carried_ticks_on_the_device(E, T, n):
    """The host re-spawns some games between two calls: their carried ticks are not stored, every other row is."""
    nA, D, k, M = 2, 5, 3, 3 * 7 * 257
    run = U.make_run(E, T, n, nA, D, shift=7)
    buf = _ring(M, nA, D, k)
    app = NStepAppender(buf, n, GAMMA, T, E)
    ref, plain, ring = U.NStepRef(n, GAMMA, E, nA, D, k), U.NStepRef(n, GAMMA, E, nA, D, k), U.RingRef(M, nA, D, k)
    mask = np.arange(E) % 3 == 0
    dropped = 0
    for c, rec in enumerate(U.chunks(run, T)):
        if c == 1:
            app.reset_carry(torch.from_numpy(mask).cuda())
            ref.reset_carry(mask)
            assert np.array_equal(app.carry_valid.cpu().numpy(), ref.valid) and ref.valid.sum() == E - mask.sum()
        if c == 2:
            app.reset_carry()
            ref.reset_carry()
            assert not app.carry_valid.any()
        stored, _ = _append(app, rec, range(nA))
        out = ref.fold(*U.team(rec, 0, nA, k))
        assert int(stored) == ring.append(out, out["skip"]), c
        U.assert_ring_equal(buf, ring, c)
        assert app.carry_valid.all()
        # against a reference nobody reset: exactly the carried ticks of the games named, where they were transitions, are missing
        kept = plain.fold(*U.team(rec, 0, nA, k))["skip"].reshape(T, E) == 0
        named = mask if c == 1 else np.ones(E, bool)
        lost = int(kept[:n - 1][:, named].sum()) if c else 0
        assert int(stored) == int(kept.sum()) - lost, c
        dropped += lost
    assert dropped > 0


@pytest.mark.parametrize("E,T,n,M", [(257, 4, 3, 700), (5, 7, 5, 60)])
def test_a_prioritised_ring_gives_the_new_rows_max_priority_and_keeps_its_tree(E, T, n, M):
    nA, D, k = 2, 8, 4
    run = U.make_run(E, T, n, nA, D)
    buf = _ring(M, nA, D, k, cls=PrioritizedReplayBuffer)
    app = NStepAppender(buf, n, GAMMA, T, E)
    ref, ring = U.NStepRef(n, GAMMA, E, nA, D, k), U.RingRef(M, nA, D, k)
    leaves = np.zeros(M, np.int64)
    for c, rec in enumerate(U.chunks(run, T)):
        prio = 65536 * (c + 1) + c
        buf.max_priority.fill_(prio)
        stored, _ = _append(app, rec, range(nA))
        out = ref.fold(*U.team(rec, 0, nA, k))
        before = ring.counter
        R = ring.append(out, out["skip"])
        leaves[[(before + j) % M for j in range(max(0, R - M), R)]] = prio
        assert int(stored) == R
        U.assert_ring_equal(buf, ring, c)
        assert np.array_equal(buf.priorities.cpu().numpy().astype(np.int64), leaves), c
        tree = buf.tree.clone()
        buf.rebuild_tree()
        assert torch.equal(tree, buf.tree) and int(buf.tree[-1]) == int(leaves.sum()), c
    assert ring.counter > M and (leaves > 0).all()


ITERS, REAL_M = 3, 100


def _real(n, E, T, auto_reset, seed):
    """A small scripted-blue rollout whose games end inside it (tests/test_hip_ddpg_loop.py's), the red team's ring, appender and learner."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.learner import DDPGLearner
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=auto_reset)
    env.reset()
    torch.manual_seed(seed)
    actor = StackedActor(2 * n, 3 * n + 2, 4, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(100.0)
    ro = PolicyRollout(env, actor, T, noise_std=0.2, opponent=instinct.Team(env.possible_blue, env.possible_red, env))
    ro.start()
    buf = DeviceReplayBuffer(REAL_M, 64, env.possible_red, env.obs_size, env.obs_size * n, 4, device="cuda", seed=3)
    app = NStepAppender(buf, 3, GAMMA, T, E)
    mine = StackedActor(n, env.obs_size, 4, device="cuda")
    with torch.no_grad():
        for p in D.PARAMS:
            getattr(mine, p).copy_(getattr(actor, p)[:n])
    torch.manual_seed(100 + seed)
    critic = StackedActor(n, D.width(n, env.obs_size, 4, False), 1, device="cuda")
    learner = DDPGLearner(buf, mine, critic, critic_input="own", **dict(D.KW, gamma=app.bootstrap_gamma))
    return env, ro, buf, app, learner


@pytest.mark.parametrize("auto_reset", [True, False])
def test_a_real_rollout_eager_and_captured_with_a_learner_behind_it(auto_reset):
    n, E, T, cols = 2, 24, 16, range(2)
    env, ro, buf, app, learner = _real(n, E, T, auto_reset, 42)
    _, ro2, buf2, app2, learner2 = _real(n, E, T, auto_reset, 42)
    assert learner.gamma == app.bootstrap_gamma == float(U.gamma_chain(GAMMA, 3)[3])
    ref, ring = U.NStepRef(3, GAMMA, E, n, env.obs_size, 4), U.RingRef(REAL_M, n, env.obs_size, 4)
    ended = 0
    for it in range(ITERS):
        ro.run()
        stored = app.append_rollout(ro, cols)
        learner.update()
        rec = {key: getattr(ro, name).cpu().numpy() for key, name in (("obs", "obs"), ("act", "scores"), ("rew", "rew"), ("done", "_done"),
                                                                       ("env_done", "env_done"))}
        out = ref.fold(*U.team(rec, 0, n, 4))
        assert int(stored) == ring.append(out, out["skip"]), it
        U.assert_ring_equal(buf, ring, it)
        assert bool(torch.isfinite(learner.stats).all()), it
        ended += int((rec["env_done"][1:] != 0).sum())
    print("game ends inside the rollouts:", ended, "rows stored:", ring.counter)
    assert ended > 0 and ring.counter > REAL_M                                # games ended inside the rollouts, the ring wrapped
    ro2.capture(then=lambda: app2.append_rollout(ro2, cols))
    learner2.capture()
    for it in range(ITERS):
        ro2.run()
        learner2.update()
        assert bool(torch.isfinite(learner2.stats).all()), it
    torch.cuda.synchronize()
    for f in ("actor_states", "actor_new_states", "action_mem", "rew_mem"):
        assert torch.equal(getattr(buf, f).view(torch.int32), getattr(buf2, f).view(torch.int32)), f
    assert torch.equal(buf.done_mem, buf2.done_mem) and buf.mem_cntr == buf2.mem_cntr
    assert torch.equal(app.carry_valid, app2.carry_valid) and torch.equal(app._c_obs, app2._c_obs)
