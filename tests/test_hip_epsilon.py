"""Epsilon-greedy exploration on the MI355X (BsxActorNoise.epsilon / .explored, bsx_epsilon_advance, PolicyRollout(epsilon=),
rollout.EpsilonSchedule), held bit for bit to the host restatement of tests/epsilon_util.py: the row finish of bsx_actor_forward at the
ragged sizes of the guard tests in all three precisions, with per-plane rates 0, 1, 0.3 and NaN, a non-zero env_offset and seq_base, and
injected uniforms; the three forms of one game (the per-tick graph, chains=2, one launch) against each other and against the restatement
applied to a greedy forward of every tick's observations; a scripted opponent's rows; the edge rates; a live rate under a captured graph;
the on-device schedule after every replay; guard canaries around `epsilon`, `explored` and the schedule's counter."""
import numpy as np
import pytest
import torch

import epsilon_util as EU
from guard_util import Buffers

pytestmark = pytest.mark.gpu

SEED, T = 23, 4
RAGGED = ((1, 33), (2, 5), (3, 7), (4, 5))           # (team size, games): the ragged sizes of tests/test_hip_guards.py
PATTERN = (0.0, 1.0, 0.3, float("nan"))
f32, u8, i64 = torch.float32, torch.uint8, torch.int64


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_np(t, want):
    got = np.ascontiguousarray(t.detach().cpu().numpy())
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def _actor(n, seed=SEED):
    from deep_rl_battlespace_amd.rollout import StackedActor
    torch.manual_seed(seed + n)
    actor = StackedActor(2 * n, 3 * n + 2, 4, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(60.0)
    return actor


def _rollout(n, E, opponent=False, **kw):
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=SEED, auto_reset=True)
    env.reset()
    opp = instinct.Team(env.possible_blue, env.possible_red, env) if opponent else None
    ro = PolicyRollout(env, _actor(n), T, seed=SEED + 1, opponent=opp, **kw)
    ro.start()
    return ro


def _restated_ticks(ro, run, cols=None):
    """(scores, explored) [T, E, A, ..] that the rule gives on a greedy forward of every recorded obs[t] at sequence run * T + t."""
    E, A = ro.env.n_envs, ro.env._A
    eps = ro.epsilon.cpu().numpy()
    tmp = torch.empty((E, A, 4), dtype=f32, device="cuda")
    sc, ex = [], []
    for t in range(T):
        ro.fused.forward_into(ro.obs[t], tmp, seq=0)
        s, x = EU.apply(tmp.cpu().numpy(), eps, ro.fused.seed, run * T + t, env_offset=ro.env.env_offset)
        sc.append(s); ex.append(x)
    return np.stack(sc), np.stack(ex)


@pytest.mark.parametrize("n,E", RAGGED)
def test_the_row_finish_is_the_restated_rule_bit_for_bit(n, E):
    from deep_rl_battlespace_amd.rollout import FusedActor
    A, D, off, seq, base = 2 * n, 3 * n + 2, 1000003, 5, 77
    actor = _actor(n)
    g = torch.Generator().manual_seed(E + 10 * n)
    obs = (torch.rand((E, A, D), generator=g) * 2 - 0.5).cuda()
    u = torch.rand((E, A, 4), generator=g).cuda()
    seq_base = torch.full((1,), base, dtype=i64, device="cuda")
    explored_rows = 0
    for precision in ("f32", "bf16x3", "bf16x6"):
        fa = FusedActor(actor, n, seed=SEED, precision=precision, env_offset=off)
        greedy = torch.full((E, A, 4), -7.0, dtype=f32, device="cuda")
        fa.forward_into(obs, greedy, seq=seq, seq_base=seq_base)
        for shift in (0, 2):
            eps = torch.tensor([PATTERN[(a + shift) % 4] for a in range(A)], dtype=f32, device="cuda")
            for inject in (None, u):
                got, ex = torch.full((E, A, 4), -7.0, dtype=f32, device="cuda"), torch.full((E, A), 7, dtype=u8, device="cuda")
                fa.forward_into(obs, got, seq=seq, seq_base=seq_base, epsilon=dict(value=eps, explored=ex, **({} if inject is None else dict(u=inject))))
                want, want_ex = EU.apply(greedy.cpu().numpy(), eps.cpu().numpy(), SEED, seq + base, env_offset=off,
                                         u=None if inject is None else inject.cpu().numpy())
                what = (n, E, precision, shift, inject is not None)
                assert _same_np(ex, want_ex), what
                assert _same_np(got, want), what
                explored_rows += int(want_ex.sum())
                for a in range(A):                   # the edge rates, whatever the draws: 0 and NaN never explore, 1 always does
                    e = PATTERN[(a + shift) % 4]
                    if e != 0.3:
                        assert bool((ex[:, a] == (1 if e == 1.0 else 0)).all()), what
                # without a record the rows are the same
                bare = torch.empty_like(got)
                fa.forward_into(obs, bare, seq=seq, seq_base=seq_base, epsilon=dict(value=eps, **({} if inject is None else dict(u=inject))))
                assert _same(bare, got), what
    assert explored_rows > 0


def _three_forms(n, E):
    forms = (dict(chains=1), dict(chains=2), dict(one_launch=True))
    ros = [_rollout(n, E, epsilon=0.3, **kw).capture() for kw in forms]
    assert ros[0].chains == 1 and ros[1].chains == 2 and ros[2].one_launch
    seen = []
    for run in range(2):
        for ro in ros:
            ro.run()
        torch.cuda.synchronize()
        per_tick = ros[0]
        for ro, kw in zip(ros[1:], forms[1:]):
            for f in ("obs", "scores", "rew", "done", "explored", "env_done"):
                assert _same(getattr(ro, f), getattr(per_tick, f)), (n, E, run, kw, f)
        want, want_ex = _restated_ticks(per_tick, run)
        assert _same_np(per_tick._explored, want_ex), (n, E, run)
        assert _same_np(per_tick.scores, want), (n, E, run)
        assert 0 < int(per_tick.explored.sum()) < per_tick.explored.numel()
        seen.append(per_tick._explored.clone())
        assert int(per_tick._seq_base) == (run + 1) * T
    assert not torch.equal(seen[0], seen[1])         # the second replay drew fresh keys


@pytest.mark.parametrize("n,E", RAGGED + ((1, 289),))      # 289 games: chains=2 really is two ranges (256 + 33)
def test_three_forms_play_one_game_and_every_tick_is_the_restated_rule(n, E):
    _three_forms(n, E)


@pytest.mark.parametrize("one_launch", [False, True])
def test_a_scripted_opponents_rows_are_untouched_and_the_learned_team_explores(one_launch):
    n, E = 2, 37
    ro = _rollout(n, E, opponent=True, epsilon=0.5, one_launch=one_launch).capture()
    mine, theirs = slice(0, n), slice(n, 2 * n)
    tmp = torch.empty((E, 2 * n, 4), dtype=f32, device="cuda")
    for run in range(2):
        ro.run()
        torch.cuda.synchronize()
        want, want_ex = _restated_ticks(ro, run)
        assert _same_np(ro.scores[:, :, mine], want[:, :, mine]) and _same_np(ro._explored[:, :, mine], want_ex[:, :, mine]), run
        assert not bool(ro.explored[:, :, theirs].any()) and 0 < int(ro.explored[:, :, mine].sum()) < T * E * n
        for t in range(T):
            tmp.fill_(-7.0)
            ro.opponent.write_actions(out=tmp, obs=ro.obs[t])
            assert _same(ro.scores[t][:, theirs], tmp[:, theirs]), (run, t)


@pytest.mark.parametrize("one_launch", [False, True])
def test_rates_none_and_zero_play_the_greedy_rollout_and_one_plays_only_random_actions(one_launch):
    n, E = 2, 37
    greedy, zero, one = (_rollout(n, E, one_launch=one_launch, **kw).capture() for kw in ({}, dict(epsilon=0.0), dict(epsilon=1.0)))
    for run in range(2):
        for ro in (greedy, zero, one):
            ro.run()
        torch.cuda.synchronize()
        for f in ("obs", "scores", "rew", "done", "env_done"):
            assert _same(getattr(zero, f), getattr(greedy, f)), (run, f)
        assert greedy.explored is None and not bool(zero.explored.any()) and bool(one.explored.all())
        s = one.scores
        assert bool((s.abs() == 1.0).all()) and bool(((s == 1.0).sum(-1) == 1).all())
        assert _same_np(one.scores, _restated_ticks(one, run)[0])
    assert len(torch.unique(one.scores.argmax(-1))) == 4


def test_a_live_rate_changes_the_next_replay_with_no_recapture():
    ro = _rollout(2, 37, epsilon=0.0).capture()
    graph = ro.graph
    ro.run(); torch.cuda.synchronize()
    assert not bool(ro.explored.any())
    ro.epsilon.fill_(1.0)
    ro.run(); torch.cuda.synchronize()
    assert ro.graph is graph and bool(ro.explored.all())
    ro.epsilon.copy_(torch.tensor([0.0, 1.0, 0.0, 1.0], device="cuda"))
    ro.run(); torch.cuda.synchronize()
    assert bool(ro.explored[:, :, 1::2].all()) and not bool(ro.explored[:, :, 0::2].any())


@pytest.mark.parametrize("one_launch", [False, True])
def test_a_captured_rollout_anneals_by_the_schedule_with_no_host_work(one_launch):
    from deep_rl_battlespace_amd.rollout import EpsilonSchedule
    start, end, steps = 1.0, 0.1, 5 * T
    sched = EpsilonSchedule(start, end, steps)
    ro = _rollout(2, 37, epsilon=sched, one_launch=one_launch)
    assert ro.epsilon is sched.value and int(sched.count) == 0 and bool((ro.epsilon == 1.0).all())
    ro.capture()
    for i in range(7):
        rate = ro.epsilon.clone()
        ro.run(); torch.cuda.synchronize()
        assert int(sched.count) == (i + 1) * T
        want = EU.schedule((i + 1) * T, start, end, steps)
        assert _same_np(ro.epsilon, np.full(4, want, np.float32)), i
        # the run played at the rate the runs before it left
        assert _same_np(ro._explored, _restated_ticks(types_ns(ro, rate), i)[1]), i
    assert float(ro.epsilon[0]) == np.float32(end)
    sched.reset(3); torch.cuda.synchronize()
    assert int(sched.count) == 3 and _same_np(ro.epsilon, np.full(4, EU.schedule(3, start, end, steps), np.float32))
    ro.run(); torch.cuda.synchronize()
    assert int(sched.count) == 3 + T


def types_ns(ro, rate):
    """`ro` with another rate tensor, for _restated_ticks."""
    import types
    return types.SimpleNamespace(env=ro.env, epsilon=rate, fused=ro.fused, obs=ro.obs)


def test_the_schedule_kernel_linear_bit_for_bit_and_exponential_within_one_ulp_of_numpy():
    from deep_rl_battlespace_amd.rollout import EpsilonSchedule
    worst = 0
    for start, end, steps in ((1.0, 0.1, 20), (0.9, 0.05, 7), (0.25, 0.75, 1000003), (1.0, 0.0, 1)):
        counts = [0, 1, steps - 1, steps, steps + 5]
        lin = EpsilonSchedule(start, end, steps).bind(3, "cuda")
        for c in counts:
            lin.reset(c); torch.cuda.synchronize()
            assert int(lin.count) == c and _same_np(lin.value, np.full(3, EU.schedule(c, start, end, steps), np.float32)), (start, end, steps, c)
        lin.reset(0).advance(2).advance(3); torch.cuda.synchronize()
        assert int(lin.count) == 5 and _same_np(lin.value, np.full(3, EU.schedule(5, start, end, steps), np.float32))
        ex = EpsilonSchedule(start, end, steps, kind="exponential").bind(3, "cuda")
        for c in counts + [2 * steps, 10 * steps, 40 * steps]:
            ex.reset(c); torch.cuda.synchronize()
            got, want = ex.value.cpu().numpy(), EU.schedule(c, start, end, steps, "exponential")
            ulps = int(np.abs(got.view(np.int32).astype(np.int64) - np.int64(want.view(np.int32))).max())
            worst = max(worst, ulps)
            print(f"exp schedule start {start} end {end} steps {steps} count {c}: device {got[0]!r} numpy {want!r} ({ulps} float32 ulp)")
            assert ulps <= 1, (start, end, steps, c)
    print("worst float32 ulp distance of the exponential kind from numpy:", worst)


@pytest.mark.parametrize("n,E", RAGGED)
def test_nothing_is_written_outside_epsilon_explored_and_the_counter(n, E):
    from deep_rl_battlespace_amd.rollout import EpsilonSchedule, FusedActor
    A, D = 2 * n, 3 * n + 2
    # the stand-alone actor
    buf = Buffers(True)
    eps, ex, sc = buf("epsilon", A, f32, 0.5), buf("explored", (E, A), u8, 7), buf("scores", (E, A, 4), f32, -7.0)
    g = torch.Generator().manual_seed(n)
    obs = (torch.rand((E, A, D), generator=g) * 2 - 0.5).cuda()
    for precision in ("f32", "bf16x3", "bf16x6"):
        FusedActor(_actor(n), n, seed=SEED, precision=precision).forward_into(obs, sc, seq=1, epsilon=dict(value=eps, explored=ex))
    torch.cuda.synchronize()
    assert buf.stray() == [] and bool((ex <= 1).all()) and bool((eps == 0.5).all())
    # the schedule kernel
    sched = EpsilonSchedule(1.0, 0.1, 10).bind(A, "cuda")
    sched.value, sched.count = buf("schedule value", A, f32, -7.0), buf("schedule count", 1, i64, 0)
    sched.reset(2).advance(3); torch.cuda.synchronize()
    assert buf.stray() == [] and int(sched.count) == 5 and _same_np(sched.value, np.full(A, EU.schedule(5, 1.0, 0.1, 10), np.float32))
    # the one-launch rollout and the per-tick graph, their record and rates inside guard slabs
    for one_launch in (True, False):
        rate = buf(f"rate {one_launch}", A, f32, 0.5)
        ro = _rollout(n, E, epsilon=rate, one_launch=one_launch)
        ro._explored = buf(f"record {one_launch}", (T, E, A), u8, 7)
        ro.explored = ro._explored.view(torch.bool)
        ro.capture().run(); ro.run()
        torch.cuda.synchronize()
        assert buf.stray() == [] and bool((ro._explored <= 1).all()) and 0 < int(ro._explored.sum()) < T * E * A
        assert _same_np(ro._explored, _restated_ticks(ro, 1)[1]), (n, E, one_launch)
