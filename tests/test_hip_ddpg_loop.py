"""The loop of DDPGLearner's docstring on real rollouts, on the MI355X: capture() on an empty ring, then run, append_rollout, update,
publish, over and over -- against an eager twin (a second env and rollout with the same seeds, a second ring with the same seed, the
update by hand from the public primitives, a publish that copies the parameter slices and packs afresh), bit for bit after every
iteration.  What only this loop reaches: a captured rollout replaying with published weights (blob rows copied in place under a frozen
pointer, the bfloat16 terms of the 64 x 64 layer included), the learner's graph reading a ring the append kernels of the same stream
have just written, a first batch larger than the ring's fill, the blue team's columns, and capture() before the first row exists."""
import gc
import types

import pytest
import torch

import ddpg_util as D
import offpolicy_util as O

pytestmark = pytest.mark.gpu

RING_FIELDS = ("actor_states", "actor_new_states", "action_mem", "rew_mem", "done_mem")
RECORDS = ("obs", "scores", "rew", "_done", "env_done")
# 1v1 and 3v3: E T of a rollout is smaller than B, so the first batches are larger than the ring's fill (2v2: 192 rows against 161).
# iters: enough for the ring to wrap (asserted)
CASES = {
    "1v1-continuous-one-launch-red-own": dict(n=1, cont=True, one_launch=True, team="red", central=False, E=32, T=8, M=600, B=300,
                                              precision="f32", then=False, iters=6),
    "2v2-discrete-graph-blue-central": dict(n=2, cont=False, one_launch=False, team="blue", central=True, E=24, T=8, M=500, B=161,
                                            precision="bf16x3", then=True, iters=6),
    "3v3-discrete-one-launch-red-central": dict(n=3, cont=False, one_launch=True, team="red", central=True, E=16, T=6, M=400, B=129,
                                                precision="f32", then=False, iters=8),
}


def _rollout(n, E, T, cont, one_launch, seed, team="red", precision="f32"):
    """tests/test_hip_replay_device.py's rollout: the other team scripted, head weights x 100 and noise 0.2, so that games end inside
    the rollouts.  team: the side the actor plays."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, continuous_actions=cont); env.reset()
    torch.manual_seed(seed)
    actor = StackedActor(2 * n, 3 * n + 2, 3 if cont else 4, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(100.0)
    mine, theirs = (env.possible_red, env.possible_blue) if team == "red" else (env.possible_blue, env.possible_red)
    ro = PolicyRollout(env, actor, T, noise_std=0.2, one_launch=one_launch, precision=precision, opponent=instinct.Team(theirs, mine, env))
    ro.start()
    return env, ro


def _team_nets(ro, cols, central, seed):
    """(actor, critic) of the team on the GPU: the team's slices of the rollout's actor, and a freshly initialised critic."""
    from deep_rl_battlespace_amd.rollout import StackedActor
    n, Do, k = len(cols), ro.actor.obs_len, ro.actor.n_actions
    actor = StackedActor(n, Do, k, device="cuda")
    with torch.no_grad():
        for p in D.PARAMS:
            getattr(actor, p).copy_(getattr(ro.actor, p)[cols[0]:cols[0] + n])
    torch.manual_seed(100 + seed)
    return actor, StackedActor(n, D.width(n, Do, k, central), 1, device="cuda")


def _twin_publish(hand, ro, cols):
    """The ten parameter slices into the rollout's actor, then a fresh pack of the whole actor."""
    with torch.no_grad():
        for p in D.PARAMS:
            getattr(ro.actor, p)[cols[0]:cols[0] + len(cols)].copy_(getattr(hand.actor, p))
    ro.fused.refresh()


def _same(what, ro, tw, buf, buf2, learner, hand):
    torch.cuda.synchronize()
    for f in RECORDS:
        assert torch.equal(getattr(ro, f), getattr(tw, f)), (what, f)
    for f in RING_FIELDS:
        assert torch.equal(getattr(buf, f), getattr(buf2, f)), (what, f)
    assert buf.mem_cntr == buf2.mem_cntr and torch.equal(buf.last_idx, buf2.last_idx), what
    a, b = D.snapshot(learner), D.snapshot(hand)
    assert O.differing(a, b) == [], (what, O.differing(a, b))
    assert torch.equal(ro.fused.weights.view(torch.int32), tw.fused.weights.view(torch.int32)), what


@pytest.mark.parametrize("name", list(CASES))
def test_the_documented_loop_equals_its_eager_twin_bit_for_bit(name):
    from deep_rl_battlespace_amd.learner import DDPGLearner
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    c = types.SimpleNamespace(**CASES[name])
    n, k, seed = c.n, 3 if c.cont else 4, 40 + c.n
    make = lambda: _rollout(n, c.E, c.T, c.cont, c.one_launch, seed, c.team, c.precision)     # noqa: E731
    (env, ro), (_, tw), (_, base) = make(), make(), make()                    # the loop's, the twin's, and one that is never published to
    cols = range(n) if c.team == "red" else range(n, 2 * n)
    agents = env.possible_red if c.team == "red" else env.possible_blue
    buf, buf2 = (DeviceReplayBuffer(c.M, c.B, agents, env.obs_size, env.obs_size * n, k, device="cuda", seed=3) for _ in range(2))
    actor, critic = _team_nets(ro, cols, c.central, seed)
    learner = DDPGLearner(buf, actor, critic, critic_input="central" if c.central else "own", updates=2, **D.KW)
    hand = D.Hand(buf2, O.gpu_copy(actor), O.gpu_copy(critic), c.central, updates=2, **D.KW)
    start = D.snapshot(learner)
    assert learner.capture() is learner and O.differing(start, D.snapshot(learner)) == []     # on the empty ring, and it ran nothing
    assert buf.mem_cntr == 0 and O.differing(start, D.snapshot(hand)) == []
    if c.then:
        ro.capture(then=lambda: buf.append_rollout(ro, cols))
    else:
        ro.capture()

    def loop():
        ro.run()
        if not c.then:
            buf.append_rollout(ro, cols)
        learner.update()
        learner.publish(ro, cols)

    def twin():
        tw.run()
        buf2.append_rollout(tw, cols)
        hand.update()
        _twin_publish(hand, tw, cols)

    dropped = sampled_done = False
    for it in range(c.iters - 2):
        loop()
        twin()
        _same(it, ro, tw, buf, buf2, learner, hand)
        dropped |= bool((ro.env_done[:c.T] != 0).any())
        sampled_done |= bool(buf._b_done.any())
        assert bool(torch.isfinite(learner.stats).all() and torch.isfinite(learner.step_stats_actor).all()
                    and torch.isfinite(learner.step_stats_critic).all()), it
        assert float(learner.stats[1, 0]) == c.B * n
        assert float(learner.stats[1, 5]) == float(buf._b_done.sum()) / (c.B * n)     # the last batch's share of finished rows
        if it == 0:
            kept = int(buf._stored)
            assert 0 < kept == buf.mem_cntr < c.M and int(buf.last_idx.max()) < kept      # drawn from the rows the first rollout left
            assert kept < c.B or c.E * c.T >= c.B                                         # ... a batch larger than the fill
            assert not torch.equal(ro.fused.weights[cols[0]], base.fused.weights[cols[0]])            # publish wrote the team's rows
        if it <= 1:
            # the first tick after the first publish: the same observations and noise keys as a rollout nobody published to, the
            # scripted team's rows the same, the team's rows not -- the captured rollout plays the published actor
            base.run()
            torch.cuda.synchronize()
            other = [a for a in range(2 * n) if a not in cols]
            assert torch.equal(base.obs[0], ro.obs[0]) and torch.equal(base.scores[0][:, other], ro.scores[0][:, other]), it
            assert torch.equal(base.scores[0][:, list(cols)], ro.scores[0][:, list(cols)]) == (it == 0), it
    del start
    torch.cuda.synchronize()
    gc.collect()                                                              # (as ppo_learner_util.allocates_nothing reads it)
    held = torch.cuda.memory_allocated()
    loop()
    loop()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held                              # the loop allocates nothing
    twin()
    twin()
    _same("end", ro, tw, buf, buf2, learner, hand)
    dropped |= bool((ro.env_done[:c.T] != 0).any())
    sampled_done |= bool(buf._b_done.any())
    assert dropped                                                            # games ended inside the rollouts: rows were left out
    assert sampled_done                                                       # finished rows reached the TD head
    assert buf.mem_cntr > c.M                                                 # the ring wrapped
    assert int(learner.step_critic) == 2 * c.iters == int(buf._draws)


def test_publish_and_append_refuse_another_teams_columns_and_another_action_count():
    from deep_rl_battlespace_amd.learner import DDPGLearner
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    env, ro = _rollout(2, 8, 2, False, False, 7)                              # 2v2 discrete: 4 env columns, 4 actions
    buf = DeviceReplayBuffer(64, 16, env.possible_red, env.obs_size, env.obs_size * 2, 4, device="cuda")
    actor, critic = _team_nets(ro, range(2), True, 7)
    learner = DDPGLearner(buf, actor, critic)
    ro.run()
    for cols in (range(1), range(3), range(4), [0, 2], range(3, 5)):          # a 1v1 team's, a 3v3 team's, both teams', a gap, past the end
        with pytest.raises(ValueError, match="contiguous range"):
            learner.publish(ro, cols)
        with pytest.raises(ValueError, match="contiguous range"):
            buf.append_rollout(ro, cols)
    assert buf.mem_cntr == 0
    _, cont = _rollout(2, 8, 2, True, False, 7)                               # the same env, continuous: an actor of 3 actions
    with pytest.raises(ValueError, match="4 actions"):
        learner.publish(cont, range(2))
    learner.publish(ro, range(2, 4))                                          # the blue columns take a team of the same shape
    assert int(buf.append_rollout(ro, range(2)).item()) > 0
