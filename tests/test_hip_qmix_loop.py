"""The loop of QMIXLearner's docstring on real rollouts, on the MI355X, through tests/offpolicy_loop_util.py's rollout, twin publish and
comparison: 64 games of a discrete 2v2 env with auto-reset, T = 8, noise_std = 0.3; capture() on the empty ring, then three iterations
of run, replay.NStepAppender(n = 3) into a PrioritizedReplayBuffer, update, publish -- each against an eager twin (a second env, rollout,
ring and appender with the same seeds, the update by hand from the public primitives), bit for bit after every iteration, the ring's
leaves, tree, max_priority and weights and the appenders' carry included.  Then the design's claim: execution stays decentralised --
on a fresh run without noise of the published Q network, what the rollout's actor kernel scored is, bit for bit, the learner's own
forward on the same observations, so each plane plays its own arg-max and the mixer never leaves the learner.
(offpolicy_loop_util.documented_loop itself is written round an actor and its critics; this learner's second network is no critic, so
the loop is spelled out here with the harness's parts, as tests/test_hip_dqn_loop.py does.)"""
import numpy as np
import pytest
import torch

import offpolicy_loop_util as LU
import offpolicy_util as O
import qmix_util as X

pytestmark = pytest.mark.gpu


def test_the_documented_loop_equals_its_eager_twin_and_the_published_rollout_plays_each_planes_own_greedy_action():
    from deep_rl_battlespace_amd import learner as L
    from deep_rl_battlespace_amd import replay
    from deep_rl_battlespace_amd.rollout import StackedActor
    c = LU.case_of(dict(X.LOOP, cont=False, one_launch=True, team="red", central=False, prio=True))
    n, seed, embed = c.n, c.seed, X.LOOP["embed"]
    make = lambda s=seed, **kw: LU.rollout(n, c.E, c.T, False, True, s, "red", "f32", **{"noise_std": c.noise_std, **kw})     # noqa: E731
    (env, ro), (_, tw) = make(), make()
    cols = range(n)
    other = [a for a in range(2 * n) if a not in cols]
    bufs = tuple(replay.PrioritizedReplayBuffer(c.M, c.B, env.possible_red, env.obs_size, env.obs_size * n, 4, device="cuda", seed=3) for _ in range(2))
    buf, buf2 = bufs
    apps = tuple(replay.NStepAppender(b, c.nstep, X.GAMMA, c.T, c.E) for b in bufs)
    app, app2 = apps
    assert app.bootstrap_gamma < X.GAMMA
    qnet, = LU.team_nets(ro, cols, False, seed, critics=0)
    torch.manual_seed(200 + seed)
    mixer = StackedActor(X.members(n, embed), n * env.obs_size, 4, device="cuda")
    kw = dict(X.KW, embed=embed, updates=c.updates, gamma=app.bootstrap_gamma)    # behind the fold: the appender's gamma^n
    learner, hand = L.QMIXLearner(buf, qnet, mixer, **kw), X.Hand(buf2, O.gpu_copy(qnet), O.gpu_copy(mixer), **kw)
    start, w0 = X.snapshot(learner), ro.fused.weights.clone()
    assert learner.capture() is learner and O.differing(start, X.snapshot(learner)) == []      # on the empty ring, and it ran nothing
    assert buf.mem_cntr == 0 and O.differing(start, X.snapshot(hand)) == [] and int(buf.tree[-1]) == 0 and int(buf.max_priority) == LU.ONE
    ro.capture()
    for it in range(c.iters):
        ro.run()
        app.append_rollout(ro, cols)
        learner.update()
        learner.publish(ro, cols)
        tw.run()
        app2.append_rollout(tw, cols)
        hand.update()
        LU.twin_publish(hand, tw, cols)
        torch.cuda.synchronize()
        assert torch.equal(ro.fused.weights[:n].view(torch.int32), learner._blob_q.view(torch.int32)), it
        assert torch.equal(ro.fused.weights[other].view(torch.int32), w0[other].view(torch.int32)), it
        LU.same(it, ro, tw, buf, buf2, learner, hand, X.snapshot, apps)
        LU.tree_is_exact(buf, it)
        assert bool(torch.isfinite(learner.stats).all() and torch.isfinite(learner.step_stats).all() and torch.isfinite(learner.step_stats_mixer).all()), it
        assert float(learner.stats[-1, 0]) == c.B and 0 < int(buf._stored) <= buf.mem_cntr
    assert int(learner.step) == c.updates * c.iters == int(buf._draws) == int(hand.step) == int(learner.step_mixer)
    moved = O.differing(start, X.snapshot(learner))
    assert "mixer.w1" in moved and "qnet.w1" in moved and int(buf.max_priority) & 0xFFFFFFFF >= LU.ONE
    # the published network on a fresh run without noise: the actor kernel's score rows are the learner's forward rows, bit for bit
    _, fresh = make(seed + 1, noise_std=0.0)
    learner.publish(fresh, cols)
    fresh.run()
    torch.cuda.synchronize()
    rows = 0
    for t in range(c.T):
        obs = fresh.obs[t][:, :n].contiguous()
        mine = O.Hand.forward(None, learner._blob_q, obs)
        played = fresh.scores[t][:, :n]
        assert torch.equal(mine.view(torch.int32), played.contiguous().view(torch.int32)), t
        assert np.array_equal(X.argmax4(played.cpu().numpy()), X.argmax4(mine.cpu().numpy())), t
        rows += mine.shape[0] * mine.shape[1]
    print(f"QMIX loop: {buf.mem_cntr} rows stored, {rows} greedy rows compared")
    assert rows == c.T * c.E * n
