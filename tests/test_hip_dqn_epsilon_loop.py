"""The documented loop of tests/test_hip_dqn_loop.py with the algorithm's own behaviour policy: the rollout is
PolicyRollout(epsilon=EpsilonSchedule(1.0, 0.1, steps = 2 T)) -- no other noise -- on 64 games of a discrete 2v2 env with auto-reset,
T = 8; capture() on the empty ring, then three iterations of run, replay.NStepAppender(n = 3) into a PrioritizedReplayBuffer, update,
publish, each against an eager twin (a second env, rollout, schedule, ring and appender with the same seeds, the rollout run eagerly, the
update by hand from the public primitives), bit for bit after every iteration -- the exploration record, the rates and the schedule's
counter included, and the rates against the numpy restatement.  At the end the ring's stored score rows, the random one-hot rows among
them, go through dqn_head: the action it replays is argmax4 of the stored row.  The same loop once with QMIXLearner."""
import numpy as np
import pytest
import torch

import dqn_util as Q
import epsilon_util as EU
import offpolicy_loop_util as LU
import offpolicy_util as O
import qmix_util as X

pytestmark = pytest.mark.gpu

START, END = 1.0, 0.1


def _loop(c, make_learners, snapshot, finite):
    from deep_rl_battlespace_amd import replay
    from deep_rl_battlespace_amd.rollout import EpsilonSchedule
    n, seed, steps = c.n, c.seed, 2 * c.T
    make = lambda: LU.rollout(n, c.E, c.T, False, True, seed, "red", "f32", noise_std=0.0,                   # noqa: E731
                              epsilon=lambda _n: EpsilonSchedule(START, END, steps))
    (env, ro), (_, tw) = make(), make()
    cols = range(n)
    other = [a for a in range(2 * n) if a not in cols]
    bufs = tuple(replay.PrioritizedReplayBuffer(c.M, c.B, env.possible_red, env.obs_size, env.obs_size * n, 4, device="cuda", seed=3) for _ in range(2))
    buf, buf2 = bufs
    apps = tuple(replay.NStepAppender(b, c.nstep, Q.GAMMA, c.T, c.E) for b in bufs)
    app, app2 = apps
    learner, hand = make_learners(ro, env, bufs, app.bootstrap_gamma)
    start, w0 = snapshot(learner), ro.fused.weights.clone()
    assert learner.capture() is learner and O.differing(start, snapshot(learner)) == []
    ro.capture()
    explored_rows = 0
    for it in range(c.iters):
        rate = EU.schedule(it * c.T, START, END, steps)
        assert bool((ro.epsilon == float(rate)).all()) and bool((tw.epsilon == float(rate)).all()), it
        ro.run()
        app.append_rollout(ro, cols)
        learner.update()
        learner.publish(ro, cols)
        tw.run()                                        # eagerly: the twin's rollout is never captured
        app2.append_rollout(tw, cols)
        hand.update()
        LU.twin_publish(hand, tw, cols)
        torch.cuda.synchronize()
        assert torch.equal(ro.fused.weights[:n].view(torch.int32), learner._blob_q.view(torch.int32)), it
        assert torch.equal(ro.fused.weights[other].view(torch.int32), w0[other].view(torch.int32)), it
        LU.same(it, ro, tw, buf, buf2, learner, hand, snapshot, apps)
        for f in ("_explored", "epsilon"):
            assert torch.equal(getattr(ro, f).view(torch.uint8).view(-1), getattr(tw, f).view(torch.uint8).view(-1)), (it, f)
        assert int(ro._eps_schedule.count) == int(tw._eps_schedule.count) == (it + 1) * c.T
        assert float(ro.epsilon[0]) == float(EU.schedule((it + 1) * c.T, START, END, steps)), it
        assert not bool(ro.explored[:, :, other].any())                                   # the scripted team's rows
        mine = ro.explored[:, :, :n]
        explored_rows += int(mine.sum())
        assert bool(mine.all()) if it == 0 else 0 < int(mine.sum()) < mine.numel(), it    # rate 1.0, then 0.55, then 0.1
        hot = ro.scores[:, :, :n][mine]
        assert bool((hot.abs() == 1.0).all()) and bool(((hot == 1.0).sum(-1) == 1).all()), it
        LU.tree_is_exact(buf, it)
        assert finite(learner), it
    assert int(learner.step) == c.updates * c.iters == int(hand.step)
    assert O.differing(start, snapshot(learner)) != [] and explored_rows > c.T * c.E * n
    return buf, learner


def _replayed_actions_are_the_stored_rows_argmax(buf):
    """dqn_head on the ring's own rows: with y_cur = the same four distinct values in every row, q = q_scale * y_cur[a] names the action
    a the head recovered from the stored score row -- argmax4 of it, for greedy and random rows alike."""
    from deep_rl_battlespace_amd import learner as L
    rows = min(buf.mem_cntr, buf.action_mem.shape[0])
    act = buf.action_mem[:rows].contiguous()
    nA = act.shape[1]
    y = torch.tensor([0.125, 0.25, 0.5, 0.75], device="cuda").expand(rows, nA, 4).contiguous()
    zero = torch.zeros((rows, nA), device="cuda")
    out = L.dqn_head(y, torch.zeros_like(y), act, zero, torch.zeros((rows, nA), dtype=torch.uint8, device="cuda"), 0.0, q_scale=4.0)
    torch.cuda.synchronize()
    got = (out.q.cpu().numpy()[..., None] == (4.0 * y.cpu().numpy())).argmax(-1)
    a = act.cpu().numpy()
    want = Q.argmax4(a)
    assert np.array_equal(got, want)
    one_hot = (np.abs(a) == 1.0).all(-1) & ((a == 1.0).sum(-1) == 1)
    assert one_hot.any() and set(np.unique(want[one_hot])) == {0, 1, 2, 3}
    return int(one_hot.sum()), rows * nA


@pytest.mark.parametrize("mix", Q.LOOP["mixes"])
def test_the_dqn_loop_on_an_annealed_epsilon_greedy_rollout_equals_its_eager_twin(mix):
    from deep_rl_battlespace_amd import learner as L
    c = LU.case_of(dict(Q.LOOP, cont=False, one_launch=True, team="red", central=False, prio=True))

    def learners(ro, env, bufs, gamma_n):
        qnet, = LU.team_nets(ro, range(c.n), False, c.seed, critics=0)
        kw = dict(Q.KW, mix=mix, updates=c.updates, gamma=gamma_n)
        return L.DQNLearner(bufs[0], qnet, **kw), Q.Hand(bufs[1], O.gpu_copy(qnet), **kw)
    buf, learner = _loop(c, learners, Q.snapshot, lambda x: bool(torch.isfinite(x.stats).all() and torch.isfinite(x.step_stats).all()))
    hot, rows = _replayed_actions_are_the_stored_rows_argmax(buf)
    print(f"epsilon loop {mix}: {buf.mem_cntr} rows stored, {hot} of {rows} stored score rows one-hot")


def test_the_qmix_loop_on_an_annealed_epsilon_greedy_rollout_equals_its_eager_twin():
    from deep_rl_battlespace_amd import learner as L
    from deep_rl_battlespace_amd.rollout import StackedActor
    c = LU.case_of(dict(X.LOOP, cont=False, one_launch=True, team="red", central=False, prio=True))
    embed = X.LOOP["embed"]

    def learners(ro, env, bufs, gamma_n):
        qnet, = LU.team_nets(ro, range(c.n), False, c.seed, critics=0)
        torch.manual_seed(200 + c.seed)
        mixer = StackedActor(X.members(c.n, embed), c.n * env.obs_size, 4, device="cuda")
        kw = dict(X.KW, embed=embed, updates=c.updates, gamma=gamma_n)
        return L.QMIXLearner(bufs[0], qnet, mixer, **kw), X.Hand(bufs[1], O.gpu_copy(qnet), O.gpu_copy(mixer), **kw)
    buf, learner = _loop(c, learners, X.snapshot,
                         lambda x: bool(torch.isfinite(x.stats).all() and torch.isfinite(x.step_stats).all() and torch.isfinite(x.step_stats_mixer).all()))
    hot, rows = _replayed_actions_are_the_stored_rows_argmax(buf)
    print(f"epsilon QMIX loop: {buf.mem_cntr} rows stored, {hot} of {rows} stored score rows one-hot")
