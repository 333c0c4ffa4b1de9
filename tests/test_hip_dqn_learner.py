"""DQNLearner on the MI355X: an update is, bit for bit, the sequence of the public primitives written out by hand (tests/dqn_util.py:
Hand), for both mixes, on a plain and on a prioritised ring; a whole update from a target network that is not the network against
float64, the float32 torch composition as the yardstick; a captured update runs nothing, replays the eager updates bit for bit -- a
prioritised ring of 4 096 rows with its leaves, tree and max_priority included -- and allocates nothing; set_lr is seen by a replay;
sync() after an outside edit; publish() writes only its rows; the constructor's refusals; and a bandit on which the learner must find
the paying arm and end at its torch twin's loss.  The by-hand, float64 and capture tests also run the 3v3 team at B = 171, where the head
has three tiles and VDN rows lie across two of them."""
import numpy as np
import pytest
import torch

import ddpg_util as D
import dqn_util as Q
import offpolicy_util as O
import qlearn_util as QL
import yardstick_util as Y

pytestmark = pytest.mark.gpu

# (team, mix, prioritised, double, batch): every team with both mixes; single Q and the prioritised ring at the ends of the table; the
# 3v3 team at B = 171: three tiles in the head, the VDN rows 85 and 170 split between two of them (dqn_util.SPLIT_SHAPES)
HAND_CASES = [(t, m, False, True, Q.B) for t in Q.TEAMS for m in Q.MIXES] + \
    [(Q.TEAMS[1], "vdn", True, True, Q.B), (Q.TEAMS[3], "independent", True, True, Q.B), (Q.TEAMS[1], "independent", False, False, Q.B),
     (Q.TEAMS[2], "vdn", True, False, Q.B), (Q.TEAMS[2], "vdn", True, True, Q.B_SPLIT), (Q.TEAMS[2], "independent", False, True, Q.B_SPLIT)]


def _case_id(c):
    team, mix, prio, dbl, batch = c
    return Q.team_id(team, mix) + ("-prioritised" if prio else "") + ("" if dbl else "-single") + ("" if batch == Q.B else "-B%d" % batch)


@pytest.mark.parametrize("case", HAND_CASES, ids=_case_id)
def test_an_update_is_the_by_hand_sequence_of_the_public_primitives_bit_for_bit(case):
    team, mix, prio, dbl, batch = case
    learner, hand = Q.learner_and_hand(team, prio, batch_size=batch, mix=mix, double=dbl, updates=2)
    start = Q.snapshot(learner)
    assert O.differing(start, Q.snapshot(hand)) == []
    for call in range(2):
        stats = learner.update()
        hand.update()
        a, b = Q.snapshot(learner), Q.snapshot(hand)
        assert O.differing(a, b) == [], (call, O.differing(a, b))
        assert stats is learner.stats and stats.shape == (2, 8) and float(stats[1, 0]) == batch * team[0]
        assert learner.td.shape == (batch, team[0])
        assert torch.equal(learner.td.view(torch.int32), hand.td.view(torch.int32)) and torch.equal(learner.q.view(torch.int32), hand.q.view(torch.int32))
    assert int(learner.step) == 4 == int(learner.buffer._draws) and torch.equal(learner.buffer.last_idx, hand.buffer.last_idx)
    moved = set(O.differing(start, a))
    assert {"qnet.w1", "qnet.b3", "target_qnet.w2", "_blob_q", "_blob_tq", "adam.m", "adam.v", "stats", "step_stats", "step", "draws"} <= moved
    assert not prio or {"leaves", "tree", "max_priority"} <= moved
    for net, blob in ((learner.qnet, learner._blob_q), (learner.target_qnet, learner._blob_tq)):
        assert torch.equal(net.pack().view(torch.int32), blob.view(torch.int32))
    assert bool(torch.isfinite(learner.stats).all()) and [float(x) for x in learner.step_stats[:, 0]] == [3.0, 4.0]
    assert 0.0 < float(learner.stats[1, 5]) < 1.0 and 0.0 <= float(learner.stats[1, 7]) <= 1.0
    if mix == "vdn":
        assert torch.equal(learner.td, learner.td[:, :1].expand_as(learner.td)) and torch.equal(learner.q, learner.q[:, :1].expand_as(learner.q))
    if not dbl:
        assert not learner._y_on.any()                                              # without double Q the second online forward is skipped


@pytest.mark.parametrize("team,mix,batch", Q.STEP_CASES, ids=[Q.team_id(*c) for c in Q.STEP_CASES])
def test_a_whole_update_with_a_distinct_target_against_float64(team, mix, batch):
    """One whole update through the primitives (Hand.one, dqn_util.STEP_KW: double Q, Huber delta = 1) from a target network that is NOT
    the network, against dqn_util.stepped_case's float64 reference with the same computation in float32 on the CPU as the yardstick:
    the gradient row, the step and the Polyak target -- each pooled over its ten tensors, ddpg_util.check_step's bars: the project's
    (2, 4), no wider factor -- and the statistics.  Rows near a kink carry no weight (tests/test_dqn_cpu.py holds the case to its cap).
    BSX_DQN_RATIOS_OUT names a file the measured ratios are appended to (profiles/dqn_float64.json keeps them)."""
    from deep_rl_battlespace_amd import learner as L
    c = Q.stepped_case(team, mix, batch)
    assert c.share <= Q.KINK_CAP
    kw = {k: v for k, v in Q.STEP_KW.items()}
    hand = Q.Hand(O.ring(c.rows, batch), O.gpu_copy(c.qnet), mix=mix, double=True, updates=1, **kw)
    with torch.no_grad():
        for p in D.PARAMS:
            getattr(hand.target_qnet, p).copy_(getattr(c.target, p))
        hand.target_qnet.pack(out=hand._blob_tq)
    row = hand.one(*O.sample_is(hand, c.idx, c.batch), 0, weight=c.w.cuda())
    torch.cuda.synchronize()
    sid, rec = Q.team_id(team, mix, batch), {}
    print("DQN", sid)
    got = O.grad_arrays(row, 4)
    tens = lambda g: {"g": [g[p] for p in D.PARAMS]}                                # noqa: E731
    D.check_step(tens(got), tens(c.ref["g"]), tens(c.yard["g"]), "row", rec, names=("g",))
    D.check_step(Q.step_arrays(hand), c.ref["net"], c.yard["net"], "qnet", rec)
    st, norm = hand.step_stats[0].cpu().numpy(), float(row.double().square().sum().sqrt())
    coef = min(1.0, float(np.float32(kw["max_grad_norm"])) / (norm + 1e-6))
    assert st[0] == 1 and abs(st[1] - norm) <= 1e-10 * norm and abs(st[2] - coef) <= 1e-10 * coef and coef < 1.0, (st, norm, coef)
    bad = Q.stats_out_of_bounds(hand.stats[0].cpu().numpy(), c.stats, c.e_stats, f"DQN {sid}")
    assert not bad, bad
    assert torch.equal(hand.qnet.pack().view(torch.int32), hand._blob_q.view(torch.int32))
    O.append_ratios("BSX_DQN_RATIOS_OUT", sid, rec)
    assert isinstance(L.DQN_STATS, tuple)


def _prio_rows(N=4096, team=Q.TEAMS[1]):
    return D.ring_rows(N, team[0], team[1], 4, 77)


@pytest.mark.parametrize("mix,prio,team,batch", [("independent", False, Q.TEAMS[1], Q.B), ("vdn", False, Q.TEAMS[1], Q.B),
                                                 ("independent", True, Q.TEAMS[1], Q.B), ("vdn", True, Q.TEAMS[1], Q.B),
                                                 ("vdn", True, Q.TEAMS[2], Q.B_SPLIT)],
                         ids=["independent", "vdn", "independent-prioritised-4096", "vdn-prioritised-4096", "vdn-prioritised-4096-nA3-B171"])
def test_a_captured_update_runs_nothing_replays_the_eager_updates_bit_for_bit_and_allocates_nothing(mix, prio, team, batch):
    """Four replays against four eager calls: parameters, targets, moments, blobs, statistics, the draw counter and, on the prioritised
    ring of 4 096 rows, leaves, tree and max_priority, exact after every one; capture() undoes its warm-up.  The last case is the 3v3
    team at B = 171: a head of three tiles with split VDN rows inside the graph."""
    rows = _prio_rows(team=team) if prio else None
    (captured, _), (eager, _) = (Q.learner_and_hand(team, prio, rows=rows, batch_size=batch, mix=mix, updates=2) for _ in range(2))
    QL.captured_update(captured, eager, prio)


def test_set_lr_is_seen_by_a_replay_and_sync_repacks_after_an_outside_edit():
    (a, _), (b, _) = (Q.learner_and_hand(Q.TEAMS[1], mix="vdn") for _ in range(2))
    QL.set_lr_and_sync(a, b)


def test_publish_writes_only_its_rows_of_the_rollouts_blob():
    from deep_rl_battlespace_amd import learner as L
    QL.publish_rows(lambda ring, qnet: L.DQNLearner(ring, qnet, **Q.KW), Q.B)


def test_the_constructor_refuses_what_it_cannot_learn_from():
    from deep_rl_battlespace_amd import learner as L
    from deep_rl_battlespace_amd.rollout import StackedActor
    team = Q.TEAMS[1]
    rows4, rows3 = D.ring_rows(128, *team, 4, 1), D.ring_rows(128, *team, 3, 1)
    net = lambda *s: StackedActor(*s, device="cuda")                                # noqa: E731
    with pytest.raises(ValueError, match="n_actions == 4"):
        L.DQNLearner(O.ring(rows3, 32), net(*team, 3), q_scale=2.0)
    buf = O.ring(rows4, 32)
    for bad in (net(team[0], team[1], 3), net(team[0], team[1] + 1, 4), net(team[0] + 1, team[1], 4)):
        with pytest.raises(ValueError, match="qnet must be a StackedActor"):
            L.DQNLearner(buf, bad, q_scale=2.0)
    for kw, match in ((dict(mix="qmix", q_scale=2.0), "mix must be"), (dict(q_scale=0.0), "q_scale"), (dict(q_scale=-1.0), "q_scale"),
                      (dict(q_scale=float("nan")), "q_scale"), (dict(q_scale=2.0, huber_delta=-0.1), "huber_delta")):
        with pytest.raises(ValueError, match=match):
            L.DQNLearner(buf, net(*team, 4), **kw)
    with pytest.raises(TypeError):
        L.DQNLearner(buf, net(*team, 4))
    assert isinstance(L.DQNLearner(buf, net(*team, 4), q_scale=2.0), L.DQNLearner)


@pytest.mark.parametrize("mix", Q.MIXES)
def test_on_a_bandit_the_learner_finds_the_paying_arm_and_ends_at_its_torch_twins_loss(mix):
    """dqn_util's bandit (four arms, one-step rows, nA = 2; N = 100 updates and probes with |o_0| >= 0.1: chosen on the CPU with the
    float32 torch composition alone, tests/test_dqn_cpu.py re-runs it).  The learner runs N eager updates; its torch twin runs the SAME
    N updates on the learner's own draws, on the CPU.  At the end the learner's greedy action -- argmax4 of its own forward kernel -- is
    the paying arm on every probe observation, and its last loss lies within yardstick_util.scalar_bound of the float64 twin's: 4 x the
    float32 twin's own error against float64, the largest over the draws' rows in the given order and in 4 permuted ones."""
    from deep_rl_battlespace_amd import learner as L
    b = Q.BANDIT
    rows, probe = Q.bandit_rows()
    learner = L.DQNLearner(O.ring(rows, b["B"]), O.gpu_copy(Q.bandit_qnet()), mix=mix, q_scale=b["q_scale"], huber_delta=b["huber_delta"],
                           gamma=Q.GAMMA, tau=b["tau"], lr=b["lr"])
    draws, losses = [], []
    for _ in range(b["N"]):
        stats = learner.update()
        draws.append(learner.buffer.last_idx.clone())
        losses.append(stats[0, 1].clone())
    torch.cuda.synchronize()
    draws, losses = [d.cpu() for d in draws], [float(x) for x in losses]
    y4 = O.Hand.forward(None, learner._blob_q, probe.cuda().contiguous()).cpu().numpy()
    assert np.array_equal(Q.argmax4(y4), Q.bandit_best(probe).numpy())
    ref = Q.bandit_twin(mix, draws, torch.float64)[1]
    own = 0.0
    for order in Y.row_orders(b["B"], 4):
        twin = Q.bandit_twin(mix, [d if order is None else d[order] for d in draws], torch.float32)[1]
        own = max(own, abs(twin[-1] - ref[-1]))
    tol = Y.scalar_bound(ref[-1], own)
    print(f"bandit {mix}, N = {b['N']}: loss {losses[0]:.4f} -> {losses[-1]:.6e}; float64 twin {ref[-1]:.6e}; |difference| "
          f"{abs(losses[-1] - ref[-1]):.3e}, the float32 twin's own (5 row orders) {own:.3e}, bound {tol:.3e}")
    assert abs(losses[0] - ref[0]) <= 1e-5 * ref[0] and losses[-1] < 0.05 * losses[0]
    assert abs(losses[-1] - ref[-1]) <= tol
