"""QMIXLearner on the MI355X: an update is, bit for bit, the sequence of the public primitives written out by hand (tests/qmix_util.py:
Hand) at every team up to (4, 14, embed 16), on a plain and on a prioritised ring, and at B = 257 and 300, two tiles in the head; a
whole update from target networks that are not the networks against float64, the float32 torch composition as the yardstick, pooled per
network; a captured update runs nothing, replays
the eager updates bit for bit -- a prioritised ring of 4 096 rows with its leaves, tree and max_priority included -- and allocates
nothing; set_lr is seen by a replay; sync() re-packs four blobs; publish() writes the Q network alone; and the one-step game an additive
mix cannot fit, which the learner must fit below half the additive floor and as well as its torch twin."""
import json
import os

import numpy as np
import pytest
import torch

import ddpg_util as D
import offpolicy_util as O
import qlearn_util as QL
import qmix_util as X
import yardstick_util as Y

pytestmark = pytest.mark.gpu

TEAM_IDS = dict(ids=X.team_id)
# (team, prioritised, double, batch): every team; single Q and the prioritised ring at the ends of the table; two tiles in the head
# inside a whole update at B = 257 and B = 300, the second at the widest mixer
HAND_CASES = [(t, False, True, X.B) for t in X.TEAMS] + [(X.TEAMS[1], True, True, X.B), (X.TEAMS[3], True, True, X.B), (X.TEAMS[1], False, False, X.B),
                                                         (X.TEAMS[2], True, False, X.B), (X.TEAMS[2], True, True, 257), (X.TEAMS[3], False, True, 300)]


def _case_id(c):
    team, prio, dbl, batch = c
    return X.team_id(team) + ("-prioritised" if prio else "") + ("" if dbl else "-single") + ("" if batch == X.B else "-B%d" % batch)


@pytest.mark.parametrize("case", HAND_CASES, ids=_case_id)
def test_an_update_is_the_by_hand_sequence_of_the_public_primitives_bit_for_bit(case):
    team, prio, dbl, batch = case
    learner, hand = X.learner_and_hand(team, prio, batch_size=batch, double=dbl, updates=2)
    start = X.snapshot(learner)
    assert O.differing(start, X.snapshot(hand)) == []
    for call in range(2):
        stats = learner.update()
        hand.update()
        a, b = X.snapshot(learner), X.snapshot(hand)
        assert O.differing(a, b) == [], (call, O.differing(a, b))
        assert stats is learner.stats and stats.shape == (2, 8) and float(stats[1, 0]) == batch
        assert torch.equal(learner.td.view(torch.int32), hand.td.view(torch.int32)) and torch.equal(learner.q.view(torch.int32), hand.q.view(torch.int32))
    assert int(learner.step) == 4 == int(learner.step_mixer) == int(learner.buffer._draws) and torch.equal(learner.buffer.last_idx, hand.buffer.last_idx)
    moved = set(O.differing(start, a))
    assert {"qnet.w1", "qnet.b3", "target_qnet.w2", "mixer.w1", "mixer.b3", "target_mixer.w2", "_blob_q", "_blob_tq", "_blob_m", "_blob_tm", "adam.m",
            "adam.v", "adam_mixer.m", "adam_mixer.v", "stats", "step_stats", "step_stats_mixer", "step", "step_mixer", "draws"} <= moved
    assert not prio or {"leaves", "tree", "max_priority"} <= moved
    for net, blob in ((learner.qnet, learner._blob_q), (learner.target_qnet, learner._blob_tq), (learner.mixer, learner._blob_m),
                      (learner.target_mixer, learner._blob_tm)):
        assert torch.equal(net.pack().view(torch.int32), blob.view(torch.int32))
    assert bool(torch.isfinite(learner.stats).all())
    assert [float(x) for x in learner.step_stats[:, 0]] == [3.0, 4.0] == [float(x) for x in learner.step_stats_mixer[:, 0]]
    assert 0.0 <= float(learner.stats[1, 5]) < 1.0 and 0.0 <= float(learner.stats[1, 7]) <= 1.0
    assert torch.equal(learner.td, learner.td[:, :1].expand_as(learner.td)) and torch.equal(learner.q, learner.q[:, :1].expand_as(learner.q))
    assert learner.members == X.members(team[0], team[2]) == learner.mixer.n_actors and learner._x_cur.shape == (batch, learner.members, team[0] * team[1])
    if not dbl:
        assert not learner._y_on.any()                                              # without double Q the second online forward is skipped


@pytest.mark.parametrize("team", X.FLOAT64_TEAMS, **TEAM_IDS)
def test_a_whole_update_with_distinct_targets_against_float64(team):
    """One whole update through the primitives (Hand.one, qmix_util.STEP_KW: double Q, Huber delta = 1) from target networks that are NOT
    the networks, against qmix_util.stepped_case's float64 reference with the same computation in float32 on the CPU as the yardstick:
    per network the gradient row, the step and the Polyak target -- each pooled over its ten tensors, the project's (2, 4), no wider
    factor -- and the statistics.  Rows near a kink carry no weight (tests/test_qmix_cpu.py holds the case to its cap).
    BSX_QMIX_RATIOS_OUT names a file the measured ratios are appended to (profiles/qmix_float64.json keeps them)."""
    c = X.stepped_case(team)
    assert c.share <= X.KINK_CAP
    kw = dict(X.STEP_KW)
    hand = X.Hand(O.ring(c.rows, X.B), O.gpu_copy(c.qnet), O.gpu_copy(c.mixer), embed=c.embed, double=True, updates=1, **kw)
    with torch.no_grad():
        for mine, src, blob in ((hand.target_qnet, c.nets[2], hand._blob_tq), (hand.target_mixer, c.nets[3], hand._blob_tm)):
            for p in D.PARAMS:
                getattr(mine, p).copy_(getattr(src, p))
            mine.pack(out=blob)
    row_q, row_m = hand.one(*O.sample_is(hand, c.idx, c.batch), 0, weight=c.w.cuda())
    torch.cuda.synchronize()
    sid, rec = X.team_id(team), {}
    print("QMIX", sid, f"left out {100 * c.share:.2f} % of the rows")
    tens = lambda g: {"g": [g[p] for p in D.PARAMS]}                                # noqa: E731
    for row, which, gkey, skey in ((row_q, "qnet", "g", "net"), (row_m, "mixer", "gm", "mix")):
        D.check_step(tens(O.grad_arrays(row, 4)), tens(c.ref[gkey]), tens(c.yard[gkey]), "row_" + which, rec, names=("g",))
        D.check_step(X.step_arrays(hand, which), c.ref[skey], c.yard[skey], which, rec)
        st = (hand.step_stats if which == "qnet" else hand.step_stats_mixer)[0].cpu().numpy()
        norm = float(row.double().square().sum().sqrt())
        coef = min(1.0, float(np.float32(kw["max_grad_norm"])) / (norm + 1e-6))
        assert st[0] == 1 and abs(st[1] - norm) <= 1e-10 * norm and abs(st[2] - coef) <= 1e-10 * coef and coef < 1.0, (which, st, norm, coef)
    bad = X.stats_out_of_bounds(hand.stats[0].cpu().numpy(), c.stats, c.e_stats, f"QMIX {sid}")
    assert not bad, bad
    assert torch.equal(hand.qnet.pack().view(torch.int32), hand._blob_q.view(torch.int32))
    assert torch.equal(hand.mixer.pack().view(torch.int32), hand._blob_m.view(torch.int32))
    O.append_ratios("BSX_QMIX_RATIOS_OUT", sid, rec)


@pytest.mark.parametrize("prio", (False, True), ids=("uniform", "prioritised-4096"))
def test_a_captured_update_runs_nothing_replays_the_eager_updates_bit_for_bit_and_allocates_nothing(prio):
    """Four replays against four eager calls: parameters, targets, moments, blobs, statistics, the draw counter and, on the prioritised
    ring of 4 096 rows, leaves, tree and max_priority, exact after every one; capture() undoes its warm-up."""
    team = X.TEAMS[1]
    rows = D.ring_rows(4096, team[0], team[1], 4, 77) if prio else None
    (captured, _), (eager, _) = (X.learner_and_hand(team, prio, rows=rows, updates=2) for _ in range(2))
    QL.captured_update(captured, eager, prio, X.NETS)


def test_set_lr_is_seen_by_a_replay_and_sync_repacks_four_blobs_after_an_outside_edit():
    (a, _), (b, _) = (X.learner_and_hand(X.TEAMS[1]) for _ in range(2))
    QL.set_lr_and_sync(a, b, X.NETS)


def test_publish_writes_only_the_q_networks_rows_of_the_rollouts_blob():
    from deep_rl_battlespace_amd import learner as L
    learner = QL.publish_rows(lambda ring, qnet: L.QMIXLearner(ring, qnet, **X.KW), X.B)    # the mixer is made: embed 8
    assert learner.mixer.n_actors == 9 and learner.mixer.obs_len == 2 * learner.Do


def test_the_constructor_refuses_what_it_cannot_learn_from():
    from deep_rl_battlespace_amd import learner as L
    from deep_rl_battlespace_amd.rollout import StackedActor
    nA, Do = 2, 8
    rows4, rows3 = D.ring_rows(128, nA, Do, 4, 1), D.ring_rows(128, nA, Do, 3, 1)
    net = lambda *s: StackedActor(*s, device="cuda")                                # noqa: E731
    with pytest.raises(ValueError, match="n_actions == 4"):
        L.QMIXLearner(O.ring(rows3, 32), net(nA, Do, 3), q_scale=2.0)
    buf = O.ring(rows4, 32)
    for bad in (net(nA, Do, 3), net(nA, Do + 1, 4), net(nA + 1, Do, 4)):
        with pytest.raises(ValueError, match="qnet must be a StackedActor"):
            L.QMIXLearner(buf, bad, q_scale=2.0)
    for bad in (net(8, 16, 4), net(9, 15, 4), net(9, 16, 3)):
        with pytest.raises(ValueError, match="mixer must be a StackedActor"):
            L.QMIXLearner(buf, net(nA, Do, 4), bad, q_scale=2.0)
    for kw, match in ((dict(embed=12, q_scale=2.0), "embed must be"), (dict(q_scale=0.0), "q_scale"), (dict(q_scale=float("nan")), "q_scale"),
                      (dict(q_scale=2.0, huber_delta=-0.1), "huber_delta")):
        with pytest.raises(ValueError, match=match):
            L.QMIXLearner(buf, net(nA, Do, 4), **kw)
    with pytest.raises(ValueError, match="1 .. 4 agents"):
        L.QMIXLearner(O.ring(D.ring_rows(128, 5, 8, 4, 1), 32), net(5, 8, 4), q_scale=2.0)
    with pytest.raises(ValueError, match="joint observation"):
        L.QMIXLearner(O.ring(D.ring_rows(128, 4, 17, 4, 1), 32), net(4, 17, 4), q_scale=2.0)
    with pytest.raises(TypeError):
        L.QMIXLearner(buf, net(nA, Do, 4))
    for embed in X.EMBEDS:
        assert isinstance(L.QMIXLearner(buf, net(nA, Do, 4), embed=embed, q_scale=2.0), L.QMIXLearner)


def test_the_learner_fits_the_pay_off_an_additive_mix_cannot_and_ends_at_its_torch_twins_table_error():
    """qmix_util's one-step game (two planes, ONE constant observation each, the team paid 1 only when both play action 0; 2 048 rows,
    B = 256, Adam 2e-3, q_scale = 2, 600 updates, embed 8).  Over the 16 joint actions no additive fit goes below a mean squared error of
    144 / 4096 (derived; tests/test_qmix_cpu.py solves it).  The learner runs 600 captured updates; its torch twin runs the SAME updates
    on the learner's own draws, on the CPU.  At the end the exact table error of the learner's Q_tot -- its own forward kernels' rows,
    mixed in float64 -- is below HALF the additive floor, each plane's own arg-max is action 0, and the table error lies within
    yardstick_util.scalar_bound of the float64 twin's: 4 x the float32 twin's own distance from it, the largest over the draws' rows in
    the given order and in 2 permuted ones.  BSX_QMIX_TASK_OUT names a file the figures are appended to (profiles/qmix_float64.json)."""
    from deep_rl_battlespace_amd import learner as L
    b, embed = X.TASK, X.TASK["embeds"][0]
    qnet, mixer = X.task_nets(embed)
    learner = L.QMIXLearner(O.ring(X.task_rows(), b["B"]), O.gpu_copy(qnet), O.gpu_copy(mixer), embed=embed, q_scale=b["q_scale"],
                            huber_delta=b["huber_delta"], gamma=X.GAMMA, tau=b["tau"], lr=b["lr"]).capture()
    draws, losses = [], []
    for _ in range(b["N"]):
        stats = learner.update()
        draws.append(learner.buffer.last_idx.clone())
        losses.append(stats[0, 1].clone())
    torch.cuda.synchronize()
    draws, losses = [d.cpu() for d in draws], [float(x) for x in losses]
    obs = X.task_obs().cuda()[None].contiguous()
    y4 = O.Hand.forward(None, learner._blob_q, obs)[0].cpu().numpy()
    hy = O.Hand.forward(None, learner._blob_m, X.joint(obs, learner.members))[0].cpu().numpy()
    table = X.table_of(y4, hy, embed, b["q_scale"])
    err = X.table_error(table)
    assert X.argmax4(y4).tolist() == [0, 0] and np.unravel_index(table.argmax(), (4, 4)) == (0, 0)
    q64, m64, ref_losses = X.task_twin(embed, draws, torch.float64)
    ref = X.table_error(X.net_table(q64, m64, embed))
    own, twin_err = 0.0, None
    for order in Y.row_orders(b["B"], 2):
        q32, m32, _ = X.task_twin(embed, [d if order is None else d[order] for d in draws], torch.float32)
        e32 = X.table_error(X.net_table(q32, m32, embed))
        twin_err = e32 if twin_err is None else twin_err
        own = max(own, abs(e32 - ref))
    tol = Y.scalar_bound(ref, own)
    print(f"QMIX task embed {embed}, N = {b['N']}: batch loss {losses[0]:.4f} -> {losses[-1]:.4f}; table error {err:.6e} (additive floor "
          f"{X.VDN_FLOOR:.4f}); float64 twin {ref:.6e}, float32 twin {twin_err:.6e}; |difference| {abs(err - ref):.3e}, the float32 twin's own "
          f"(3 row orders) {own:.3e}, bound {tol:.3e}")
    path = os.environ.get("BSX_QMIX_TASK_OUT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": f"embed{embed}", "figures": dict(first_loss=losses[0], last_loss=losses[-1], table_error=err,
                                                                           float64_twin_table_error=ref, float32_twin_table_error=twin_err,
                                                                           float32_twin_own_distance=own, bound=tol)}) + "\n")
    assert abs(losses[0] - ref_losses[0]) <= 1e-5 * ref_losses[0]
    assert err < 0.5 * X.VDN_FLOOR
    assert abs(err - ref) <= tol
