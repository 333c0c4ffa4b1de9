"""DDPGLearner on the MI355X: an update is, bit for bit, the sequence of the public primitives written out by hand
(tests/ddpg_util.py: Hand); a captured update replays as one graph with fresh draws and allocates nothing; the first update's two
gradient rows against float64 CPU autograd of the two MADDPG losses with torch float32 autograd as the yardstick; a whole update from
target networks that are not the networks -- both gradient rows, both steps, both Polyak targets, the statistics -- against float64, and
a learner from such targets against the by-hand update; finished rows keep the targets out; set_lr reaches a captured graph; publish
writes the team's rows alone; and a bandit on which the captured updates must learn at least half of what the torch composition learns."""
import types

import numpy as np
import pytest
import torch

import adam_util as AU
import ddpg_util as D
import mlp_grad_util as M
import offpolicy_util as O

pytestmark = pytest.mark.gpu

def _pair(shape, **kw):
    """(a DDPGLearner, a Hand) from equal copies of the shape's starting state (learner_case at `seed`), each on a ring of its own with
    the same rows and seed."""
    return D.SUITE.learner(shape, **kw), D.SUITE.hand(shape, **kw)


@pytest.mark.parametrize("shape", D.LEARNER_SHAPES, ids=D.shape_id)
def test_an_update_is_the_by_hand_sequence_of_the_public_primitives_bit_for_bit(shape):
    learner, hand = _pair(shape)
    start = D.snapshot(learner)
    assert O.differing(start, D.snapshot(hand)) == []
    for u in range(3):
        stats = learner.update()
        hand.update()
        a, b = D.snapshot(learner), D.snapshot(hand)
        assert O.differing(a, b) == [], (u, O.differing(a, b))
        assert stats is learner.stats and float(stats[0, 0]) == shape[0] * shape[1]
    assert int(learner.step_actor) == 3 == int(learner.step_critic) and int(learner.buffer._draws) == 3
    assert torch.equal(learner.buffer.last_idx, hand.buffer.last_idx)
    moved = set(O.differing(start, a))
    assert {"actor.w1", "critic.w1", "target_actor.w2", "target_critic.w2", "_blob_a", "_blob_c", "_blob_ta", "_blob_tc", "adam_actor.m",
            "adam_critic.v", "stats", "step_stats_actor", "step_stats_critic", "draws"} <= moved
    O.blobs_are_packs(learner)
    if shape[3] == 3:                                                         # three actions: the head's fourth column carries nothing
        pad = torch.from_numpy(AU.pad_mask(shape[2], 3)).cuda()
        assert pad.sum() == 65 and not learner._g_a4.view(torch.int32)[..., 3].any()
        assert not learner._buf_a["grad"].view(torch.int32)[:, pad].any() and learner._buf_a["grad"][:, ~pad].abs().max() > 0


@pytest.mark.parametrize("shape", D.LEARNER_SHAPES, ids=D.shape_id)
def test_a_captured_update_runs_nothing_replays_the_eager_updates_with_fresh_draws_and_allocates_nothing(shape):
    captured, eager = (D.SUITE.learner(shape, updates=2) for _ in range(2))
    O.capture_runs_nothing(captured, D.snapshot)
    draws = []
    O.replays_the_eager_updates(captured, eager, D.snapshot, 3, lambda u: draws.append(captured.buffer.last_idx.clone()))
    # fresh draws (a batch of one row draws one of four indices: there the draw counter below and the eager twin say it)
    assert shape[0] == 1 or (not torch.equal(draws[0], draws[1]) and not torch.equal(draws[1], draws[2]))
    assert int(captured.step_actor) == 6 == int(captured.step_critic) and int(captured.buffer._draws) == 6
    O.blobs_are_packs(captured)
    O.allocates_nothing(captured)


@pytest.mark.parametrize("shape", D.LEARNER_SHAPES, ids=D.shape_id)
def test_the_first_updates_gradient_rows_against_float64_autograd_of_the_two_maddpg_losses(shape):
    """The ring sampled with fixed idx, the kink-free weights passed as `weight` through the primitives; no optimiser step, so both rows
    are gradients at the starting parameters.  torch float32 autograd on the CPU is the yardstick (mlp_grad_util.check)."""
    B, nA, Do, k, central = shape
    actor, critic, rows, idx, w, share = D.learner_case(shape)
    assert share < D.U.KINK_CAP
    hand = D.SUITE.hand(shape)
    batch = tuple(r[idx] for r in rows)
    row_c, row_a = hand.step(*O.sample_is(hand, idx, batch), 0, weight=w.cuda(), adam=False)
    torch.cuda.synchronize()
    gc64, ga64 = D.maddpg_grads(actor, critic, batch, w, central, torch.float64)
    gc32, ga32 = D.maddpg_grads(actor, critic, batch, w, central, torch.float32)
    M.check(O.grad_arrays(row_c, 1), gc64, gc32, f"DDPG critic {D.shape_id(shape)}", names=D.PARAMS)
    M.check(O.grad_arrays(row_a, k), ga64, ga32, f"DDPG actor {D.shape_id(shape)}", names=D.PARAMS)
    assert all(float(np.abs(g).max()) > 0 for g in list(gc64.values()) + list(ga64.values()))


def _set_targets(x, case, sync=False):
    O.set_targets(x, dict(actor=case.ta, critic=case.tc), sync)


@pytest.mark.parametrize("shape", D.LEARNER_SHAPES, ids=D.shape_id)
def test_an_update_with_distinct_targets_and_a_stepped_critic_against_float64(shape):
    """One whole update through the primitives (Hand.step with both optimiser steps) from target networks that are NOT the networks,
    against ddpg_util.stepped_case's float64 reference with the same computation in float32 on the CPU as the yardstick: the critic's
    gradient row reads y from the target critic on the target actors' actions, the actor's row is taken at the STEPPED critic
    (tests/test_ddpg_cpu.py: each misreading lies 2e5 yardstick errors away), networks, moments and Polyak targets hold the bars of
    adam_case_util.meets_the_bars, the statistics check_td's, and the four blobs are the packs of what they stand for.
    BSX_DDPG_RATIOS_OUT names a file the measured ratios are appended to (profiles/ddpg_float64.json records them)."""
    B, nA, Do, k, central = shape
    c = D.stepped_case(shape)
    assert c.share < D.U.KINK_CAP
    hand = D.SUITE.hand(shape, seed=c.seed, **D.STEP_KW)
    _set_targets(hand, c)
    O.blobs_are_packs(hand)
    row_c, row_a = hand.step(*O.sample_is(hand, c.idx, c.batch), 0, weight=c.w.cuda(), adam=True)
    torch.cuda.synchronize()
    sid, rec = D.shape_id(shape), {}
    for which, row, na in (("gc", row_c, 1), ("ga", row_a, k)):
        r = D.U.check(O.grad_arrays(row, na), c.ref[which], c.yard[which], f"DDPG {which} {sid}", D.PARAMS, D.stepped_factor_of(shape, which))
        rec.update({f"{which}.{p}": [round(v[0], 4), round(v[1], 4)] for p, v in r.items()})
    for which in ("critic", "actor"):
        D.check_step(O.step_arrays(hand, which), c.ref[which], c.yard[which], which, rec)
    assert int(hand.step_critic) == 1 == int(hand.step_actor)
    for which, stats, row in (("critic", hand.step_stats_critic, row_c), ("actor", hand.step_stats_actor, row_a)):
        # (adam_case_util.check_stats' bound: the norm of the row the step read -- checked against float64 above -- and the clip
        # coefficient from it, both float64 on the device)
        got, norm = stats[0].cpu().numpy(), float(row.double().square().sum().sqrt())
        coef = min(1.0, float(np.float32(D.STEP_KW["max_grad_norm"])) / (norm + 1e-6))
        assert got[0] == 1 and abs(got[1] - norm) <= 1e-10 * norm and abs(got[2] - coef) <= 1e-10 * coef, (which, got, norm, coef)
        assert coef < 1.0                                         # both steps are clipped at every shape: the coefficient is in the check
    bad = D.HEAD.stats_out_of_bounds(hand.stats[0].cpu().numpy(), c.stats, c.e_stats, f"DDPG {sid}")
    assert not bad, bad
    O.blobs_are_packs(hand)
    O.append_ratios("BSX_DDPG_RATIOS_OUT", sid, rec)


def test_a_learners_updates_from_distinct_targets_are_the_by_hand_updates_bit_for_bit():
    """The same starting state on a DDPGLearner (its targets edited from outside, then sync()) and a Hand: three updates leave the same
    bits, which carries the float64 checks of the Hand over to the learner where the targets differ from the networks."""
    shape = D.LEARNER_SHAPES[1]
    c = D.stepped_case(shape)
    learner, hand = _pair(shape, seed=c.seed, **D.STEP_KW)
    _set_targets(learner, c, sync=True)
    _set_targets(hand, c)
    O.blobs_are_packs(learner)
    start = D.snapshot(learner)
    assert O.differing(start, D.snapshot(hand)) == []
    assert not torch.equal(start["target_critic.w1"], start["critic.w1"]) and not torch.equal(start["_blob_ta"], start["_blob_a"])
    for u in range(3):
        learner.update()
        hand.update()
        a, b = D.snapshot(learner), D.snapshot(hand)
        assert O.differing(a, b) == [], (u, O.differing(a, b))
    assert int(learner.step_critic) == 3 and {"critic.w1", "target_critic.w1", "target_actor.w1"} <= set(O.differing(start, a))
    O.blobs_are_packs(learner)


def test_finished_rows_keep_the_target_networks_out_of_every_gradient():
    """done = 1 on every row: y = rew.  Two learners whose target networks differ (NaN-free) leave the same bits in the actor, the
    critic, their moments, their blobs and the statistics."""
    shape = D.LEARNER_SHAPES[1]
    _, _, rows, *_ = D.learner_case(shape)
    rows = (*rows[:4], torch.ones_like(rows[4]))
    a = D.SUITE.learner(shape, rows=rows)
    b = D.SUITE.learner(shape, rows=rows)
    with torch.no_grad():
        for t in (b.target_actor, b.target_critic):
            for p in t.parameters():
                p.add_(0.25 * torch.randn(p.shape, generator=torch.Generator().manual_seed(5)).to(p.device))
    b.sync()
    O.blobs_are_packs(b)
    for _ in range(2):
        a.update()
        b.update()
    x, y = D.snapshot(a), D.snapshot(b)
    diff = O.differing(x, y)
    assert diff and all(k.startswith("target_") or k in ("_blob_ta", "_blob_tc") for k in diff), diff
    assert float(a.stats[0, 5]) == 1.0 and torch.equal(a.td.view(torch.int32), a.buffer._b_rew.view(torch.int32))


def test_set_lr_reaches_a_captured_update():
    shape = D.LEARNER_SHAPES[0]
    learner = D.SUITE.learner(shape)
    learner.capture()
    learner.set_lr(actor=0.0, critic=0.0)
    before = D.snapshot(learner)
    learner.update()
    after = D.snapshot(learner)
    same = [k for k in before if k.startswith(("actor.", "critic."))]
    assert all(torch.equal(before[k], after[k]) for k in same) and int(learner.step_actor) == 1
    assert float(learner.step_stats_actor[0, 3]) == 0.0 == float(learner.step_stats_critic[0, 3])
    learner.set_lr(actor=2e-3)
    learner.update()
    assert float(learner.step_stats_actor[0, 3]) == float(np.float32(2e-3)) and float(learner.step_stats_critic[0, 3]) == 0.0
    moved = O.differing(after, D.snapshot(learner))
    assert "actor.w1" in moved and not [k for k in moved if k.startswith("critic.")]
    with pytest.raises(ValueError):
        learner.set_lr(actor=-1.0)


@pytest.mark.parametrize("c0", [0, 2])
def test_publish_writes_the_teams_blob_rows_and_parameter_slices_and_nothing_else(c0):
    from deep_rl_battlespace_amd.rollout import FusedActor, StackedActor
    shape = D.LEARNER_SHAPES[1]                                               # 2v2: the rollout's actor has 4 agents of obs_len 8
    learner = D.SUITE.learner(shape)
    learner.update()
    torch.manual_seed(3)
    ro_actor = StackedActor(4, 8, 4, device="cuda")
    ro = types.SimpleNamespace(actor=ro_actor, fused=FusedActor(ro_actor, 2))
    blob0 = ro.fused.weights.clone()
    params0 = {p: getattr(ro_actor, p).detach().clone() for p in D.PARAMS}
    learner.publish(ro, range(c0, c0 + 2))
    torch.cuda.synchronize()
    team, rest = slice(c0, c0 + 2), slice(2 - c0, 4 - c0)
    bits = lambda t: t.detach().view(torch.int32)                             # noqa: E731
    assert torch.equal(bits(ro.fused.weights[team]), bits(learner._blob_a)) and torch.equal(bits(ro.fused.weights[rest]), bits(blob0[rest]))
    assert not torch.equal(bits(ro.fused.weights[team]), bits(blob0[team]))
    for p in D.PARAMS:
        assert torch.equal(bits(getattr(ro_actor, p)[team]), bits(getattr(learner.actor, p))), p
        assert torch.equal(bits(getattr(ro_actor, p)[rest]), bits(params0[p][rest])), p
    assert torch.equal(bits(ro_actor.pack()), bits(ro.fused.weights))         # the rows published are the pack of the slices published
    for cols in ([0, 2], range(3, 5), range(0, 3)):
        with pytest.raises(ValueError, match="contiguous range"):
            learner.publish(ro, cols)
    with pytest.raises(ValueError, match="obs_len 8"):
        learner.publish(types.SimpleNamespace(actor=StackedActor(4, 5, 4, device="cuda"), fused=None), range(0, 2))


def test_the_constructor_names_the_shape_it_wanted():
    from deep_rl_battlespace_amd.learner import DDPGLearner
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, ReplayBuffer
    from deep_rl_battlespace_amd.rollout import StackedActor
    buf = DeviceReplayBuffer(64, 16, list(range(2)), 8, 16, 4, device="cuda")
    actor = StackedActor(2, 8, 4, device="cuda")
    learner = DDPGLearner(buf, actor)
    assert (learner.critic.n_actors, learner.critic.obs_len, learner.critic.n_actions) == (2, 24, 1) and learner.stats.shape == (1, 8)
    assert DDPGLearner(buf, actor, critic_input="own", updates=3).step_stats_critic.shape == (3, 4)
    with pytest.raises(ValueError, match=r"StackedActor\(2, 8, 4\)"):
        DDPGLearner(buf, StackedActor(2, 5, 4, device="cuda"))
    with pytest.raises(ValueError, match=r"StackedActor\(2, 24, 1\)"):
        DDPGLearner(buf, actor, StackedActor(2, 12, 1, device="cuda"))
    with pytest.raises(ValueError, match=r"StackedActor\(2, 12, 1\)"):
        DDPGLearner(buf, actor, StackedActor(2, 24, 1, device="cuda"), critic_input="own")
    with pytest.raises(ValueError, match="DeviceReplayBuffer"):
        DDPGLearner(ReplayBuffer(64, 16, list(range(2)), 8, 16, 4, device="cuda"), actor)
    with pytest.raises(ValueError, match="critic_input"):
        DDPGLearner(buf, actor, critic_input="joint")
    for kw in (dict(gamma=1.5), dict(tau=-0.1), dict(lr_actor=-1.0), dict(max_grad_norm=0.0), dict(updates=0)):
        with pytest.raises(ValueError):
            DDPGLearner(buf, actor, **kw)
    wide = DeviceReplayBuffer(64, 16, list(range(4)), 14, 56, 4, device="cuda")
    with pytest.raises(ValueError, match="4v4 central is 72"):
        DDPGLearner(wide, StackedActor(4, 14, 4, device="cuda"))
    assert DDPGLearner(wide, StackedActor(4, 14, 4, device="cuda"), critic_input="own").Dc == 18


def test_captured_updates_on_a_bandit_learn_at_least_half_of_what_the_torch_composition_learns():
    """A bandit ring: every row finished, r = -mean_k (a_k - 0.5 sign(o_k))^2, own critics.  N and the torch composition's figures are
    recorded in profiles/ddpg_float64.json, chosen on the CPU with the torch composition alone, which itself closes at least half of the
    gap from its initial reward to 0 in N updates (re-run here: a fraction of a second)."""
    from deep_rl_battlespace_amd.learner import DDPGLearner
    b = O.BANDIT
    make = lambda ring, actor, critic: DDPGLearner(ring, actor, critic, critic_input="own", tau=b["tau"], lr_actor=b["lr"], lr_critic=b["lr"],     # noqa: E731
                                                   updates=10)
    learner, N, _ = O.bandit_test(D.PROFILE, D.bandit_torch_run, make, O.bandit_nets(), "torch composition")
    assert int(learner.step_actor) == N
