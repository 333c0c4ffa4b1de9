"""learner.PPOLearner on a PolicyRollout(central_critic=) -- MAPPO's update -- on the MI355X: a minibatch is the six calls made by hand,
bit for bit; its gradient rows and the first optimiser step meet the float64 yardstick's bars (tests/mappo_util.py builds the
restatement on ppo_head_util's and adam_util's references; the bars are actor_grad_util.check's and adam_util.check_step's); the
captured update is the eager one and allocates nothing; actor and critic are clipped by their own norms; a tied team's first step
meets the same bars against the float64 sum of its members' rows (groups of 2, 3 and 4) and shared teams stay identical; a scripted
team keeps every bit (categorical 2v2 blue, gaussian 3v3 red); shuffled minibatches; the next run's values come from the stepped
critic, behind the per-tick graph and behind the one-launch rollout.  T = 8; 1v1, 2v2, 3v3, 4v4 (the critic's widest input: 56
floats on 8 planes); 96 and 33 games; both kinds."""
import numpy as np
import pytest
import torch

import actor_grad_util as G
import mappo_util as M
import ppo_learner_util as L
import yardstick_util as Y
from ppo_learner_util import HEAD_KW, KW, STEPS

pytestmark = pytest.mark.gpu

# (kind, n, E): every team size, both game counts and both kinds
SHAPES = (("gaussian", 1, 96), ("categorical", 1, 33), ("categorical", 2, 96), ("gaussian", 2, 33), ("gaussian", 3, 96), ("categorical", 3, 33),
          ("categorical", 4, 96), ("gaussian", 4, 33))
IDS = ["%s-n%d-E%d" % s for s in SHAPES]


def _bits(x):
    return x.detach().contiguous().view(torch.int32 if x.element_size() == 4 else torch.int64).cpu()


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("kind,n,E", SHAPES, ids=IDS)
def test_a_minibatch_is_the_six_calls_made_by_hand_bit_for_bit(kind, n, E):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = M.central_rollout(kind, n=n, E=E)
    learner = PPOLearner(ro, **KW)
    assert learner.critic is ro.central_critic and learner.critic_input == "central" and learner.central
    assert learner.critic.obs_len == n * (3 * n + 2)
    for t0, t1 in ((0, ro.T), (4, 8), (3, 4)):
        got = [x.clone() if x is not None else None for x in learner.minibatch_grads(t0, t1)]
        want = M.six_calls(ro, kind, M.minibatch_of(ro, t0, t1, clone=True), ro.actor.pack(), ro.central_critic.pack(), HEAD_KW)
        torch.cuda.synchronize()
        assert _same(got, want), (t0, t1)
        assert float(got[3][0]) == float(ro.mask[t0:t1].sum()) and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        assert float(got[1].abs().max()) > 0 and tuple(got[1].shape) == (2 * n, 64 * learner.critic.obs_len + 64 * 64 + 6 * 64 + 260)
    own = PPOLearner(M.central_rollout(kind, n=n, E=E, critic="own"), **KW)
    assert own.critic_input == "own" and not own.central


# ---------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("kind,n,E", SHAPES, ids=IDS)
def test_the_gradient_rows_of_a_minibatch_meet_the_bars_against_the_float64_restatement(kind, n, E):
    """Both networks a nudge away from the ones that played, so that ratios leave 1 and values leave the recorded ones; rows near a kink
    of the loss or of a ReLU (in float64) are taken out of the mask for every path alike."""
    from deep_rl_battlespace_amd.learner import PPOLearner, split_grad
    ro = M.central_rollout(kind, n=n, E=E)
    G.nudge(ro.actor, 0.12)
    G.nudge(ro.central_critic, 0.03, seed=6)
    mask, dropped = M.kept_rows(ro, kind)
    kept = int((mask != 0).sum())
    print(f"{kind} n={n} E={E}: rows kept {kept}, dropped near a kink {dropped:.4f}")
    assert kept >= 100 and dropped <= 0.2
    ro._mask.copy_(mask.view(ro._mask.shape).cuda())
    ref, yard = M.minibatch_float(ro, kind, torch.float64, mask), M.minibatch_float(ro, kind, torch.float32, mask)
    learner = PPOLearner(ro, **dict(KW, epochs=1, minibatches=1))
    row_a, row_v, g_ls, stats = learner.minibatch_grads(0, ro.T)
    torch.cuda.synchronize()
    assert float(stats[0]) == kept == ref["stats"][0]
    got_a = {k: g.double().cpu().numpy() for k, g in zip(L.PARAMS, split_grad(row_a, ro.actor.n_actions))}
    got_v = {k: g.double().cpu().numpy() for k, g in zip(L.PARAMS, split_grad(row_v, 1))}
    G.check(got_a, ref["actor"], yard["actor"], f"MAPPO {kind} n={n} E={E} actor")
    G.check(got_v, ref["critic"], yard["critic"], f"MAPPO {kind} n={n} E={E} critic")
    if kind == "gaussian":
        e_ls = float(np.abs(yard["g_log_std"] - ref["g_log_std"]).max())
        err = float(np.abs(g_ls.double().cpu().numpy() - ref["g_log_std"]).max())
        print(f"log_std gradient: |learner - f64| {err:.3e}, torch's own error {e_ls:.3e}, bound {Y.scalar_bound(ref['g_log_std'], e_ls):.3e}")
        assert err <= Y.scalar_bound(ref["g_log_std"], e_ls)


@pytest.mark.parametrize("kind,n,E", (SHAPES[0], SHAPES[2], SHAPES[5], SHAPES[7]), ids=(IDS[0], IDS[2], IDS[5], IDS[7]))
def test_the_first_step_meets_the_bars_and_each_network_is_clipped_by_its_own_norm(kind, n, E):
    ro = M.central_rollout(kind, n=n, E=E)
    # a max_grad_norm small enough that both networks clip: each coefficient follows from its own norm
    (norm_a, coef_a), (norm_v, coef_v) = M.first_step_meets_the_bars(ro, dict(max_grad_norm=0.01)).values()
    assert coef_a < 1.0 and coef_v < 1.0 and norm_a != norm_v and abs(coef_a * (norm_a + 1e-6) - coef_v * (norm_v + 1e-6)) < 1e-9


# (kind, n, E, max_grad_norm): groups of 2, 3 (odd) and 4 with both networks clipping; a group of 4 with log_std tied too, at the suite's 0.5
TIED = (("categorical", 2, 96, 0.01), ("gaussian", 3, 33, 0.01), ("categorical", 4, 96, 0.01), ("gaussian", 4, 33, 0.5))


@pytest.mark.parametrize("kind,n,E,max_grad_norm", TIED, ids=["%s-g%d-E%d-clip%g" % c for c in TIED])
def test_a_tied_teams_first_step_meets_the_bars_against_the_float64_sum_of_its_members_rows(kind, n, E, max_grad_norm):
    """share="team" on a central critic, device and torch paths: the reference steps every group with the float64 sum of its members'
    gradient rows and counts it once in the norm, so a step that dropped a member's row or summed the wrong planes moves the leaders
    off it by a whole row, not by rounding.  The device adds a group's rows in float32 (as the torch path's install does), so the
    recorded norm is held to the float64 one to 1e-6, the shared PPO test's allowance: g - 1 roundings of 2^-24 per element at most."""
    ro = M.central_rollout(kind, n=n, E=E, group=n)
    figures = M.first_step_meets_the_bars(ro, dict(share="team", max_grad_norm=max_grad_norm), g=n, norm_rtol=1e-6)
    (norm_a, coef_a), (norm_v, coef_v) = figures.values()
    assert norm_a > 0 and norm_v > 0 and norm_a != norm_v
    if max_grad_norm == 0.01:                        # both networks clip: each coefficient follows from its own norm
        assert coef_a < 1.0 and coef_v < 1.0 and abs(coef_a * (norm_a + 1e-6) - coef_v * (norm_v + 1e-6)) < 1e-9


# ---------------------------------------------------------------------------------------------------- the device update
@pytest.mark.parametrize("kind,n,E", (SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[5], SHAPES[6]), ids=(IDS[0], IDS[2], IDS[3], IDS[5], IDS[6]))
def test_the_device_update_is_the_sequence_by_hand_captured_is_eager_and_nothing_is_allocated(kind, n, E):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = M.central_rollout(kind, n=n, E=E)
    rv = M.view(ro)
    make = lambda: PPOLearner(ro, device_step=True, **KW)     # noqa: E731
    start = L.keep(rv)
    assert L.blobs_are_packs(rv)
    # the update against adam_step of the actor and mlp_adam_step of the critic, by hand, on minibatch_grads' rows
    learner = make()
    stats = learner.update()
    got = M.everything(learner)
    assert stats.shape == (STEPS, 8) and bool(torch.isfinite(stats).all()) and bool((stats[:, 0] > 30).all())
    for count, st in ((learner.step_count, learner.step_stats), (learner.critic_step_count, learner.critic_step_stats)):
        assert int(count) == STEPS and st[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and bool((st[:, 1] > 0).all()) and bool((st[:, 2] <= 1).all())
        assert bool((st[:, 3] == float(np.float32(KW["lr"]))).all())
    assert not torch.equal(learner.step_stats[:, 1], learner.critic_step_stats[:, 1])          # two norms
    assert all(p.grad is None for p in learner.params) and L.blobs_are_packs(rv) and not torch.equal(got[0], start[0])
    L.restore(rv, start)
    assert L.equal(got, M.by_hand(ro, kind, L.tick_ranges_of(make())))
    # eager and captured twins over two updates, from the same state and the same records; capture() itself moves nothing
    L.restore(rv, start)
    eager, graph = make(), make()
    before = M.everything(graph)
    assert graph.capture() is graph
    assert L.equal(M.everything(graph), before) and int(graph.step_count) == 0 and int(graph.critic_step_count) == 0
    for update in range(2):
        eager.update()
        a = M.everything(eager)
        L.restore(rv, start)
        graph.update()
        b = M.everything(graph)
        assert L.equal(a, b), update
        assert not torch.equal(b[0], start[0]) and L.blobs_are_packs(rv)
        # the next run's values come from the stepped critic, with no refresh call
        ro.run()
        torch.cuda.synchronize()
        assert torch.equal(_bits(ro._values), _bits(M.central_values(ro, ro.central_critic.pack()))), update
        start = L.keep(rv)
    assert int(graph.step_count) == 2 * STEPS and int(graph.critic_step_count) == 2 * STEPS
    L.allocates_nothing(M.learner_view(graph), warm=False)
    # set_lr moves both networks' rate: one hyper tensor
    graph.set_lr(2e-3)
    graph.update()
    torch.cuda.synchronize()
    assert bool((graph.step_stats[:, 3] == float(np.float32(2e-3))).all()) and bool((graph.critic_step_stats[:, 3] == float(np.float32(2e-3))).all())
    with pytest.raises(ValueError, match="lr_critic"):
        graph.set_lr(1e-3, critic=1e-3)


def test_lr_critic_gives_the_critic_a_rate_of_its_own_on_both_paths():
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = M.central_rollout("categorical", n=2, E=33)
    learner = PPOLearner(ro, device_step=True, lr_critic=5e-3, **KW)
    assert learner.hyper_critic is not learner.hyper
    learner.update()
    learner.set_lr(2e-4, critic=7e-3)
    first = learner.critic_step_stats[:, 3].clone()
    learner.update()
    torch.cuda.synchronize()
    assert bool((first == float(np.float32(5e-3))).all()) and bool((learner.critic_step_stats[:, 3] == float(np.float32(7e-3))).all())
    assert bool((learner.step_stats[:, 3] == float(np.float32(2e-4))).all())
    torch_path = PPOLearner(ro, lr_critic=5e-3, **KW)
    assert [g["lr"] for g in torch_path.optimizer.param_groups] == [KW["lr"], 5e-3]
    assert len(torch_path.optimizer.param_groups[1]["params"]) == 10
    torch_path.update()
    own = M.central_rollout("categorical", n=1, E=33, critic="own")
    with pytest.raises(ValueError, match="lr_critic"):
        PPOLearner(own, lr_critic=1e-3)


# ---------------------------------------------------------------------------------------------------- sharing, scripted opponent
@pytest.mark.parametrize("device_step", [True, False])
@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_a_shared_team_stays_identical_over_two_updates_on_both_paths(kind, device_step, n=2):
    from deep_rl_battlespace_amd.learner import PPOLearner, tie_
    ro = M.central_rollout(kind, n=n, E=96, group=n)
    learner = PPOLearner(ro, share="team", device_step=device_step, **KW)
    assert learner.group == n
    start = L.keep(M.view(ro))
    for _ in range(2):
        learner.update()
        ro.run()
    torch.cuda.synchronize()
    rv = M.view(ro)
    for i, t in enumerate(L.shared(rv) + (L.moments(learner) if device_step else [])):        # parameters, log_std, both blobs[, the moments]
        v = t.detach().contiguous().view(torch.int32).view(t.shape[0] // n, n, -1)
        assert torch.equal(v, v[:, :1].expand_as(v)), i
    assert L.blobs_are_packs(rv) and not torch.equal(L.keep(rv)[0], start[0]) and not torch.equal(L.keep(rv)[10], start[10])
    # an untied central critic is refused by name
    with torch.no_grad():
        ro.central_critic.b3[1].add_(1.0)
    with pytest.raises(ValueError, match="central_critic differs"):
        PPOLearner(ro, share="team", device_step=device_step, **KW)
    tie_(ro.central_critic, n)


@pytest.mark.parametrize("device_step", [True, False])
@pytest.mark.parametrize("kind,n", [("categorical", 3), ("gaussian", 4)], ids=["categorical-n3", "gaussian-n4"])
def test_a_shared_team_of_three_and_of_four_stays_identical_over_two_updates_on_both_paths(kind, n, device_step):
    """The cheap check at the wider groups (an odd one, and the largest a tied step sums); that the members are RIGHT is the tied first
    step's test above."""
    test_a_shared_team_stays_identical_over_two_updates_on_both_paths(kind, device_step, n)


@pytest.mark.parametrize("device_step", [True, False])
def test_a_scripted_team_keeps_every_bit_and_the_learned_team_moves(device_step, kind="categorical", n=2, opponent="blue"):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = M.central_rollout(kind, n=n, E=96, opponent=opponent)
    scripted, learned = L.scripted_columns(n, opponent)
    learner = PPOLearner(ro, device_step=device_step, **KW)
    if device_step:
        lv = M.learner_view(learner)
        before = L.everything(lv)
        learner.update()
        after = L.everything(lv)
        assert int(learner.step_count) == STEPS and int(learner.critic_step_count) == STEPS
        L.scripted_keep_every_bit_and_learned_move(lv, before, after, scripted, learned)
    else:
        before = L.keep(M.view(ro))
        learner.update()
        after = L.keep(M.view(ro))
        for b, a in zip(before, after):
            assert torch.equal(L.bits(b, scripted), L.bits(a, scripted)) and not torch.equal(L.bits(b, learned), L.bits(a, learned))
    assert L.blobs_are_packs(M.view(ro))


@pytest.mark.parametrize("device_step", [True, False])
def test_a_scripted_red_team_keeps_every_bit_at_3v3_under_the_gaussian_head(device_step):
    """The other team, the other head (log_std rows and their moments have an agent axis too) and an odd team: blue learns."""
    test_a_scripted_team_keeps_every_bit_and_the_learned_team_moves(device_step, "gaussian", 3, "red")


# ---------------------------------------------------------------------------------------------------- behind the one-launch rollout
@pytest.mark.parametrize("kind,n,E", (SHAPES[2], SHAPES[7]), ids=(IDS[2], IDS[7]))
def test_behind_a_one_launch_rollout_a_minibatch_is_the_six_calls_and_the_next_runs_values_come_from_the_stepped_critic(kind, n, E):
    """The form a central critic opens beyond 1v1: the ticks are one kernel, the critic's pass follows it inside the same captured run."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = M.central_rollout(kind, n=n, E=E, one_launch=True)
    rv = M.view(ro)
    assert ro.one_launch and ro.graph is not None and ro._value_w is None
    learner = PPOLearner(ro, device_step=True, **KW)
    got = [x.clone() if x is not None else None for x in learner.minibatch_grads(0, ro.T)]
    want = M.six_calls(ro, kind, M.minibatch_of(ro, clone=True), ro.actor.pack(), ro.central_critic.pack(), HEAD_KW)
    torch.cuda.synchronize()
    assert _same(got, want) and float(got[3][0]) == float(ro.mask.sum()) > 0 and float(got[1].abs().max()) > 0
    assert learner.capture() is learner
    for update in range(2):
        before = L.keep(rv)
        learner.update()
        ro.run()
        torch.cuda.synchronize()
        assert not torch.equal(L.keep(rv)[10], before[10]), update                    # the critic moved
        assert torch.equal(_bits(ro._values), _bits(M.central_values(ro, ro.central_critic.pack()))), update
        assert L.blobs_are_packs(rv), update
    assert int(learner.step_count) == 2 * STEPS and int(learner.critic_step_count) == 2 * STEPS


# ---------------------------------------------------------------------------------------------------- shuffle
@pytest.mark.parametrize("kind,n,E", (SHAPES[1], SHAPES[4], SHAPES[7]), ids=(IDS[1], IDS[4], IDS[7]))
def test_shuffled_minibatches_with_vclip_are_the_six_calls_on_the_gathered_rows(kind, n, E):
    from deep_rl_battlespace_amd.learner import Minibatch, PPOLearner
    ro = M.central_rollout(kind, n=n, E=E)
    assert KW["vclip"] is not None
    learner = PPOLearner(ro, shuffle=True, shuffle_seed=9, device_step=True, **KW)
    T = ro.T
    for i in (0, 3):
        got = [x.clone() if x is not None else None for x in learner.shuffled_grads(i)]
        idx = learner.minibatch_idx[i]
        assert idx.numel() == T * E // KW["minibatches"] and len(set(idx.tolist())) == idx.numel()
        pick = lambda x: x[:T].reshape(T * E, *x.shape[2:])[idx].contiguous()      # noqa: E731
        mb = Minibatch(pick(ro.obs), pick(ro.scores), pick(ro.logp), pick(ro.adv), pick(ro.ret), pick(ro._mask), pick(ro.value))
        want = M.six_calls(ro, kind, mb, ro.actor.pack(), ro.central_critic.pack(), HEAD_KW)
        torch.cuda.synchronize()
        assert _same(got, want), i
    start = L.keep(M.view(ro))
    stats = learner.update()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(stats).all()) and int(learner.shuffle_base) == KW["epochs"] and int(learner.critic_step_count) == STEPS
    assert not torch.equal(L.keep(M.view(ro))[10], start[10]) and L.blobs_are_packs(M.view(ro))
