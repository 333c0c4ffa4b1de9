"""SACLearner on the MI355X: an update is, bit for bit, the sequence of the public primitives written out by hand (tests/sac_util.py:
Hand), on a plain and on a prioritised ring, own-critic teams of 2, 4 and 16 agents included; a captured update runs nothing, replays the eager updates with fresh draws and fresh noise
and allocates nothing; with lr_alpha=None the temperature never moves; a whole update from target critics that are not the critics
against float64; with own critics one agent's temperature and spread reach that agent's target and gradients and no other's; one iteration of the documented loop on a real continuous 1v1 env with a Gaussian rollout; and a bandit on which the
captured updates must learn at least half of what the torch composition of the same SAC learns."""
import math

import numpy as np
import pytest
import torch

import ddpg_util as D
import offpolicy_util as O
import sac_util as S

pytestmark = pytest.mark.gpu

KW = D.KW


_learner, _hand = S.SUITE.learner, S.SUITE.hand
NO_CLIP = dict(D.STEP_KW, max_grad_norm=None)

HAND_CASES = [(s, False) for s in S.HAND_SHAPES] + [(s, True) for s in S.HAND_SHAPES[:2]]
HAND_CASES += [(s, False) for s in S.TEAM_SHAPES] + [(S.AGENTS_SHAPE, True)]       # (own-critic teams; one of them prioritised)


@pytest.mark.parametrize("shape,prio", HAND_CASES, ids=[D.shape_id(s) + ("-prioritised" if prio else "") for s, prio in HAND_CASES])
def test_an_update_is_the_by_hand_sequence_of_the_public_primitives_bit_for_bit(shape, prio):
    learner, hand = _learner(shape, prio, updates=2), _hand(shape, prio, updates=2)
    start = S.snapshot(learner)
    assert O.differing(start, S.snapshot(hand)) == []
    for call in range(2):
        stats = learner.update()
        hand.update()
        a, b = S.snapshot(learner), S.snapshot(hand)
        assert O.differing(a, b) == [], (call, O.differing(a, b))
        assert stats is learner.stats and stats.shape == (2, 8) and float(stats[1, 0]) == shape[0] * shape[1]
        assert torch.equal(learner.td.view(torch.int32), hand.td.view(torch.int32))
    assert int(learner.step_critic) == 4 == int(learner.step_actor) == int(learner.step_alpha) and int(learner.buffer._draws) == 4
    assert int(learner._noise_draws) == 8                                      # two draws per update
    assert torch.equal(learner.buffer.last_idx, hand.buffer.last_idx)
    moved = set(O.differing(start, a))
    assert {"actor.w1", "critic.w1", "critic2.w1", "target_critic.w2", "target_critic2.w2", "_blob_a", "_blob_c", "_blob_c2", "_blob_tc", "_blob_tc2",
            "adam_actor.m", "adam_critic.v", "adam_critic2.v", "stats", "stats_pi", "step_stats_actor", "step_stats_critic", "draws", "noise_draws",
            "log_std", "log_alpha", "adam_log_std.m", "adam_alpha.v", "step_alpha"} <= moved
    assert not prio or {"leaves", "tree", "max_priority"} <= moved
    # SAC has no target actor: the inherited one is never read or stepped
    assert not {k for k in moved if k.startswith("target_actor.")} and "_blob_ta" not in moved
    O.blobs_are_packs(learner)
    pi = learner.stats_pi.cpu().numpy()
    assert (pi[:, 0] == shape[0] * shape[1]).all() and (pi[:, 7] == 0).all() and ((0 <= pi[:, 6]) & (pi[:, 6] <= 1)).all()
    # alpha's mean: four Adam steps of at most about lr_alpha = 3e-4 each from log 0.2;  q_gap: the critics differ
    assert (np.abs(np.log(pi[:, 4] / 0.2)) <= 4 * 1.5 * 3e-4).all() and float(learner.stats[1, 7]) > 0.0


@pytest.mark.parametrize("prio,shape", [(False, S.MAIN_SHAPES[0]), (True, S.MAIN_SHAPES[0]), (False, S.AGENTS_SHAPE)],
                         ids=["uniform", "prioritised", "uniform-" + D.shape_id(S.AGENTS_SHAPE)])
def test_a_captured_update_runs_nothing_replays_the_eager_updates_with_fresh_draws_and_noise_and_allocates_nothing(prio, shape):
    captured, eager = (_learner(shape, prio, updates=2) for _ in range(2))
    state = [t.detach().clone() for t in captured._state()]
    O.capture_runs_nothing(captured, S.snapshot)
    assert all(torch.equal(a.view(torch.uint8), b.detach().view(torch.uint8)) for a, b in zip(state, captured._state()))
    for t in (captured._noise_draws, captured.log_std, captured.log_alpha, captured.step_alpha, captured.adam_alpha.m, captured.adam_log_std.v,
              captured._blob_c2, captured._blob_tc2, captured.stats_pi):
        assert any(t is s for s in captured._state())
    assert not prio or any(t is captured.buffer.tree for t in captured._state())
    draws, tds, logps = [], [], []

    def each(u):
        draws.append(captured.buffer.last_idx.clone())
        tds.append(captured.td.clone())
        logps.append(captured._logp.clone())
        assert torch.equal(captured.td.view(torch.int32), eager.td.view(torch.int32))
    O.replays_the_eager_updates(captured, eager, S.snapshot, 2, each)
    assert not torch.equal(draws[0], draws[1]) and not torch.equal(tds[0], tds[1]) and not torch.equal(logps[0], logps[1])
    assert int(captured.buffer._draws) == 4 and int(captured._noise_draws) == 8 and int(captured.step_critic) == 4 == int(captured.step_alpha)
    O.blobs_are_packs(captured)
    O.allocates_nothing(captured)


def test_with_lr_alpha_none_the_temperature_never_moves_and_set_lr_reaches_the_captured_step():
    shape = S.MAIN_SHAPES[0]
    fixed = _learner(shape, updates=2, lr_alpha=None, alpha=0.3).capture()
    la0 = fixed.log_alpha.clone()
    for _ in range(2):
        fixed.update()
    assert torch.equal(fixed.log_alpha.view(torch.int32), la0.view(torch.int32)) and int(fixed.step_alpha) == 0 and fixed.adam_alpha is None
    assert float(la0[0]) == float(np.float32(math.log(0.3))) and int(fixed.step_actor) == 4
    assert np.allclose(fixed.stats_pi[:, 4].cpu().numpy(), 0.3, rtol=1e-6)
    with pytest.raises(ValueError, match="lr_alpha=None"):
        fixed.set_lr(alpha=1e-3)
    moving = _learner(shape, updates=1, lr_alpha=1e-2).capture()
    moving.update()
    la1 = moving.log_alpha.clone()
    assert not torch.equal(la1, la0) and int(moving.step_alpha) == 1
    moving.set_lr(alpha=0.0)                                                    # a rate of 0: the captured step reads it and stands still
    moving.update()
    assert torch.equal(moving.log_alpha.view(torch.int32), la1.view(torch.int32)) and int(moving.step_alpha) == 2
    # the learner steps the caller's log_std in place
    own = torch.full((shape[1], 3), -0.5, device="cuda")
    x = _learner(shape, log_std=own)
    x.update()
    assert x.log_std is own and bool((own != -0.5).all())


@pytest.mark.parametrize("shape", S.STEP_SHAPES, ids=D.shape_id)
def test_a_whole_update_with_distinct_targets_and_distinct_critics_against_float64(shape):
    """One whole update through the primitives (Hand.step, ddpg_util.STEP_KW, both draws' normals injected, random log_std and
    log_alpha) from target critics that are NOT the critics, against sac_util.stepped_case's float64 reference with the same computation
    in float32 on the CPU as the yardstick: both critics' gradient rows and their joint step with both targets, the actor's row at the
    STEPPED critics and its step, log_std's gradient and step, log_alpha's gradient and step -- each pooled, ddpg_util.check_step's bars
    (2, 4); log_std's and log_alpha's gradients, three numbers and one per agent, by (2, 4) or the factor yardstick_util's rule makes of
    the yardstick's own recorded spread (profiles/sac_float64.json) -- and both statistics rows.  BSX_SAC_RATIOS_OUT names a file the measured ratios are appended to."""
    B, nA, Do, k, central = shape
    c = S.stepped_case(shape)
    assert c.share < D.U.KINK_CAP
    hand = _hand(shape, seed=c.seed, updates=1, log_std=c.log_std.cuda().contiguous(), lr_alpha=S.ALPHA_LR, **D.STEP_KW)
    hand.log_alpha.copy_(c.log_alpha)
    for name, net in zip(("actor", "critic", "critic2"), c.nets):
        assert all(torch.equal(getattr(getattr(hand, name), p).cpu(), getattr(net, p)) for p in D.PARAMS), name
    O.set_targets(hand, dict(zip(("critic", "critic2"), c.targets)))
    O.blobs_are_packs(hand)
    out = hand.step(*O.sample_is(hand, c.idx, c.batch), 0, weight=c.w.cuda(), z_next=c.z_next.cuda(), z_pi=c.z_pi.cuda())
    torch.cuda.synchronize()
    sid, rec = D.shape_id(shape), {}
    num = lambda row, na: list(O.grad_arrays(row, na).values())                            # noqa: E731
    lst = lambda g: [g[p] for p in D.PARAMS]                                               # noqa: E731
    print("SAC", sid)
    got = dict(gc1=num(out["row_c"], 1), gc2=num(out["row_c2"], 1), ga=num(out["row_a"], k), g_ls=[out["g_log_std"].double().cpu().numpy()],
               g_la=[out["g_log_alpha"].double().cpu().numpy()])
    ref, yard = ({**{w_: lst(r[w_]) for w_ in ("gc1", "gc2", "ga")}, "g_ls": [r["g_ls"]], "g_la": [r["g_la"]]} for r in (c.ref, c.yard))
    D.check_step(got, ref, yard, "row", rec, names=("gc1", "gc2", "ga"))
    for which in ("critic", "critic2"):
        D.check_step(O.step_arrays(hand, which), c.ref[which], c.yard[which], which, rec)
    D.check_step(O.step_arrays(hand, "actor"), c.ref["actor"], c.yard["actor"], "actor", rec, names=("p", "m", "v"))
    # what has one value per agent (and column): (2, 4), or the factor the rule makes of the yardstick's own recorded spread
    arr = lambda *ts: dict(zip(("p", "m", "v"), (t.detach().double().cpu().numpy() for t in ts)))          # noqa: E731
    mine = dict(g_ls=got["g_ls"][0], g_la=got["g_la"][0])
    for name, step in (("log_std", arr(hand.log_std, hand.adam_log_std.m, hand.adam_log_std.v)),
                       ("log_alpha", arr(hand.log_alpha, hand.adam_alpha.m, hand.adam_alpha.v))):
        mine.update({f"{name}.{k_}": v for k_, v in step.items()})
    f, r64, r32 = S.stepped_factor_of(shape), S.small(c.ref), S.small(c.yard)
    ratios, bad = S.Y.check_tensors([(n_, mine[n_], r64[n_], r32[n_], f(n_)) for n_ in S.SMALL], "small", "pooled")
    rec.update({f"small.{n_}": [round(v[0], 4), round(v[1], 4)] for n_, v in ratios.items()})
    assert not bad, (bad, ratios)
    assert int(hand.step_critic) == 1 == int(hand.step_actor) == int(hand.step_alpha) and int(hand._noise_draws) == 0
    bad = S.HEAD.stats_out_of_bounds(hand.stats[0].cpu().numpy(), c.stats, c.e_stats, f"SAC {sid}")
    bad += O.stats_out_of_bounds(hand.stats_pi[0].cpu().numpy(), c.stats_pi, c.e_stats_pi, S.PI_STAT_NAMES, f"SAC {sid} policy")
    assert not bad, bad
    O.blobs_are_packs(hand)
    O.append_ratios("BSX_SAC_RATIOS_OUT", sid, rec)


@pytest.mark.parametrize("which", ["log_alpha", "log_std"])
def test_every_agent_s_own_temperature_and_spread_reach_its_own_update_and_no_other_agent_s(which):
    """4v4 with own critics, the same ring, networks, seed and so the same batch and the same Philox normals, no clipping (a clip norm is
    one number over all agents) and ddpg_util.STEP_KW's eps (at 1e-8 Adam's first step is lr sign(g): a stepped critic would hardly see its
    gradient move): with log_alpha[2], or log_std[2], alone changed, agent 2's column of td and its rows of critic 1's and
    of the actor's gradient (through both stepped critics) differ, and those of agents 0, 1 and 3 keep their bits: own critics share
    nothing between agents.  The device-side twin of test_sac_cpu.py's agent-index misreadings."""
    shape, j = S.AGENTS_SHAPE, 2
    nA = shape[1]
    g = torch.Generator().manual_seed(32)
    log_std, log_alpha = -1.0 + 0.3 * torch.randn((nA, 3), generator=g), math.log(0.2) + 0.3 * torch.randn((nA,), generator=g)
    runs = []
    for changed in (False, True):
        ls, la = log_std.clone(), log_alpha.clone()
        if changed:
            (la if which == "log_alpha" else ls)[j] += 0.5
        hand = _hand(shape, updates=1, log_std=ls.cuda(), **NO_CLIP)
        hand.log_alpha.copy_(la)
        out = hand.step(*O.batch_of(hand.buffer.sample()), 0)
        torch.cuda.synchronize()
        runs.append(dict(idx=hand.buffer.last_idx.clone(), td=hand.td.t().contiguous(), gc1=out["row_c"], ga=out["row_a"]))
        assert int(hand._noise_draws) == 2
    a, b = runs
    assert torch.equal(a["idx"], b["idx"])
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))                   # noqa: E731
    for name in ("td", "gc1", "ga"):                                                            # each [nA, .]: one row per agent
        assert a[name].shape[0] == nA and bool(torch.isfinite(a[name]).all())
        assert [same(a[name][i], b[name][i]) for i in range(nA)] == [i != j for i in range(nA)], (which, name)


def test_one_iteration_of_the_documented_loop_on_a_continuous_1v1_env_with_a_gaussian_rollout():
    """tests/test_hip_ddpg_loop.py's first case -- 1v1 continuous, E = 32, T = 8, a scripted opponent, red plays -- with
    PolicyRollout(sample="gaussian", log_std=...): run, append_rollout, update, publish; the team's rows of the rollout's log_std and of
    its packed weights are the learner's bit for bit, the other team's rows are untouched, and the next run() plays with them."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.learner import SACLearner
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    n, E, Tn, seed = 1, 32, 8, 41

    def make():
        env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, continuous_actions=True); env.reset()
        torch.manual_seed(seed)
        actor = StackedActor(2 * n, 3 * n + 2, 3, device="cuda")
        with torch.no_grad():
            actor.w3.mul_(100.0)
        log_std = torch.full((2 * n, 3), math.log(0.2), device="cuda")
        ro = PolicyRollout(env, actor, Tn, noise_std=0.0, one_launch=True, sample="gaussian", log_std=log_std,
                           opponent=instinct.Team(env.possible_blue, env.possible_red, env))
        ro.start()
        return env, ro
    (env, ro), (_, base) = make(), make()
    cols = range(n)
    buf = DeviceReplayBuffer(600, 300, env.possible_red, env.obs_size, env.obs_size * n, 3, device="cuda", seed=3)
    actor = StackedActor(n, ro.actor.obs_len, 3, device="cuda")
    with torch.no_grad():
        for p in D.PARAMS:
            getattr(actor, p).copy_(getattr(ro.actor, p)[:n])
    learner = SACLearner(buf, actor, critic_input="own", updates=2, **KW)
    w0, ls0 = ro.fused.weights.clone(), ro.log_std.clone()
    ro.run(); base.run()
    assert torch.equal(ro.scores, base.scores)
    assert int(buf.append_rollout(ro, cols).item()) > 0
    learner.update()
    learner.publish(ro, cols)
    torch.cuda.synchronize()
    assert torch.equal(ro.log_std[:n].view(torch.int32), learner.log_std.view(torch.int32)) and not torch.equal(ro.log_std[:n], ls0[:n])
    assert torch.equal(ro.fused.weights[:n].view(torch.int32), learner._blob_a.view(torch.int32)) and not torch.equal(ro.fused.weights[:n], w0[:n])
    assert torch.equal(ro.log_std[n:].view(torch.int32), ls0[n:].view(torch.int32))
    assert torch.equal(ro.fused.weights[n:].view(torch.int32), w0[n:].view(torch.int32))
    for p in D.PARAMS:
        assert torch.equal(getattr(ro.actor, p)[:n], getattr(learner.actor, p)) and torch.equal(getattr(ro.actor, p)[n:], getattr(base.actor, p)[n:])
    ro.run(); base.run()
    torch.cuda.synchronize()
    assert not torch.equal(ro.scores[..., :n, :], base.scores[..., :n, :])       # the next run() plays the published policy
    assert bool(torch.isfinite(learner.stats).all()) and bool(torch.isfinite(learner.stats_pi).all())


def test_captured_updates_on_a_bandit_learn_at_least_half_of_what_the_torch_composition_learns():
    """offpolicy_util's bandit at k = 3 (every row finished), own critics, a fixed temperature, updates = 10, captured.  N and the torch
    composition's figures are recorded in profiles/sac_float64.json, chosen on the CPU with the torch composition of the same SAC alone,
    which itself closes at least half of the gap from its initial reward to 0 in N updates (re-run here: a fraction of a second)."""
    from deep_rl_battlespace_amd.learner import SACLearner
    b = S.BANDIT
    make = lambda ring, *nets: SACLearner(ring, *nets, critic_input="own", alpha=b["alpha"], lr_alpha=None, tau=b["tau"], lr_actor=b["lr"],     # noqa: E731
                                          lr_critic=b["lr"], updates=10)
    learner, N, rec = O.bandit_test(S.PROFILE, S.bandit_torch_run, make, O.bandit_nets(b=b, critic2="next"), "torch composition of SAC", b)
    assert {k: rec[k] for k in b} == b
    assert int(learner.step_actor) == N == int(learner.step_critic) and int(learner.step_alpha) == 0
