"""PPOLearner(device_step=True) on the GPU: update() with the fused optimiser step (learner.adam_step) against the hand-written sequence,
the captured update against the eager one, allocation, the first step against the default torch path, a scripted opponent, refusals.
The rollout is tests/ppo_learner_util.small_rollout: n = 1, E = 96, T = 8, both kinds; the harness is that file's."""
import numpy as np
import pytest
import torch

import adam_util as U
import ppo_learner_util as L
from ppo_learner_util import KW, STEPS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_the_device_update_is_the_hand_written_sequence_bit_for_bit_allocates_once_and_reaches_the_rollout(kind):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout(kind)
    start = L.keep(ro)
    assert L.blobs_are_packs(ro)
    learner = PPOLearner(ro, device_step=True, **KW)
    stats = learner.update()
    got = L.everything(learner)
    assert stats.shape == (STEPS, 8) and bool(torch.isfinite(stats).all()) and bool((stats[:, 0] > 100).all())
    assert learner.step_stats[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and int(learner.step_count) == STEPS
    assert bool((learner.step_stats[:, 1] > 0).all()) and bool((learner.step_stats[:, 2] <= 1).all())
    assert bool((learner.step_stats[:, 3] == float(np.float32(KW["lr"]))).all())
    assert all(p.grad is None for p in learner.params)                              # .grad stays unset on this path
    assert not torch.equal(got[0], start[0]) and L.blobs_are_packs(ro)
    # the same sequence by hand from the same start: minibatch_grads on the blobs as they stand, then adam_step on the rows
    L.restore(ro, start)
    assert L.equal(got, L.by_hand(ro, kind, L.tick_ranges_of(PPOLearner(ro, device_step=True, **KW))))
    L.restore(ro, start)
    L.allocates_nothing(learner)
    assert L.blobs_are_packs(ro)
    ro.run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro.logp).all()) and bool(torch.isfinite(ro.adv).all()) and bool(torch.isfinite(ro.scores).all())


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_the_captured_update_is_the_eager_one_bit_for_bit_and_follows_set_lr(kind):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout(kind)
    _, graph, _ = L.eager_and_captured(ro, lambda: PPOLearner(ro, device_step=True, **KW))
    assert int(graph.step_count) == 8 and graph.step_stats[:, 0].tolist() == [5.0, 6.0, 7.0, 8.0]
    # a learning rate set between replays is the one the next replay steps with
    def moved():                                                                    # noqa: E306
        kept = L.keep(ro)
        graph.update()
        torch.cuda.synchronize()
        d = torch.sqrt(sum(((a.double() - b.double()) ** 2).sum() for a, b in zip([t.detach() for t in L.shared(ro)[:20]], kept[:20])))
        L.restore(ro, kept)
        return float(d)
    own = [t.clone() for t in L.own(graph)]
    small = moved()
    with torch.no_grad():
        for t, k in zip(L.own(graph), own):
            t.copy_(k)
    graph.set_lr(1e-2)
    large = moved()
    assert bool((graph.step_stats[:, 3] == float(np.float32(1e-2))).all()) and graph.step_stats[:, 0].tolist() == [9.0, 10.0, 11.0, 12.0]
    assert 5.0 * small < large < 20.0 * small, (small, large)


def test_the_first_device_step_agrees_with_the_default_torch_path_around_the_float64_restatement():
    L.first_step_meets_the_bars(L.small_rollout("gaussian"), {}, U.reference_step, norm_rtol=1e-10)


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_a_scripted_opponents_agents_keep_every_bit_and_the_learned_ones_move(kind):
    from deep_rl_battlespace_amd.learner import PPOLearner
    n = 2
    ro = L.small_rollout(kind, n=n, opponent="blue")
    learner = PPOLearner(ro, device_step=True, **KW)
    before = L.everything(learner)
    learner.update()
    after = L.everything(learner)
    assert int(learner.step_count) == 4 and L.blobs_are_packs(ro)
    L.scripted_keep_every_bit_and_learned_move(learner, before, after, *L.scripted_columns(n, "blue"))


def test_the_device_path_refuses_what_it_cannot_do():
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout("categorical")
    opt = torch.optim.SGD([ro.actor.w1], lr=1.0)
    with pytest.raises(ValueError, match="optimizer"):
        PPOLearner(ro, device_step=True, optimizer=opt)
    plain = PPOLearner(ro)
    for call in (plain.capture, plain.sync, lambda: plain.set_lr(1e-3)):
        with pytest.raises(ValueError, match="device_step=True"):
            call()
    with pytest.raises(ValueError, match="betas"):
        PPOLearner(ro, device_step=True, betas=(0.9, 1.5))
    learner = PPOLearner(ro, device_step=True, epochs=1, minibatches=1)
    with pytest.raises(ValueError, match="lr"):
        learner.set_lr(-1.0)
    kept = L.keep(ro)
    w2 = ro.actor.w2
    ro.actor.w2 = torch.nn.Parameter(w2.detach().transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match=r"w2.*contiguous"):
        learner.update()
    ro.actor.w2 = w2
    torch.cuda.synchronize()
    assert int(learner.step_count) == 0 and L.equal(L.keep(ro), kept)               # refused before the step was launched
    # sync(): parameters edited from outside reach both blobs
    with torch.no_grad():
        ro.actor.b3.add_(0.25)
        ro.value_actor.b3.sub_(0.5)
    assert not L.blobs_are_packs(ro)
    learner.sync()
    assert L.blobs_are_packs(ro)
    learner.update()
    assert int(learner.step_count) == 1 and L.blobs_are_packs(ro)
