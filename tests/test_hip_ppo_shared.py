"""PPOLearner(share=) on the GPU: one policy and one value function per team (or for everyone).  The shared device update against the
hand-written sequence (minibatch_grads, then adam_step(group=g)), members that stay identical in parameters, moments and the rollout's
blob rows, allocation, the captured update against the eager one with and without shuffle=True, the first step against the torch path
around the float64 restatement, a scripted opponent, the refusals, and share=None against a learner built without the argument.

The rollout is tests/ppo_learner_util.small_rollout (T = 8, E = 96), tied after it returns, re-packed and run once more: n = 2 with
share="team", n = 1 with share="all", both kinds; n = 2 with a scripted blue team.  The hyper-parameters and the harness are that file's."""
import pytest
import torch

import ppo_learner_util as L
import shared_step_util as S
from ppo_learner_util import KW, STEPS

pytestmark = pytest.mark.gpu
#        id                         kind        n  share  opponent
CASES = {"categorical-2v2-team": ("categorical", 2, "team", None), "gaussian-2v2-team": ("gaussian", 2, "team", None),
         "categorical-1v1-all": ("categorical", 1, "all", None), "gaussian-1v1-all": ("gaussian", 1, "all", None),
         "gaussian-2v2-team-vs-scripted-blue": ("gaussian", 2, "team", "blue")}
FREE = [c for c in CASES if CASES[c][3] is None]


def _tied_rollout(case, tie=True):
    """-> (rollout, share, g): small_rollout with its networks and log_std tied in groups of g, both blobs re-packed, one more run."""
    from deep_rl_battlespace_amd.learner import share_group, tie_
    kind, n, share, opponent = CASES[case]
    ro = L.small_rollout(kind, n=n, opponent=opponent)
    g = share_group(share, n)
    if tie:
        for x in (ro.actor, ro.value_actor, ro.log_std):
            if x is not None:
                tie_(x, g)
        ro.fused.refresh()
        ro.value_actor.pack(out=ro._value_w)
        ro.run()
        torch.cuda.synchronize()
    return ro, share, g


@pytest.mark.parametrize("case", list(CASES))
def test_the_shared_device_update_is_the_hand_written_sequence_bit_for_bit_and_members_stay_identical(case):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro, share, g = _tied_rollout(case)
    kind = CASES[case][0]
    start = L.keep(ro)
    assert L.blobs_are_packs(ro)
    learner = PPOLearner(ro, device_step=True, share=share, **KW)
    assert learner.group == g and g > 1
    stats = learner.update()
    got = L.everything(learner)
    assert stats.shape == (STEPS, 8) and bool(torch.isfinite(stats).all())
    assert learner.step_stats[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and int(learner.step_count) == STEPS
    assert bool((learner.step_stats[:, 1] > 0).all()) and bool((learner.step_stats[:, 2] <= 1).all())
    assert not torch.equal(got[0], start[0]) and L.blobs_are_packs(ro)
    assert L.members_are_identical(learner, g) is None
    # the same sequence by hand from the same start: minibatch_grads on the blobs as they stand, then adam_step(group=g) on the rows
    L.restore(ro, start)
    assert L.equal(got, L.by_hand(ro, kind, L.tick_ranges_of(PPOLearner(ro, device_step=True, share=share, **KW)), group=g))
    # the untied step on the same rows is another update: the argument reached the kernel
    L.restore(ro, start)
    PPOLearner(ro, device_step=True, **KW).update()
    torch.cuda.synchronize()
    assert not torch.equal(ro.actor.w1.detach(), got[0])
    L.restore(ro, start)
    L.allocates_nothing(learner)
    assert L.blobs_are_packs(ro) and L.members_are_identical(learner, g) is None
    ro.run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro.logp).all()) and bool(torch.isfinite(ro.adv).all()) and bool(torch.isfinite(ro.scores).all())


@pytest.mark.parametrize("shuffle", [False, True], ids=["ticks", "shuffle"])
@pytest.mark.parametrize("case", FREE)
def test_the_captured_shared_update_replays_to_the_eager_bits(case, shuffle):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro, share, g = _tied_rollout(case)
    kw = dict(KW, shuffle=True, shuffle_seed=5) if shuffle else KW

    def each(update, graph):
        assert L.members_are_identical(graph, g) is None
    _, graph, _ = L.eager_and_captured(ro, lambda: PPOLearner(ro, device_step=True, share=share, **kw), each=each)
    assert int(graph.step_count) == 8 and graph.step_stats[:, 0].tolist() == [5.0, 6.0, 7.0, 8.0]
    if shuffle:
        assert int(graph.shuffle_base) == 2 * KW["epochs"]


def test_the_first_shared_device_step_agrees_with_the_torch_path_around_the_float64_restatement():
    """The method and the bars of the unshared learner's test, PPOLearner(share="team") against shared_reference_step."""
    ro, share, g = _tied_rollout("gaussian-2v2-team")
    L.first_step_meets_the_bars(ro, dict(share=share), lambda *step: S.shared_reference_step(*step, g), g=g, norm_rtol=1e-6)


@pytest.mark.parametrize("device_step", [True, False], ids=["device", "torch"])
def test_with_a_scripted_blue_team_red_moves_as_one_and_blue_keeps_every_bit(device_step):
    from deep_rl_battlespace_amd.learner import PPOLearner
    case = "gaussian-2v2-team-vs-scripted-blue"
    ro, share, g = _tied_rollout(case)
    n = CASES[case][1]
    scripted, learned = L.scripted_columns(n, "blue")
    with pytest.raises(ValueError, match="scripted"):
        PPOLearner(ro, device_step=device_step, share="all", **KW)
    with pytest.raises(ValueError, match="scripted"):
        PPOLearner(ro, device_step=device_step, share=2 * n, **KW)
    learner = PPOLearner(ro, device_step=device_step, share="team", **KW)
    before = L.keep(ro) + ([t.clone() for t in L.moments(learner)] if device_step else [])
    learner.update()
    after = L.keep(ro) + ([t.clone() for t in L.moments(learner)] if device_step else [])
    assert L.blobs_are_packs(ro)
    for i, (b, a) in enumerate(zip(before, after)):
        assert torch.equal(L.bits(b, scripted), L.bits(a, scripted)), i
        assert not torch.equal(L.bits(b, learned[:1]), L.bits(a, learned[:1])), i
        red = L.bits(a, learned).view(len(learned), -1)
        assert torch.equal(red, red[:1].expand_as(red)), i                          # red's planes hold one policy, still


def test_untied_networks_are_refused_with_the_message_that_names_tie_and_nothing_is_tied_silently():
    from deep_rl_battlespace_amd.learner import PPOLearner, is_tied, tie_
    ro, share, g = _tied_rollout("gaussian-2v2-team", tie=False)
    kept = L.keep(ro)
    for device_step in (True, False):
        with pytest.raises(ValueError, match=r"learner\.tie_"):
            PPOLearner(ro, device_step=device_step, share=share, **KW)
    # each of the three on its own is enough to refuse
    tie_(ro.actor, g); tie_(ro.value_actor, g); tie_(ro.log_std, g)
    tied = L.keep(ro)
    for name, t in (("actor", ro.actor.b3), ("value_actor", ro.value_actor.w2), ("log_std", ro.log_std)):
        with torch.no_grad():
            t[1].add_(0.5)
        with pytest.raises(ValueError, match=rf"{name}.*learner\.tie_"):
            PPOLearner(ro, device_step=True, share=share, **KW)
        L.restore(ro, tied)
    assert not is_tied(ro.actor, 2 * g)
    with pytest.raises(ValueError, match=r"learner\.tie_"):
        PPOLearner(ro, device_step=True, share="all", **KW)                         # tied per team is not tied for everyone
    assert L.equal(L.keep(ro), tied) and not L.equal(tied, kept)
    for bad in ("red", 3, 0, 2.0):
        with pytest.raises(ValueError):
            PPOLearner(ro, share=bad, **KW)
    ro.fused.refresh(); ro.value_actor.pack(out=ro._value_w)
    assert PPOLearner(ro, device_step=True, share=share, **KW).group == g


@pytest.mark.parametrize("device_step", [True, False], ids=["device", "torch"])
def test_share_none_gives_the_bits_of_a_learner_built_without_the_argument(device_step):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout("gaussian", n=2)
    start = L.keep(ro)
    results = []
    for kw in ({}, dict(share=None), dict(share=1)):
        L.restore(ro, start)
        learner = PPOLearner(ro, device_step=device_step, **KW, **kw)
        assert learner.group == 1
        learner.update()
        torch.cuda.synchronize()
        results.append(L.keep(ro) + [learner.stats.clone()] + ([t.clone() for t in L.moments(learner)] if device_step else []))
    assert L.equal(results[0], results[1]) and L.equal(results[0], results[2])
    assert not L.equal(results[0][:1], start[:1])
