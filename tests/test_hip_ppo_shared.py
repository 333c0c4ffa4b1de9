"""PPOLearner(share=) on the GPU: one policy and one value function per team (or for everyone).  The shared device update against the
hand-written sequence (minibatch_grads, then adam_step(group=g)), members that stay identical in parameters, moments and the rollout's
blob rows, allocation, the captured update against the eager one with and without shuffle=True, the first step against the torch path
around the float64 restatement, a scripted opponent, the refusals, and share=None against a learner built without the argument.

The rollout is tests/ppo_learner_util.small_rollout (T = 8, E = 96), tied after it returns, re-packed and run once more: n = 2 with
share="team", n = 1 with share="all", both kinds; n = 2 with a scripted blue team."""
import numpy as np
import pytest
import torch

import adam_util as U
import ppo_learner_util as L
import shared_step_util as S

pytestmark = pytest.mark.gpu
KW = dict(clip=0.2, c_v=0.5, c_e=0.01, vclip=0.2, epochs=2, minibatches=2, max_grad_norm=0.5, lr=1e-3)
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


def _shared(ro):
    """The tensors two learners on one rollout share: the parameters, the rollout's two blobs and log_std."""
    out = [getattr(net, k) for net in (ro.actor, ro.value_actor) for k in U.PARAMS] + [ro.fused.weights, ro._value_w]
    return out + ([ro.log_std] if ro.log_std is not None else [])


def _keep(ro):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in _shared(ro)]


def _restore(ro, kept):
    with torch.no_grad():
        for t, k in zip(_shared(ro), kept):
            t.copy_(k)


def _moments(learner):
    out = [learner.adam_a.m, learner.adam_a.v, learner.adam_v.m, learner.adam_v.v]
    return out + ([learner.adam_ls.m, learner.adam_ls.v] if learner.adam_ls is not None else [])


def _own(learner):
    out = _moments(learner) + [learner.step_count, learner.stats, learner.step_stats]
    return out + ([learner.shuffle_base, learner.minibatch_idx] if learner.shuffle else [])


def _everything(learner):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in _shared(learner.rollout) + _own(learner)]


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def _blobs_are_packs(ro):
    return (torch.equal(ro.fused.weights.view(torch.int32), ro.actor.pack().view(torch.int32))
            and torch.equal(ro._value_w.view(torch.int32), ro.value_actor.pack().view(torch.int32)))


def _members_are_identical(learner, g):
    """Every member equals its group's leader, bit for bit: parameters, log_std, the rollout's blob rows, the moments."""
    torch.cuda.synchronize()
    for i, t in enumerate(_shared(learner.rollout) + _moments(learner)):
        v = t.detach().contiguous().view(torch.int32).view(t.shape[0] // g, g, -1)
        if not torch.equal(v, v[:, :1].expand_as(v)):
            return i
    return None


def _held(learner):
    from deep_rl_battlespace_amd.learner import _buffers
    out = {("head", R, k): v.data_ptr() for R, b in learner._by_rows.items() for k, v in b.items() if v is not None}
    for net in (learner.actor, learner.critic):
        for key, b in _buffers(net).by_key.items():
            out.update({(id(net), key, k): (v.data_ptr() if v is not None else None) for k, v in b.items()})
    out.update({("own", i): t.data_ptr() for i, t in enumerate(_own(learner) + [learner.hyper, learner._adam_ws])})
    out.update({("shared", i): t.data_ptr() for i, t in enumerate(_shared(learner.rollout))})
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_the_shared_device_update_is_the_hand_written_sequence_bit_for_bit_and_members_stay_identical(case):
    from deep_rl_battlespace_amd.learner import AdamState, PPOLearner, adam_hyper, adam_step
    ro, share, g = _tied_rollout(case)
    kind = CASES[case][0]
    start = _keep(ro)
    assert _blobs_are_packs(ro)
    learner = PPOLearner(ro, device_step=True, share=share, **KW)
    assert learner.group == g and g > 1
    stats = learner.update()
    got = _everything(learner)
    steps = KW["epochs"] * KW["minibatches"]
    assert stats.shape == (steps, 8) and bool(torch.isfinite(stats).all())
    assert learner.step_stats[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and int(learner.step_count) == steps
    assert bool((learner.step_stats[:, 1] > 0).all()) and bool((learner.step_stats[:, 2] <= 1).all())
    assert not torch.equal(got[0], start[0]) and _blobs_are_packs(ro)
    assert _members_are_identical(learner, g) is None
    # the same sequence by hand from the same start: minibatch_grads on the blobs as they stand, then adam_step(group=g) on the rows
    _restore(ro, start)
    hand = PPOLearner(ro, device_step=True, share=share, **KW)
    nets = [ro.actor, ro.value_actor]
    states = [AdamState(ro.actor), AdamState(ro.value_actor)]
    ls_state = AdamState(ro.log_std) if kind == "gaussian" else None
    hyper, count = adam_hyper(KW["lr"], (0.9, 0.999), 1e-8, KW["max_grad_norm"]), torch.zeros(1, dtype=torch.int64, device="cuda")
    head_rows, step_rows, span = [], [], ro.T // KW["minibatches"]
    for _ in range(KW["epochs"]):
        for m in range(KW["minibatches"]):
            row_a, row_v, g_ls, st = hand.minibatch_grads(m * span, (m + 1) * span, pack=False)
            head_rows.append(st.clone())
            step_rows.append(adam_step(nets, [row_a, row_v], states, [ro.fused.weights, ro._value_w], hyper, count,
                                       log_std=ro.log_std if ls_state else None, g_log_std=g_ls, log_std_state=ls_state, group=g).clone())
    torch.cuda.synchronize()
    want = [t.detach().clone() for t in _shared(ro)] + [states[0].m, states[0].v, states[1].m, states[1].v] + \
        ([ls_state.m, ls_state.v] if ls_state else []) + [count, torch.stack(head_rows), torch.stack(step_rows)]
    assert _equal(got, want)
    # the untied step on the same rows is another update: the argument reached the kernel
    _restore(ro, start)
    PPOLearner(ro, device_step=True, **KW).update()
    torch.cuda.synchronize()
    assert not torch.equal(ro.actor.w1.detach(), got[0])
    # a second update allocates nothing: the same bytes in use, the same buffers at the same addresses
    _restore(ro, start)
    learner.update()
    torch.cuda.synchronize()
    before, in_use = _held(learner), torch.cuda.memory_allocated()
    learner.update()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == in_use and _held(learner) == before
    assert _blobs_are_packs(ro) and _members_are_identical(learner, g) is None
    ro.run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro.logp).all()) and bool(torch.isfinite(ro.adv).all()) and bool(torch.isfinite(ro.scores).all())


@pytest.mark.parametrize("shuffle", [False, True], ids=["ticks", "shuffle"])
@pytest.mark.parametrize("case", FREE)
def test_the_captured_shared_update_replays_to_the_eager_bits(case, shuffle):
    """Twin learners on one rollout, one eager, one captured; what they share is put back between their turns."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro, share, g = _tied_rollout(case)
    kw = dict(KW, shuffle=True, shuffle_seed=5) if shuffle else KW
    eager, graph = PPOLearner(ro, device_step=True, share=share, **kw), PPOLearner(ro, device_step=True, share=share, **kw)
    start, own = _keep(ro), _everything(graph)
    assert graph.capture() is graph
    assert _equal(_everything(graph), own)                                          # capture() itself moved nothing
    for update in range(2):
        eager.update()
        a = _everything(eager)
        _restore(ro, start)
        graph.update()
        b = _everything(graph)
        assert _equal(a, b), update
        assert not torch.equal(b[0], start[0]) and _blobs_are_packs(ro) and _members_are_identical(graph, g) is None
        ro.run()                                                                    # fresh records under the updated policy
        start = _keep(ro)
    assert int(graph.step_count) == 8 and graph.step_stats[:, 0].tolist() == [5.0, 6.0, 7.0, 8.0]
    if shuffle:
        assert int(graph.shuffle_base) == 2 * KW["epochs"]


def test_the_first_shared_device_step_agrees_with_the_torch_path_around_the_float64_restatement():
    """The method and the bars of the unshared learner's test: one optimiser step from one start state on the same gradient rows and
    the same float32-representable hyperparameters, PPOLearner(share="team")'s torch path (group sums on the leaders' .grad, torch's
    clip_grad_norm_ + Adam, leaders copied over followers) and its device path, both against shared_reference_step -- per network,
    pooled over the leaders' tensors: mean |error| at most 2x torch's, maximum at most 4x.  On both paths every member ends equal to
    its leader."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro, share, g = _tied_rollout("gaussian-2v2-team")
    hp = U.hyper32(lr=3e-4, max_grad_norm=0.5)
    kw = dict(KW, epochs=1, minibatches=1, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], share=share)
    start = _keep(ro)
    device = PPOLearner(ro, device_step=True, **kw)
    rows = [r.clone() if r is not None else None for r in device.minibatch_grads(0, ro.T, pack=False)[:3]]
    nets = (ro.actor, ro.value_actor)
    lead = lambda xs: [np.asarray(x)[::g] for x in xs]     # noqa: E731

    def arrays():
        torch.cuda.synchronize()
        return [U.net_arrays(ro.actor) + [ro.log_std.detach().cpu().numpy().copy()], U.net_arrays(ro.value_actor)]
    p0 = arrays()
    grads = [U.row_to_tensors(rows[0].cpu().numpy(), 3) + [rows[2].cpu().numpy()], U.row_to_tensors(rows[1].cpu().numpy(), 1)]
    flat = lambda groups: [x for grp in groups for x in grp]     # noqa: E731
    zeros = [np.zeros_like(x, dtype=np.float64) for x in flat(p0)]
    P, M, V, t, norm, coef = S.shared_reference_step(flat(p0), flat(grads), zeros, zeros, 0, hp, g)
    assert coef < 1.0                                                                # the bound bites: clipping is part of what is compared
    device.update()
    got = arrays()
    got_m = [U.row_to_tensors(device.adam_a.m.cpu().numpy(), 3) + [device.adam_ls.m.cpu().numpy()], U.row_to_tensors(device.adam_v.m.cpu().numpy(), 1)]
    got_v = [U.row_to_tensors(device.adam_a.v.cpu().numpy(), 3) + [device.adam_ls.v.cpu().numpy()], U.row_to_tensors(device.adam_v.v.cpu().numpy(), 1)]
    assert abs(float(device.step_stats[0, 1]) - norm) <= 1e-6 * norm                # (float32 group sums against float64 ones)
    assert _members_are_identical(device, g) is None
    _restore(ro, start)
    default = PPOLearner(ro, **kw)
    assert all(torch.equal(a, b) for a, b in zip(default.minibatch_grads(0, ro.T)[:3], rows))      # the same gradient rows, bit for bit
    default.update()
    torch.cuda.synchronize()
    assert _blobs_are_packs(ro)
    for t_ in _shared(ro):                                                           # the torch path ties after its step, before the re-pack
        v = t_.detach().view(t_.shape[0] // g, g, -1)
        assert torch.equal(v, v[:, :1].expand_as(v))
    ref_p, ref_m, ref_v = [P[:11], P[11:]], [M[:11], M[11:]], [V[:11], V[11:]]
    tor = arrays()
    state = lambda key: [[default.optimizer.state[getattr(net, k)][key].cpu().numpy() for k in U.PARAMS] for net in nets]     # noqa: E731
    tor_m, tor_v = state("exp_avg"), state("exp_avg_sq")
    tor_m[0].append(default.optimizer.state[ro.log_std]["exp_avg"].cpu().numpy())
    tor_v[0].append(default.optimizer.state[ro.log_std]["exp_avg_sq"].cpu().numpy())
    failed = []
    for i in range(2):
        for what, mine, theirs, want in (("p", got, tor, ref_p), ("m", got_m, tor_m, ref_m), ("v", got_v, tor_v, ref_v)):
            (em, ex), (tm, tx) = U.pooled_errors(lead(mine[i]), lead(want[i])), U.pooled_errors(lead(theirs[i]), lead(want[i]))
            print(f"net{i}.{what}: device {em:.3e} / {ex:.3e}, torch {tm:.3e} / {tx:.3e}")
            assert tm > 0.0 and tx > 0.0
            if em > 2.0 * tm or ex > 4.0 * tx:
                failed.append((i, what, em, tm, ex, tx))
    assert not failed, failed


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
    before = _keep(ro) + ([t.clone() for t in _moments(learner)] if device_step else [])
    learner.update()
    after = _keep(ro) + ([t.clone() for t in _moments(learner)] if device_step else [])
    assert _blobs_are_packs(ro)
    bits = lambda x, cols: x[cols].contiguous().view(torch.int32)     # noqa: E731
    for i, (b, a) in enumerate(zip(before, after)):
        assert torch.equal(bits(b, scripted), bits(a, scripted)), i
        assert not torch.equal(bits(b, learned[:1]), bits(a, learned[:1])), i
        red = bits(a, learned).view(len(learned), -1)
        assert torch.equal(red, red[:1].expand_as(red)), i                          # red's planes hold one policy, still


def test_untied_networks_are_refused_with_the_message_that_names_tie_and_nothing_is_tied_silently():
    from deep_rl_battlespace_amd.learner import PPOLearner, is_tied, tie_
    ro, share, g = _tied_rollout("gaussian-2v2-team", tie=False)
    kept = _keep(ro)
    for device_step in (True, False):
        with pytest.raises(ValueError, match=r"learner\.tie_"):
            PPOLearner(ro, device_step=device_step, share=share, **KW)
    # each of the three on its own is enough to refuse
    tie_(ro.actor, g); tie_(ro.value_actor, g); tie_(ro.log_std, g)
    tied = _keep(ro)
    for name, t in (("actor", ro.actor.b3), ("value_actor", ro.value_actor.w2), ("log_std", ro.log_std)):
        with torch.no_grad():
            t[1].add_(0.5)
        with pytest.raises(ValueError, match=rf"{name}.*learner\.tie_"):
            PPOLearner(ro, device_step=True, share=share, **KW)
        _restore(ro, tied)
    assert not is_tied(ro.actor, 2 * g)
    with pytest.raises(ValueError, match=r"learner\.tie_"):
        PPOLearner(ro, device_step=True, share="all", **KW)                         # tied per team is not tied for everyone
    assert _equal(_keep(ro), tied) and not _equal(tied, kept)
    for bad in ("red", 3, 0, 2.0):
        with pytest.raises(ValueError):
            PPOLearner(ro, share=bad, **KW)
    ro.fused.refresh(); ro.value_actor.pack(out=ro._value_w)
    assert PPOLearner(ro, device_step=True, share=share, **KW).group == g


@pytest.mark.parametrize("device_step", [True, False], ids=["device", "torch"])
def test_share_none_gives_the_bits_of_a_learner_built_without_the_argument(device_step):
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout("gaussian", n=2)
    start = _keep(ro)
    results = []
    for kw in ({}, dict(share=None), dict(share=1)):
        _restore(ro, start)
        learner = PPOLearner(ro, device_step=device_step, **KW, **kw)
        assert learner.group == 1
        learner.update()
        torch.cuda.synchronize()
        results.append(_keep(ro) + [learner.stats.clone()] + ([t.clone() for t in _moments(learner)] if device_step else []))
    assert _equal(results[0], results[1]) and _equal(results[0], results[2])
    assert not _equal(results[0][:1], start[:1])
