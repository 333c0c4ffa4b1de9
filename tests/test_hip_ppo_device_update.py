"""PPOLearner(device_step=True) on the GPU: update() with the fused optimiser step (learner.adam_step) against the hand-written sequence,
the captured update against the eager one, allocation, the first step against the default torch path, a scripted opponent, refusals.
The rollout is tests/ppo_learner_util.small_rollout: n = 1, E = 96, T = 8, both kinds."""
import numpy as np
import pytest
import torch

import adam_util as U
import ppo_learner_util as L

pytestmark = pytest.mark.gpu
KW = dict(clip=0.2, c_v=0.5, c_e=0.01, vclip=0.2, epochs=2, minibatches=2, max_grad_norm=0.5, lr=1e-3)


def _shared(ro):
    """The tensors two learners on one rollout share: the parameters, log_std and the rollout's two blobs."""
    out = [getattr(net, k) for net in (ro.actor, ro.value_actor) for k in U.PARAMS] + [ro.fused.weights, ro._value_w]
    return out + ([ro.log_std] if ro.log_std is not None else [])


def _keep(ro):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in _shared(ro)]


def _restore(ro, kept):
    with torch.no_grad():
        for t, k in zip(_shared(ro), kept):
            t.copy_(k)


def _own(learner):
    out = [learner.adam_a.m, learner.adam_a.v, learner.adam_v.m, learner.adam_v.v, learner.step_count, learner.stats, learner.step_stats]
    return out + ([learner.adam_ls.m, learner.adam_ls.v] if learner.adam_ls is not None else [])


def _everything(learner):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in _shared(learner.rollout) + _own(learner)]


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def _blobs_are_packs(ro):
    return (torch.equal(ro.fused.weights.view(torch.int32), ro.actor.pack().view(torch.int32))
            and torch.equal(ro._value_w.view(torch.int32), ro.value_actor.pack().view(torch.int32)))


def _held(learner):
    from deep_rl_battlespace_amd.learner import _buffers
    out = {("head", R, k): v.data_ptr() for R, b in learner._by_rows.items() for k, v in b.items() if v is not None}
    for net in (learner.actor, learner.critic):
        for key, b in _buffers(net).by_key.items():
            out.update({(id(net), key, k): (v.data_ptr() if v is not None else None) for k, v in b.items()})
    out.update({("own", i): t.data_ptr() for i, t in enumerate(_own(learner) + [learner.hyper, learner._adam_ws])})
    out.update({("shared", i): t.data_ptr() for i, t in enumerate(_shared(learner.rollout))})
    return out


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_the_device_update_is_the_hand_written_sequence_bit_for_bit_allocates_once_and_reaches_the_rollout(kind):
    from deep_rl_battlespace_amd.learner import AdamState, PPOLearner, adam_hyper, adam_step
    ro = L.small_rollout(kind)
    start = _keep(ro)
    assert _blobs_are_packs(ro)
    learner = PPOLearner(ro, device_step=True, **KW)
    stats = learner.update()
    got = _everything(learner)
    steps = KW["epochs"] * KW["minibatches"]
    assert stats.shape == (steps, 8) and bool(torch.isfinite(stats).all()) and bool((stats[:, 0] > 100).all())
    assert learner.step_stats[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and int(learner.step_count) == steps
    assert bool((learner.step_stats[:, 1] > 0).all()) and bool((learner.step_stats[:, 2] <= 1).all())
    assert bool((learner.step_stats[:, 3] == float(np.float32(KW["lr"]))).all())
    assert all(p.grad is None for p in learner.params)                              # .grad stays unset on this path
    assert not torch.equal(got[0], start[0]) and _blobs_are_packs(ro)
    # the same sequence by hand from the same start: minibatch_grads on the blobs as they stand, then adam_step on the rows
    _restore(ro, start)
    hand = PPOLearner(ro, device_step=True, **KW)
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
                                       log_std=ro.log_std if ls_state else None, g_log_std=g_ls, log_std_state=ls_state).clone())
    torch.cuda.synchronize()
    want = [t.detach().clone() for t in _shared(ro)] + [states[0].m, states[0].v, states[1].m, states[1].v, count, torch.stack(head_rows),
                                                      torch.stack(step_rows)] + ([ls_state.m, ls_state.v] if ls_state else [])
    assert _equal(got, want)
    # a second update allocates nothing: the same bytes in use, the same buffers at the same addresses
    _restore(ro, start)
    learner.update()
    torch.cuda.synchronize()
    before, in_use = _held(learner), torch.cuda.memory_allocated()
    learner.update()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == in_use and _held(learner) == before
    assert _blobs_are_packs(ro)
    ro.run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro.logp).all()) and bool(torch.isfinite(ro.adv).all()) and bool(torch.isfinite(ro.scores).all())


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_the_captured_update_is_the_eager_one_bit_for_bit_and_follows_set_lr(kind):
    """Twin learners on one rollout, one eager, one captured; what they share (parameters, log_std, blobs) is put back between their
    turns, so both take every update from the same state and the same records."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout(kind)
    eager, graph = PPOLearner(ro, device_step=True, **KW), PPOLearner(ro, device_step=True, **KW)
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
        assert not torch.equal(b[0], start[0]) and _blobs_are_packs(ro)
        ro.run()                                                                    # fresh records under the updated policy
        start = _keep(ro)
    assert int(graph.step_count) == 8 and graph.step_stats[:, 0].tolist() == [5.0, 6.0, 7.0, 8.0]
    # a learning rate set between replays is the one the next replay steps with
    def moved():                                                                    # noqa: E306
        kept = _keep(ro)
        graph.update()
        torch.cuda.synchronize()
        d = torch.sqrt(sum(((a.double() - b.double()) ** 2).sum() for a, b in zip([t.detach() for t in _shared(ro)[:20]], kept[:20])))
        _restore(ro, kept)
        return float(d)
    own = [t.clone() for t in _own(graph)]
    small = moved()
    with torch.no_grad():
        for t, k in zip(_own(graph), own):
            t.copy_(k)
    graph.set_lr(1e-2)
    large = moved()
    assert bool((graph.step_stats[:, 3] == float(np.float32(1e-2))).all()) and graph.step_stats[:, 0].tolist() == [9.0, 10.0, 11.0, 12.0]
    assert 5.0 * small < large < 20.0 * small, (small, large)


def test_the_first_device_step_agrees_with_the_default_torch_path_around_the_float64_restatement():
    """One optimiser step from one start state on the same gradient rows and the same (float32-representable) Adam hyperparameters:
    PPOLearner's default path (install + clip_grad_norm_ + torch Adam) and the device path, both against the float64 restatement --
    the kernel test's bars: mean |error| at most 2x torch's, maximum at most 4x, pooled per network."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout("gaussian")
    hp = U.hyper32(lr=3e-4, max_grad_norm=0.5)
    kw = dict(KW, epochs=1, minibatches=1, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    start = _keep(ro)
    device = PPOLearner(ro, device_step=True, **kw)
    rows = [r.clone() if r is not None else None for r in device.minibatch_grads(0, ro.T, pack=False)[:3]]
    nets = (ro.actor, ro.value_actor)

    def arrays():
        torch.cuda.synchronize()
        return [U.net_arrays(ro.actor) + [ro.log_std.detach().cpu().numpy().copy()], U.net_arrays(ro.value_actor)]
    p0 = arrays()
    grads = [U.row_to_tensors(rows[0].cpu().numpy(), 3) + [rows[2].cpu().numpy()], U.row_to_tensors(rows[1].cpu().numpy(), 1)]
    flat = lambda groups: [x for g in groups for x in g]     # noqa: E731
    zeros = [np.zeros_like(x, dtype=np.float64) for x in flat(p0)]
    P, M, V, t, norm, coef = U.reference_step(flat(p0), flat(grads), zeros, zeros, 0, hp)
    assert coef < 1.0                                                                # the bound bites: clipping is part of what is compared
    device.update()
    got = arrays()
    got_m = [U.row_to_tensors(device.adam_a.m.cpu().numpy(), 3) + [device.adam_ls.m.cpu().numpy()], U.row_to_tensors(device.adam_v.m.cpu().numpy(), 1)]
    got_v = [U.row_to_tensors(device.adam_a.v.cpu().numpy(), 3) + [device.adam_ls.v.cpu().numpy()], U.row_to_tensors(device.adam_v.v.cpu().numpy(), 1)]
    assert abs(float(device.step_stats[0, 1]) - norm) <= 1e-10 * norm
    _restore(ro, start)
    default = PPOLearner(ro, **kw)
    assert all(torch.equal(a, b) for a, b in zip(default.minibatch_grads(0, ro.T)[:3], rows))      # the same gradient rows, bit for bit
    default.update()
    torch.cuda.synchronize()
    ref_p = [P[:11], P[11:]]
    ref_m, ref_v = [M[:11], M[11:]], [V[:11], V[11:]]
    tor = arrays()
    state = lambda key: [[default.optimizer.state[getattr(net, k)][key].cpu().numpy() for k in U.PARAMS] for net in nets]     # noqa: E731
    tor_m, tor_v = state("exp_avg"), state("exp_avg_sq")
    tor_m[0].append(default.optimizer.state[ro.log_std]["exp_avg"].cpu().numpy())
    tor_v[0].append(default.optimizer.state[ro.log_std]["exp_avg_sq"].cpu().numpy())
    failed = []
    for i in range(2):
        for what, mine, theirs, want in (("p", got, tor, ref_p), ("m", got_m, tor_m, ref_m), ("v", got_v, tor_v, ref_v)):
            (em, ex), (tm, tx) = U.pooled_errors(mine[i], want[i]), U.pooled_errors(theirs[i], want[i])
            print(f"net{i}.{what}: device {em:.3e} / {ex:.3e}, torch {tm:.3e} / {tx:.3e}")
            assert tm > 0.0 and tx > 0.0
            if em > 2.0 * tm or ex > 4.0 * tx:
                failed.append((i, what, em, tm, ex, tx))
    assert not failed, failed


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_a_scripted_opponents_agents_keep_every_bit_and_the_learned_ones_move(kind):
    from deep_rl_battlespace_amd.learner import PPOLearner
    n = 2
    ro = L.small_rollout(kind, n=n, opponent="blue")
    scripted, learned = L.scripted_columns(n, "blue")
    learner = PPOLearner(ro, device_step=True, **KW)
    before = _everything(learner)
    learner.update()
    after = _everything(learner)
    assert int(learner.step_count) == 4 and _blobs_are_packs(ro)
    names = [f"{net}.{k}" for net in ("actor", "critic") for k in U.PARAMS] + ["blob_a", "blob_v"] + (["log_std"] if kind == "gaussian" else [])
    names += ["m_a", "v_a", "m_v", "v_v", "step", "stats", "step_stats"] + (["m_ls", "v_ls"] if kind == "gaussian" else [])
    assert len(names) == len(before)
    for name, b, a in zip(names, before, after):
        if name in ("step", "stats", "step_stats"):
            continue
        bits = lambda x, cols: x[cols].contiguous().view(torch.int32)     # noqa: E731
        assert torch.equal(bits(b, scripted), bits(a, scripted)), name
        assert not torch.equal(bits(b, learned), bits(a, learned)), name


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
    kept = _keep(ro)
    w2 = ro.actor.w2
    ro.actor.w2 = torch.nn.Parameter(w2.detach().transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match=r"w2.*contiguous"):
        learner.update()
    ro.actor.w2 = w2
    torch.cuda.synchronize()
    assert int(learner.step_count) == 0 and _equal(_keep(ro), kept)                 # refused before the step was launched
    # sync(): parameters edited from outside reach both blobs
    with torch.no_grad():
        ro.actor.b3.add_(0.25)
        ro.value_actor.b3.sub_(0.5)
    assert not _blobs_are_packs(ro)
    learner.sync()
    assert _blobs_are_packs(ro)
    learner.update()
    assert int(learner.step_count) == 1 and _blobs_are_packs(ro)
