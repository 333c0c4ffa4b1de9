"""learner.PPOLearner on the MI355X, over the small rollout record of the existing PPO test: one minibatch's gradients and loss against
the torch loss of tests/test_hip_actor_grad.py (`_ppo`: the same reference, the same bounds); update() against the same sequence written
out by hand, bit for bit, with nothing allocated the second time and the rollout playing the updated weights; constructor refusals."""
import numpy as np
import pytest
import torch

import actor_grad_util as U
import ppo_learner_util as L
from test_hip_actor_grad import CLIP, _ppo, _to

pytestmark = pytest.mark.gpu


def _record(ro, cont):
    T = ro.T
    act = ro.scores.clone() if cont else ro.scores.argmax(-1)
    rec = dict(obs=ro.obs[:T].clone(), act=act, logp=ro.logp.clone(), adv=ro.adv.clone(), ret=ro.ret.clone(), mask=ro.mask.clone())
    return {k: v.cpu() for k, v in rec.items()}


# ---------------------------------------------------------------------------------------------------- 1. against torch
@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_one_minibatch_meets_the_bounds_of_the_fused_ppo_loss_against_torch(kind):
    from deep_rl_battlespace_amd.learner import PPOLearner, split_grad
    ro = L.small_rollout(kind)
    cont = kind == "gaussian"
    rec = _record(ro, cont)
    actor0, critic = _to(ro.actor, "cpu"), _to(ro.value_actor, "cpu")
    ls_cpu = ro.log_std.cpu() if cont else None
    T, E, A, D = rec["obs"].shape
    flat_obs = rec["obs"].reshape(-1, A, D)
    # the learner's policy is one step of the existing test's ladder away from the one that played; rows kept as there
    for scale in (0.03, 0.06, 0.12, 0.25, 0.5, 1.0):
        actor = _to(actor0, "cpu")
        L.nudge(actor, scale)
        near = (U.pre_relu64(actor, flat_obs).abs() < U.KINK).any(-1) | (U.pre_relu64(critic, flat_obs).abs() < U.KINK).any(-1)
        keep = rec["mask"] & ~near.transpose(0, 1).reshape(T, E, A)
        r64 = _ppo(actor, critic, ls_cpu, rec, keep, kind, False, "cpu", torch.float64)[4].reshape(T, E, A)
        keep = keep & ((r64 - (1 - CLIP)).abs() > 1e-4) & ((r64 - (1 + CLIP)).abs() > 1e-4)
        kept, clipped = int(keep.sum()), int((keep & ((r64 < 1 - CLIP) | (r64 > 1 + CLIP))).sum())
        print(kind, "step", scale, "rows kept", kept, "of", int(rec["mask"].sum()), "masked; clipped", clipped)
        if 0.05 * kept <= clipped <= 0.6 * kept:
            break
    assert kept >= 0.9 * int(rec["mask"].sum()) and kept >= 500 and 0.05 * kept <= clipped <= 0.6 * kept
    L64, a64, c64, l64, _ = _ppo(actor, critic, ls_cpu, rec, keep, kind, False, "cpu", torch.float64)
    _, a32, c32, _, _ = _ppo(actor, critic, ls_cpu, rec, keep, kind, False, "cpu", torch.float32)
    Lt, _, _, lt, _ = _ppo(actor, critic, ls_cpu, rec, keep, kind, False, "cuda", torch.float32)
    e_loss, e_ls = abs(Lt - L64), (np.abs(lt - l64).max() if cont else 0.0)
    for p in range(8):
        perm = torch.randperm(T * E, generator=torch.Generator().manual_seed(4000 + p))
        Lp, _, _, lp, _ = _ppo(actor, critic, ls_cpu, rec, keep, kind, False, "cuda", torch.float32, perm)
        e_loss = max(e_loss, abs(Lp - L64))
        if cont:
            e_ls = max(e_ls, np.abs(lp - l64).max())
    e_loss = max(e_loss, 0.5 * float(np.spacing(np.float32(abs(L64)))))
    # the learner over the rollout itself: its actor moved to the learner's policy, its mask cut to the kept rows
    with torch.no_grad():
        for k in U.PARAMS:
            getattr(ro.actor, k).copy_(getattr(actor, k))
    ro._mask.copy_(keep.to(torch.uint8))
    # `_ppo` weighs (v - ret)^2 by 0.5 and the entropy by 0.01: c_v = 1 on lv = (v - ret)^2 / 2
    learner = PPOLearner(ro, clip=CLIP, c_v=1.0, c_e=0.01, epochs=1, minibatches=1)
    row_a, row_v, g_ls, stats = learner.minibatch_grads(0, T)
    torch.cuda.synchronize()
    af = {k: g.double().cpu().numpy() for k, g in zip(U.PARAMS, split_grad(row_a, ro.actor.n_actions))}
    cf = {k: g.double().cpu().numpy() for k, g in zip(U.PARAMS, split_grad(row_v, 1))}
    Lf = float(stats[1])
    assert float(stats[0]) == kept
    print(kind, f"loss float64 {L64:.9g} learner {Lf:.9g} torch {Lt:.9g}; |learner - torch| {abs(Lf - Lt):.3e}, |learner - f64| {abs(Lf - L64):.3e}, "
                f"torch's own error (max of 9 row orders, at least half a float32 spacing) {e_loss:.3e}")
    assert abs(Lf - Lt) <= 4 * e_loss and abs(Lf - L64) <= 4 * e_loss
    U.check(af, a64, a32, f"PPO learner {kind} actor")
    U.check(cf, c64, c32, f"PPO learner {kind} critic")
    if cont:
        lf = g_ls.double().cpu().numpy()
        print(kind, f"log_std gradient: |learner - f64| {np.abs(lf - l64).max():.3e}, torch's own error {e_ls:.3e}, max |g| {np.abs(l64).max():.3e}")
        assert np.abs(lf - l64).max() <= 4 * e_ls
    else:
        assert g_ls is None


# ---------------------------------------------------------------------------------------------------- 2. update()
def _state(learner):
    """Clones of everything an update moves: parameters (log_std among them) and the optimiser's state, in parameter order."""
    out = [p.detach().clone() for p in learner.params]
    for p in learner.params:
        for k, v in sorted(learner.optimizer.state[p].items()):
            out.append(v.detach().clone() if isinstance(v, torch.Tensor) else torch.tensor(v))
    return out


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_update_is_the_hand_written_sequence_bit_for_bit_allocates_once_and_reaches_the_rollout(kind):
    from deep_rl_battlespace_amd.learner import PPOLearner, _buffers, split_grad
    ro = L.small_rollout(kind)
    T, kw = ro.T, dict(clip=0.2, c_v=0.5, c_e=0.01, vclip=0.2, epochs=2, minibatches=2)
    start = [p.detach().clone() for p in PPOLearner(ro, **kw).params]
    learner = PPOLearner(ro, lr=1e-3, **kw)
    stats = learner.update()
    torch.cuda.synchronize()
    assert stats.shape == (4, 8) and stats.is_cuda and bool(torch.isfinite(stats).all()) and bool((stats[:, 0] > 100).all())
    assert float((stats[1:, 5] - stats[0, 5]).abs().max()) > 0                  # later minibatches see a policy that has moved
    assert not torch.equal(learner.params[0], start[0])
    got = _state(learner)
    # the next run plays the updated weights
    assert torch.equal(ro.fused.weights, ro.actor.pack()) and torch.equal(ro._value_w, ro.value_actor.pack())
    # the same sequence by hand, from the same start: ticks [0, T/2) then [T/2, T) in each of two epochs, every gradient replaced
    with torch.no_grad():
        for p, s in zip(learner.params, start):
            p.copy_(s)
            p.grad = None
    hand = PPOLearner(ro, optimizer=torch.optim.Adam(learner.params, lr=1e-3), **kw)
    rows = []
    for _ in range(2):
        for t0, t1 in ((0, T // 2), (T // 2, T)):
            row_a, row_v, g_ls, st = hand.minibatch_grads(t0, t1)
            for net, row in ((ro.actor, row_a), (ro.value_actor, row_v)):
                for k, g in zip(U.PARAMS, split_grad(row, net.n_actions)):
                    getattr(net, k).grad = g.clone(memory_format=torch.contiguous_format)
            if g_ls is not None:
                ro.log_std.grad = g_ls.clone()
            hand.optimizer.step()
            rows.append(st.clone())
    torch.cuda.synchronize()
    want = _state(hand)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(torch.stack(rows), stats)
    # a second update allocates nothing: the same buffers, at the same addresses
    def held():                                                                 # noqa: E306
        out = {("head", R, k): v.data_ptr() for R, b in hand._by_rows.items() for k, v in b.items() if v is not None}
        for net in (ro.actor, ro.value_actor):
            for key, b in _buffers(net).by_key.items():
                out.update({(id(net), key, k): (v.data_ptr() if v is not None else None) for k, v in b.items()})
        return out
    hand.update()
    before = held()
    assert len(hand._by_rows) == 1 and all(b["go"] is None for b in _buffers(ro.actor).by_key.values())
    hand.update()
    torch.cuda.synchronize()
    assert held() == before
    assert torch.equal(ro.fused.weights, ro.actor.pack())
    ro.run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ro.logp).all()) and bool(torch.isfinite(ro.adv).all())


def test_max_grad_norm_bounds_the_step_and_an_own_optimizer_is_used():
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout("categorical")
    learner = PPOLearner(ro, epochs=1, minibatches=1, max_grad_norm=1e-3)
    opt = torch.optim.SGD(learner.params, lr=1.0)
    learner = PPOLearner(ro, epochs=1, minibatches=1, max_grad_norm=1e-3, optimizer=opt)
    before = [p.detach().clone() for p in learner.params]
    learner.update()
    moved = torch.sqrt(sum(((p.detach() - b) ** 2).sum() for p, b in zip(learner.params, before)))
    assert 0 < float(moved) <= 1e-3 * (1 + 1e-4)                                # lr 1: the step IS the clipped gradient


# ---------------------------------------------------------------------------------------------------- 3. refusals
def test_the_learner_refuses_rollouts_it_cannot_learn_from():
    from deep_rl_battlespace_amd.learner import PPOLearner
    with pytest.raises(ValueError, match="gae="):
        PPOLearner(L.small_rollout("categorical", gae=False))
    with pytest.raises(ValueError, match="sample="):
        PPOLearner(L.small_rollout("gaussian", sample=False))
    ro = L.small_rollout("categorical")
    with pytest.raises(ValueError, match="divides T"):
        PPOLearner(ro, minibatches=3)
    with pytest.raises(ValueError, match="clip"):
        PPOLearner(ro, clip=1.5)
    learner = PPOLearner(ro, minibatches=4)
    with pytest.raises(ValueError, match="ticks"):
        learner.minibatch_grads(4, 4)
    with pytest.raises(ValueError, match="ticks"):
        learner.minibatch_grads(0, ro.T + 1)
