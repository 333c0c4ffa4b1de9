"""What tests/dqn_util.py and tests/qmix_util.py share, as csrc/bsx_q_head.h and learner.dqn._QLearner are what the two heads and the two
learners share:

  tail32, tail64, element_loss   the head's tail from the TD target down restated ONCE each: in numpy float32 operation by operation
                     (both contract32), in numpy float64 (both ref64, with stats64) and as the torch element loss (both torch_loss)
  stats_out_of_bounds, guarded_head   the head suites' scaffolding, which differs between the two by a list
  NAMES, snapshot, Hand, step_arrays   what a learner of one or two networks holds under which names, the bits an update leaves, and
                     the base of the two by-hand updates: each Hand.one keeps its own sequence of public primitives
  captured_update, set_lr_and_sync, publish_rows   the bodies of the learner suites' capture, set_lr / sync and publish tests

Nothing here imports the native library at import time."""
import copy

import numpy as np
import torch

import actor_grad_util as U
import offpolicy_util as O
import yardstick_util as Y

PARAMS = U.PARAMS


# ------------------------------------------------------------------------------------------------ the head's tail
def tail32(fmaf, Q, N, R, w, gamma, q_scale, delta, B):
    """include/battlespace_hip.h's tail of both heads in numpy float32, every operation rounded once -> (y, g).  Q, N, R, w: float32
    arrays of one shape; fmaf: the caller's float32 fused multiply-add; call it under np.errstate(all="ignore")."""
    f32 = np.float32
    qs, dl, s2 = f32(q_scale), f32(delta), f32(2.0 / B)
    y = fmaf(gamma, N, R)
    d = (Q - y).astype(f32)
    c = np.where(d == d, np.minimum(np.maximum(d, -dl), dl), d).astype(f32) if delta > 0 else d      # a NaN stays a NaN
    return y, (((w * c).astype(f32) * s2).astype(f32) * qs).astype(f32)


def tail64(Q, N, R, w, gamma, q_scale, delta, B):
    """The same in float64 on the terms as given -> (y, d, the loss term l(d), g); gamma: already float32's."""
    y = gamma * N + R
    d = Q - y
    c = np.clip(d, -delta, delta) if delta > 0 else d
    loss = np.where(np.abs(d) <= delta, d * d, delta * (2 * np.abs(d) - delta)) if delta > 0 else d * d
    return y, d, loss, w * c * (2.0 / B) * q_scale


def stats64(n, w, loss, Q, y, d, over, greedy):
    """stats [8] from tail64's terms: means over n of the arrays' sums (over and greedy: the head's own terms of those two)."""
    return np.array([n, (w * loss).sum() / n, Q.sum() / n, y.sum() / n, np.abs(d).sum() / n, over.sum() / n, w.sum() / n, greedy.sum() / n])


def element_loss(Q, y, delta):
    """l(Q - y) per element as a torch user writes it: mse, or 2 delta smooth_l1(beta=delta)."""
    F = torch.nn.functional
    return 2.0 * delta * F.smooth_l1_loss(Q, y, reduction="none", beta=delta) if delta > 0 else F.mse_loss(Q, y, reduction="none")


# ------------------------------------------------------------------------------------------------ the head suites' scaffolding
def stats_out_of_bounds(got, ref, e_stats, names, exact, what=""):
    """exact: the (index, name) pairs held exactly (n and the counts' means: exact in float64); the others by yardstick_util.scalar_bound."""
    return [name for i, name in exact if got[i] != ref[i]] + Y.stats_out_of_bounds(got, ref, e_stats, names, what)


def guarded_head(inp, outs, workspace_bytes, call, guarded=False, fill=7.0, td=True, keep=None):
    """call(dev, out, ws), a head binding on `inp`, with every input, output and the workspace between guard slabs (guarded) and every
    output float starting as `fill` -> (the binding's result: the `out` tensors themselves, the strays).  outs: the (name, shape) pairs of
    the float32 outputs ahead of td and stats.  keep: receives the workspace (int64, -1 before the call) as [workgroups, 8] partial rows."""
    from guard_util import Buffers
    B, nA = inp["rew"].shape
    G = Buffers(guarded)
    dev = O.put(G, inp)
    out = tuple(G(k, s, torch.float32, init=fill) for k, s in outs) + (G("td", (B, nA), torch.float32, init=fill) if td else None,
                                                                       G("stats", (8,), torch.float64, init=fill))
    ws = G("workspace", (workspace_bytes // 8,), torch.int64, init=-1)
    res = call(dev, out, ws)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(res, out))
    if keep is not None:
        keep["workspace"] = ws.view(-1, 8)
    return res, G.stray()


# ------------------------------------------------------------------------------------------------ one update by hand
# per network of a learner: its blob, its target's blob, its AdamState, its step counter and its step statistics
NAMES = dict(qnet=("_blob_q", "_blob_tq", "adam", "step", "step_stats"), mixer=("_blob_m", "_blob_tm", "adam_mixer", "step_mixer", "step_stats_mixer"))


def snapshot(x, nets=("qnet",)):
    """{name: bits} of everything an update of x (a learner or a Hand of the networks `nets`) writes that outlives it: per network the
    blobs, step word, step statistics, parameters, target and moments; the statistics, the ring's draw counter and prioritised state."""
    torch.cuda.synchronize()
    out = dict(stats=x.stats.detach().clone(), draws=x.buffer._draws.clone())
    for net in nets:
        blob, tblob, adam, step, step_stats = NAMES[net]
        out.update({k: getattr(x, k).detach().clone() for k in (blob, tblob, step, step_stats)})
        for name in (net, "target_" + net):
            for p in PARAMS:
                out[f"{name}.{p}"] = getattr(getattr(x, name), p).detach().clone()
        out[adam + ".m"], out[adam + ".v"] = getattr(x, adam).m.clone(), getattr(x, adam).v.clone()
    if hasattr(x.buffer, "tree"):
        out.update(leaves=x.buffer._leaves.clone(), tree=x.buffer.tree.clone(), max_priority=x.buffer.max_priority.clone())
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v.view(torch.int64) if v.dtype == torch.float64 else v) for k, v in out.items()}


class Hand:
    """What a learner of the networks `nets` (name -> network, NAMES' names) holds, under the same names: per network its target, both
    blobs, AdamState, step counter and step statistics; ONE hyper row; the statistics.  A subclass writes one() with public primitives alone."""

    def __init__(self, buffer, nets, double=True, q_scale=None, huber_delta=0.0, gamma=None, tau=0.01, lr=1e-3, max_grad_norm=None, updates=1,
                 betas=(0.9, 0.999), eps=1e-8):
        from deep_rl_battlespace_amd import learner as L
        self.buffer, self.double, self.q_scale, self.huber_delta, self.gamma, self.updates = buffer, double, q_scale, huber_delta, gamma, updates
        self.prioritized = hasattr(buffer, "tree")
        dev = nets["qnet"].w1.device
        for name, net in nets.items():
            blob, tblob, adam, step, step_stats = NAMES[name]
            target = copy.deepcopy(net)
            target.__dict__.pop("_bsx_mlp_buffers", None)
            for k, v in ((name, net), ("target_" + name, target), (blob, net.pack()), (tblob, target.pack()), (adam, L.AdamState(net)),
                         (step, torch.zeros(1, dtype=torch.int64, device=dev)),
                         (step_stats, torch.zeros((updates, 4), dtype=torch.float64, device=dev))):
                setattr(self, k, v)
        self.actor = self.qnet                                                      # (actor: what offpolicy_loop_util.twin_publish copies)
        self.hyper = L.adam_hyper(lr, betas, eps, max_grad_norm, dev, tau)
        self.stats = torch.zeros((updates, 8), dtype=torch.float64, device=dev)
        self.q = self.td = None

    def update(self):
        for u in range(self.updates):
            self.one(*O.batch_of(self.buffer.sample()), u, weight=self.buffer.weights if self.prioritized else None)
        return self.stats

    forward = O.Hand.forward

    def q_rows(self, obs, obs_next):
        """The Q network's three forwards -> (y_cur, y_next_online or None without double Q, y_next_target)."""
        return (self.forward(self._blob_q, obs), self.forward(self._blob_q, obs_next) if self.double else None, self.forward(self._blob_tq, obs_next))


def step_arrays(x, which="qnet"):
    """dict(p, m, v, target) of lists of ten numpy arrays: x's network `which`, its moments and its target (offpolicy_util.step_arrays' form)."""
    import adam_util as AU
    state = getattr(x, NAMES[which][2])
    cut = lambda row: AU.row_to_tensors(row.detach().cpu().numpy(), 4)              # noqa: E731
    return dict(p=AU.net_arrays(getattr(x, which)), m=cut(state.m), v=cut(state.v), target=AU.net_arrays(getattr(x, "target_" + which)))


# ------------------------------------------------------------------------------------------------ the learner suites' shared bodies
def _pairs(x, nets):
    """(network, its blob) of every network and target of x."""
    return [(getattr(x, t + net), getattr(x, NAMES[net][1 if t else 0])) for net in nets for t in ("", "target_")]


def captured_update(captured, eager, prio, nets=("qnet",)):
    """Four replays against four eager calls, every bit of snapshot() exact after each one and the tree of a prioritised ring exact;
    capture() undoes its warm-up; every network's state is in _state(); nothing is allocated."""
    snap = lambda x: snapshot(x, nets)                                              # noqa: E731
    state = [t.detach().clone() for t in captured._state()]
    O.capture_runs_nothing(captured, snap)
    assert all(torch.equal(a.view(torch.uint8), b.detach().view(torch.uint8)) for a, b in zip(state, captured._state()))
    assert any(t is captured.buffer._draws for t in captured._state()) and len(state) == len(eager._state())
    for net in nets:
        blob, tblob, adam, step, _ = NAMES[net]
        assert all(any(t is x for t in captured._state()) for x in (getattr(captured, blob), getattr(captured, tblob), getattr(captured, adam).m,
                                                                    getattr(captured, step))), net
    assert not prio or all(any(t is x for t in captured._state()) for x in (captured.buffer.tree, captured.buffer._leaves, captured.buffer.max_priority))
    draws = []

    def each(u):
        draws.append(captured.buffer.last_idx.clone())
        assert torch.equal(captured.td.view(torch.int32), eager.td.view(torch.int32))
        if prio:
            tree = captured.buffer.tree.clone()
            captured.buffer.rebuild_tree()
            torch.cuda.synchronize()
            assert torch.equal(tree, captured.buffer.tree), u                        # the tree is exact after every replay
    O.replays_the_eager_updates(captured, eager, snap, 4, each)
    assert not torch.equal(draws[0], draws[1]) and int(captured.buffer._draws) == 8
    assert all(int(getattr(captured, NAMES[net][3])) == 8 for net in nets)
    O.allocates_nothing(captured)


def set_lr_and_sync(a, b, nets=("qnet",)):
    """a, b: two learners alike.  A replay sees set_lr(0): every step runs and moves nothing; sync() re-packs every blob after an edit."""
    import pytest
    snap = lambda x: snapshot(x, nets)                                              # noqa: E731
    a.capture(), b.capture()
    a.update(), b.update()
    assert O.differing(snap(a), snap(b)) == []
    a.set_lr(0.0)
    before = snap(a)
    a.update(), b.update()
    after, other = snap(a), snap(b)
    for net in nets:
        blob, _, adam, step, _ = NAMES[net]
        assert all(torch.equal(before[f"{net}.{p}"], after[f"{net}.{p}"]) for p in PARAMS) and torch.equal(before[blob], after[blob])
        assert not torch.equal(before[adam + ".m"], after[adam + ".m"]) and int(getattr(a, step)) == 2     # the step ran, with a rate of 0
        assert not torch.equal(after[f"{net}.w1"], other[f"{net}.w1"])
    with pytest.raises(ValueError, match="lr"):
        a.set_lr(-1.0)
    # an outside edit: the blobs are stale until sync()
    with torch.no_grad():
        for net in nets:
            getattr(a, net).w3.mul_(0.5)
            getattr(a, "target_" + net).b3.add_(0.25)
    assert all(not torch.equal(net.pack().view(torch.int32), blob.view(torch.int32)) for net, blob in _pairs(a, nets))
    a.sync()
    assert all(torch.equal(net.pack().view(torch.int32), blob.view(torch.int32)) for net, blob in _pairs(a, nets))


def publish_rows(make, B):
    """make(ring, qnet) -> a learner on a 2v2 env's shapes; publish() writes the Q network's blob rows and parameter slices into its own
    columns of the rollout and nothing else, and refuses columns that are no contiguous range of the team's size.  -> the learner"""
    import pytest

    import ddpg_util as D
    import offpolicy_loop_util as LU
    from deep_rl_battlespace_amd.rollout import StackedActor
    env, ro = LU.rollout(2, 16, 4, False, True, 7)
    n = 2
    torch.manual_seed(5)
    qnet = StackedActor(n, env.obs_size, 4, device="cuda")
    learner = make(O.ring(D.ring_rows(4 * B, n, env.obs_size, 4, 3), B), qnet)
    assert learner._actor_net.net is qnet
    learner.update()
    for cols in (range(n), range(n, 2 * n)):
        w0 = ro.fused.weights.clone()
        p0 = {p: getattr(ro.actor, p).detach().clone() for p in PARAMS}
        learner.publish(ro, cols)
        torch.cuda.synchronize()
        mine, other = list(cols), [c for c in range(2 * n) if c not in cols]
        assert torch.equal(ro.fused.weights[mine].view(torch.int32), learner._blob_q.view(torch.int32))
        assert torch.equal(ro.fused.weights[other].view(torch.int32), w0[other].view(torch.int32))
        for p in PARAMS:
            assert torch.equal(getattr(ro.actor, p)[mine], getattr(learner.qnet, p)) and torch.equal(getattr(ro.actor, p)[other], p0[p][other]), p
    for bad in (range(1, 2), [0, 2], range(3, 5)):
        with pytest.raises(ValueError, match="contiguous range"):
            learner.publish(ro, bad)
    return learner
