"""What the tests of the three off-policy learners (DDPG, TD3, SAC) share that does not depend on the algorithm; tests/ddpg_util.py,
td3_util.py and sac_util.py keep what is theirs and build on this:

  Head               a TD head's kind -- its inputs, its target's next value in numpy float64 and in torch, its critics, whether it seeds
                     the actor -- and, written once over that: the float64 contract (ref), the head as a torch user writes it with
                     autograd (autograd: in float64 the check of the restatement, in float32 the yardstick), both cached per shape (case),
                     the yardstick's own spread (spread), the recorded factors, yardstick_util's bounds (check, stats_out_of_bounds)
  min32, target32    the two lines the float32 contracts of the twin heads share
  first_step         one first Adam step from zero moments over networks and loose tensors with one clip norm and Polyak targets:
                     float64 by adam_mlp_util.reference_step, float32 as a torch user takes it
  kink_fixed_point   the kink filter of the whole-update cases, iterated until no row with a weight lies near a kink
  Hand               what a learner holds, under the same names, and the parts of its update the three by-hand updates share, written
                     with the public primitives alone
  ring, batch_of     a (prioritised) device ring filled with given rows; a sample as the batch the learners read
  the bandit         its rows, reward, networks, the loop round a torch composition, and the GPU test's body
  Suite              what the three learner suites do alike: networks, a learner, a Hand, targets, blobs, a capture against eager updates
  bits, same_bits, numpy_of, put, guarded_head, sentinel_x   what the three head suites do alike
  bandit_section, head_sections, sharpness, kept_kernel   what tools/measure_{ddpg,td3,sac}.py write alike

Nothing here imports the native library at import time."""
import copy
import functools
import gc
import json
import os
import sys

import numpy as np
import torch

import actor_grad_util as U
import actor_ref_util as R
import adam_mlp_util as AM
import adam_util as AU
import yardstick_util as Y

PARAMS = U.PARAMS
GAMMA = 0.95
MAX_ROUNDS = 4                                      # of kink_fixed_point
STAT_NAMES = ("critic_loss", "q", "target", "abs_td", "done", "weight", "q_gap")      # stats[1..7]; a single critic has no q_gap
gpu_copy = U._to


def head_id(B, nA, weight):
    return "B%d-nA%d-%s" % (B, nA, "weighted" if weight else "plain")


# ------------------------------------------------------------------------------------------------ the TD head
def stats_out_of_bounds(got, ref, e_stats, names, what=""):
    """A statistics row against float64 -> the names out of bounds: n exactly, entry 7 exactly 0 where `names` leaves it unnamed, the
    named entries by yardstick_util.stats_out_of_bounds.  got, ref, e_stats: float64 [8]; prints every figure."""
    counts = [] if got[0] == ref[0] and (len(names) == 7 or got[7] == 0.0) else ["n"]
    return counts + Y.stats_out_of_bounds(got, ref, e_stats, names, what)


class Head:
    """A TD head's kind.  inputs(B, nA, seed=0) -> {name: CPU tensor}; qs: the names of its critics' values ("q" / "q1", "q2"), each
    with a g_<name>; pi: whether it has g_pi (from -mean w Q of the first critic); value64(f) / value(t): the next state's value in y =
    r + gamma (1 - done) value, from float64 arrays / from torch tensors; entry, args: learner's binding and its positional arguments
    (input names, "gamma" where gamma goes); profile: the JSON file its factors are recorded in; contract32: the twin heads' float32
    contract.  stats[7] is mean |q1 - q2| with two critics and 0 with one."""

    def __init__(self, inputs, qs, pi, value64, value, entry, args, profile, contract32=None):
        self.inputs, self.qs, self.pi, self.value64, self.value, self.entry, self.args = inputs, qs, pi, value64, value, entry, args
        self.profile, self.contract32 = profile, contract32
        self.grads = tuple("g_" + k for k in qs) + (("g_pi",) if pi else ())
        self.names = self.grads + ("td",)
        self.stat_names = STAT_NAMES[:5 + len(qs)]

    @staticmethod
    def _squares(w, d):
        """The critic loss's summand, in numpy or torch: each kind's own association."""
        return w * d[0] * d[0] if len(d) == 1 else w * (d[0] * d[0] + d[1] * d[1])

    def ref(self, inp, gamma=GAMMA, weight=True):
        """The contract in float64 numpy -> dict(g_*: [B, nA, 4], td [B, nA], stats [8]).  weight=False: w = 1."""
        f = {k: v.double().numpy() for k, v in inp.items()}
        q = [f[k] for k in self.qs]
        B, nA = q[0].shape
        over = f["done"] != 0
        w = f["weight"] if weight else np.ones((B, nA))
        with np.errstate(all="ignore"):
            y = gamma * np.where(over, 0.0, self.value64(f)) + f["rew"]
        d = [x - y for x in q]
        out = {k: np.zeros((B, nA, 4)) for k in self.grads}
        for k, dk in zip(self.grads, d):
            out[k][..., 0] = w * dk * (2.0 / B)
        if self.pi:
            out["g_pi"][..., 0] = -w * (1.0 / B)
        n = float(B * nA)
        stats = np.array([n, self._squares(w, d).sum() / n, q[0].sum() / n, y.sum() / n, np.abs(d[0]).sum() / n, over.sum() / n, w.sum() / n,
                          np.abs(q[0] - q[1]).sum() / n if len(q) == 2 else 0.0])
        return dict(out, td=y, stats=stats)

    def autograd(self, inp, dtype, gamma=GAMMA, weight=True, perm=None):
        """The head as a torch user writes it, on the CPU in `dtype`, with autograd from the critics' values of the sum of the critic
        losses sum_i mean_b w (Q - y)^2 (and of -mean w Q) -> dict of float64 numpy (the gradients padded to 4 columns; the statistics
        computed in `dtype`).  perm: the rows in another order (the per-row outputs come back in the original one)."""
        t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
        if perm is not None:
            t = {k: (v[perm] if v.dim() == 2 else v) for k, v in t.items()}
        q = [t[k].clone().requires_grad_() for k in self.qs]
        w = t["weight"] if weight else torch.ones_like(q[0])
        y = t["rew"] + gamma * (1.0 - t["done"].to(dtype)) * self.value(t)
        functools.reduce(torch.add, [(w * (x - y) ** 2).mean(0).sum() for x in q]).backward()
        leaves = list(q)
        if self.pi:
            q_pi = t[self.qs[0]].clone().requires_grad_()
            (-(w * q_pi).mean(0).sum()).backward()
            leaves.append(q_pi)
        gs = {k: torch.zeros((*q[0].shape, 4), dtype=dtype) for k in self.grads}
        for k, x in zip(self.grads, leaves):
            gs[k][..., 0] = x.grad
        gs["td"] = y
        if perm is not None:
            inv = torch.argsort(perm)
            gs = {k: v[inv] for k, v in gs.items()}
        with torch.no_grad():
            d = [x - y for x in q]
            num = lambda x: float(x.double())                     # noqa: E731
            stats = np.array([float(q[0].numel()), num(self._squares(w, d).mean()), num(q[0].mean()), num(y.mean()), num(d[0].abs().mean()),
                              num(t["done"].to(dtype).mean()), num(w.mean()), num((q[0] - q[1]).abs().mean()) if len(q) == 2 else 0.0])
        return dict({k: v.detach().double().numpy() for k, v in gs.items()}, stats=stats)

    def case(self, B, nA, weight=True, perms=8):
        """(inputs, float64 reference, float32 yardstick, the yardstick's own error on stats [8]: the largest over the given order and
        `perms` permutations of the rows).  Computed once and shared: read-only."""
        return _head_case(self, B, nA, weight, perms)

    def spread(self, B, nA, weight=True, perms=8):
        """{tensor: (max ratio, mean ratio)}: how far the float32 yardstick's own error on the head's tensors moves over equivalent
        float32 evaluations -- the contract's association (contract32) and autograd over yardstick_util.row_orders.  No kernel output
        enters.  With a handful of elements the error is a few draws of a rounding and moves by more than (2, 4): at B = nA = 1 it is ONE."""
        inp, ref, yard, _ = self.case(B, nA, weight)
        others = [self.contract32(inp, weight=weight)] + [self.autograd(inp, torch.float32, weight=weight, perm=o)
                                                         for o in list(Y.row_orders(B, perms))[1:]]
        return U.spread(ref, yard, others, self.names)

    def factors(self, B, nA, weight):
        """tensor -> (mean factor, max factor): what the profile records for the case (from spread), or for the tensor at every shape,
        else the project's (2, 4)."""
        rec = Y.recorded(self.profile, "factors")
        return Y.factor_of(rec.get(head_id(B, nA, weight), {}), rec)

    def stats_out_of_bounds(self, got, ref, e_stats, what=""):
        return stats_out_of_bounds(got, ref, e_stats, self.stat_names, what)

    def check(self, got, ref, yard, e_stats, what="", factor_of=None):
        """got: dict of the head's tensors and stats as float64 numpy from the kernel; factor_of: factors(B, nA, weight).  Prints every
        figure, then asserts."""
        bad = Y.check_tensors([(k, got[k], ref[k], yard[k], (factor_of or Y.factor_of({}))(k)) for k in self.names], what, unit="x")[1]
        bad += self.stats_out_of_bounds(got["stats"], ref["stats"], e_stats, what)
        assert not bad, (what, bad)


@functools.lru_cache(maxsize=None)
def _head_case(head, B, nA, weight, perms):
    inp = head.inputs(B, nA)
    ref, yard = head.ref(inp, weight=weight), head.autograd(inp, torch.float32, weight=weight)
    return inp, ref, yard, Y.own_error(lambda order: head.autograd(inp, torch.float32, weight=weight, perm=order), ref, B, perms)[0]


def min32(a, b):
    """The twin heads' smaller of two float32 arrays as the header writes it: a where a < b or a is a NaN, else b."""
    return np.where((a < b) | (a != a), a, b)


def target32(gamma, done, value, rew):
    """y = fmaf(gamma, done ? 0 : value, rew) in float32 (the fmaf through float64: its product is exact there)."""
    qn = np.where(done != 0, np.float32(0.0), value)
    return (np.float64(np.float32(gamma)) * qn.astype(np.float64) + rew.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the reference optimiser step
def net_of(arrays, like, dtype):
    """A StackedActor of `like`'s shape on the CPU in `dtype` holding the ten arrays."""
    net = R._new(like.n_actors, like.obs_len, like.n_actions, dtype=dtype)
    with torch.no_grad():
        for p, x in zip(PARAMS, arrays):
            getattr(net, p).copy_(torch.as_tensor(np.asarray(x)).to(dtype))
    return net


def first_step(nets, grads, targets, lr, kw, dtype, loose=(), clip=True):
    """ONE first Adam step from zero moments over every network of `nets` and every loose tensor (one clip norm over all of them; none
    with clip=False), then the Polyak line of the networks that have a target.  nets, targets: CPU StackedActors (a target may be None);
    grads: {tensor: array} per network; loose: (tensor, gradient array) pairs such as log_std; kw: betas, eps, max_grad_norm, tau.
    float64: adam_mlp_util.reference_step; float32: as a torch user takes it -- clip_grad_norm_, torch.optim.Adam, target.mul_(1 -
    tau).add_(p, alpha=tau) (adam_case_util.TorchPath's composition).
    -> per network dict(p, m, v, target: lists of ten arrays (no target without one); net: the stepped network in `dtype`), then per
    loose tensor dict(p, m, v: one-element lists); in float64 each also has the call's norm and coef."""
    hp = AU.hyper32(lr, *kw["betas"], kw["eps"], (kw["max_grad_norm"] or 0.0) if clip else 0.0)
    tau = float(np.float32(kw["tau"]))
    P0 = [getattr(n, p) for n in nets for p in PARAMS] + [t for t, _ in loose]
    G = [g[p] for g in grads for p in PARAMS] + [g for _, g in loose]
    T0 = [None if t is None else getattr(t, p) for t in targets for p in PARAMS] + [None] * len(loose)
    if dtype == torch.float64:
        num = lambda xs: [None if x is None else x.detach().cpu().numpy().copy() for x in xs]      # noqa: E731
        Z = [np.zeros(x.shape) for x in P0]
        P, M_, V, T, _, norm, coef = AM.reference_step(num(P0), G, Z, Z, num(T0), 0, hp, tau)
        more = dict(norm=norm, coef=coef)
    else:
        ps = [p.detach().clone().float().requires_grad_() for p in P0]
        ts = [None if t is None else t.detach().clone().float() for t in T0]
        for p, g in zip(ps, G):
            p.grad = torch.from_numpy(np.ascontiguousarray(g)).float()
        if hp["max_grad_norm"] > 0.0:
            torch.nn.utils.clip_grad_norm_(ps, hp["max_grad_norm"])
        opt = torch.optim.Adam(ps, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
        opt.step()
        with torch.no_grad():
            for t, p in zip(ts, ps):
                if t is not None:
                    t.mul_(1.0 - tau).add_(p, alpha=tau)
        f = lambda xs: [None if x is None else x.detach().numpy() for x in xs]               # noqa: E731
        P, M_, V, T, more = f(ps), f([opt.state[p]["exp_avg"] for p in ps]), f([opt.state[p]["exp_avg_sq"] for p in ps]), f(ts), {}
    out = []
    for i, (n, t) in enumerate(zip(nets, targets)):
        cut = slice(10 * i, 10 * i + 10)
        out.append(dict(p=P[cut], m=M_[cut], v=V[cut], net=net_of(P[cut], n, dtype), **({} if t is None else dict(target=T[cut])), **more))
    return out + [dict(p=[P[i]], m=[M_[i]], v=[V[i]], **more) for i in range(10 * len(nets), len(P0))]


# ------------------------------------------------------------------------------------------------ the kink filter's fixed point
def kink_fixed_point(w, update, near, max_rounds=MAX_ROUNDS):
    """The row weights of a whole-update case: zeroing a row moves the gradients and so the stepped networks, so the filter is repeated
    until no row that still has a weight lies near a kink.  w: the starting weights [B, nA]; update(w) -> the float64 reference;
    near(ref) -> bool [B, nA] -> (ref, w, rounds: the zeroing rounds it took); ref is None where the filter has not closed within
    max_rounds (w and rounds say how far it got)."""
    w, rounds = w.clone(), 0
    while True:
        ref = update(w)
        hit = near(ref) & (w != 0)
        if not hit.any():
            return ref, w, rounds
        rounds += 1
        if rounds > max_rounds:
            return None, w, rounds
        w[hit] = 0.0


def distances(wrong, ref, yard, names):
    """({tensor: mean |wrong - ref|}, {tensor: the yardstick's mean error}) over `names`: what a misreading's sharpness is read from."""
    dist = lambda a, b: {p: float(np.abs(a[p] - b[p]).mean()) for p in names}       # noqa: E731
    return dist(wrong, ref), dist(yard, ref)


# ------------------------------------------------------------------------------------------------ rings and batches
def ring(rows, B, seed=3, device="cuda", prioritized=False):
    """A DeviceReplayBuffer (prioritized: a PrioritizedReplayBuffer) of len(rows) transitions filled through _put with `rows` (obs, act,
    rew, obs_next, done), batches of B."""
    from deep_rl_battlespace_amd import replay
    obs, act, rew, obs_next, done = (r.to(device) for r in rows)
    N, nA, Do = obs.shape
    buf = (replay.PrioritizedReplayBuffer if prioritized else replay.DeviceReplayBuffer)(N, B, list(range(nA)), Do, Do * nA, act.shape[2],
                                                                                        device=device, seed=seed)
    buf._put(obs, act, rew, obs_next, done)
    return buf


def batch_of(s):
    """A ring's sample as the batch the learners read: (obs, act [B, nA, .], rew, obs_next [B, nA, Do], done)."""
    return s[0].transpose(0, 1), s[2].transpose(0, 1), s[3], s[4].transpose(0, 1), s[6]


# ------------------------------------------------------------------------------------------------ one update by hand
class Hand:
    """What a learner holds, under the same names, and the parts of its update that DDPG, TD3 and SAC share, written out with the public
    primitives alone: the ring's sample(), bsx_mlp_forward, ddpg_put_actions, mlp_grad (its padded copy of grad_out included),
    ddpg_action_grad, mlp_adam_step.  critic2: a second critic with its target, blobs and moments (TD3, SAC)."""

    def __init__(self, buffer, actor, critic, central, critic2=None, gamma=GAMMA, tau=0.01, lr_actor=1e-3, lr_critic=1e-3, max_grad_norm=None,
                 updates=1, betas=(0.9, 0.999), eps=1e-8):
        from deep_rl_battlespace_amd import learner as L
        self.buffer, self.central, self.gamma, self.updates = buffer, bool(central), gamma, updates
        self.prioritized = hasattr(buffer, "tree")
        for name, sfx, net in (("actor", "a", actor), ("critic", "c", critic), ("critic2", "c2", critic2)):
            if net is None:
                continue
            target = copy.deepcopy(net)
            target.__dict__.pop("_bsx_mlp_buffers", None)
            for attr, value in ((name, net), ("target_" + name, target), ("_blob_" + sfx, net.pack()), ("_blob_t" + sfx, target.pack()),
                                ("adam_" + name, L.AdamState(net))):
                setattr(self, attr, value)
        dev = actor.w1.device
        self.hyper_actor = L.adam_hyper(lr_actor, betas, eps, max_grad_norm, dev, tau)
        self.hyper_critic = L.adam_hyper(lr_critic, betas, eps, max_grad_norm, dev, tau)
        self.step_actor, self.step_critic = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        self.stats = torch.zeros((updates, 8), dtype=torch.float64, device=dev)
        self.step_stats_actor, self.step_stats_critic = (torch.zeros((updates, 4), dtype=torch.float64, device=dev) for _ in range(2))

    def update(self, stop_after=None):
        for u in range(self.updates if stop_after is None else stop_after):
            self.step(*batch_of(self.buffer.sample()), u, **self.step_args(u))
        return self.stats

    def step_args(self, u):
        """What update() passes to step() beside the batch and u."""
        return dict(weight=self.buffer.weights if self.prioritized else None)

    def forward(self, blob, x, raw=False):
        """bsx_mlp_forward of the network packed in `blob` on x [B, nA, D] -> y4 [B, nA, 4], or with raw the unsquashed first output [B, nA]."""
        from deep_rl_battlespace_amd import _lib
        (B, nA, D), dev = x.shape, x.device
        y4 = torch.empty((B, nA, 4), device=dev)
        r = torch.empty((B, nA), device=dev) if raw else None
        _lib.check(_lib.load().bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y4.data_ptr(), r.data_ptr() if raw else None, B, nA, D,
                                               torch.cuda.current_stream(dev).cuda_stream), "bsx_mlp_forward")
        return r if raw else y4

    def _twin(self, fmt, n):
        return [getattr(self, fmt + s) for s in ("", "2")[:n]]

    def critic_rows(self, x_cur, seeds):
        """Each critic's gradient row at x_cur from its head seed [B, nA, 4] -> copies of mlp_grad's cached rows."""
        from deep_rl_battlespace_amd import learner as L
        return [L.mlp_grad(c, blob, x_cur, g[..., :1].contiguous(), squash=False, input_grad=False)[0].clone()
                for c, blob, g in zip(self._twin("critic", len(seeds)), self._twin("_blob_c", len(seeds)), seeds)]

    def critics_step(self, rows, u, targets=True):
        """ONE mlp_adam_step over the critics the rows belong to, with their Polyak targets unless targets=False."""
        from deep_rl_battlespace_amd import learner as L
        n = len(rows)
        polyak = dict(targets=self._twin("target_critic", n), target_blobs=self._twin("_blob_tc", n)) if targets else {}
        L.mlp_adam_step(self._twin("critic", n), rows, self._twin("adam_critic", n), self._twin("_blob_c", n), self.hyper_critic, self.step_critic,
                        stats=self.step_stats_critic[u], **polyak)

    def actor_row(self, obs, g_a4, k):
        from deep_rl_battlespace_amd import learner as L
        return L.mlp_grad(self.actor, self._blob_a, obs, g_a4[..., :k].contiguous(), squash=True, input_grad=False)[0].clone()

    def deterministic_actor_step(self, obs, x_pi, g_pi, k, u, adam=True):
        """DDPG's and TD3's actor: pi(o) into its own slot of x_pi, critic 1's input gradient there from the head's g_pi, the actor's row
        from its own action columns and, with adam, its step with its Polyak target -> the row."""
        from deep_rl_battlespace_amd import learner as L
        Do, c = obs.shape[2], self.central
        L.ddpg_put_actions(self.forward(self._blob_a, obs), x_pi, Do, k, central=c, own_only=True)
        _, gx = L.mlp_grad(self.critic, self._blob_c, x_pi, g_pi[..., :1].contiguous(), squash=False, input_grad=True)
        row_a = self.actor_row(obs, L.ddpg_action_grad(gx, Do, k, central=c), k)
        if adam:
            L.mlp_adam_step([self.actor], [row_a], [self.adam_actor], [self._blob_a], self.hyper_actor, self.step_actor,
                            targets=[self.target_actor], target_blobs=[self._blob_ta], stats=self.step_stats_actor[u])
        return row_a


# ------------------------------------------------------------------------------------------------ the bandit
BANDIT = dict(nA=2, Do=5, k=4, rows=2048, B=256, held_out=1024, lr=1e-3, tau=0.01)


def bandit_reward(obs, a):
    """r = -mean_k (a_k - 0.5 sign(o_k))^2 over the k action columns, against the first k observation columns -> [.., nA]."""
    return -((a - 0.5 * torch.sign(obs[..., :a.shape[-1]])) ** 2).mean(-1)


def bandit_rows(seed=0, b=BANDIT):
    """The bandit ring (every row finished: done = 1, the next observation plays no part) and a held-out observation set."""
    g = torch.Generator().manual_seed(9900 + seed)
    uni = lambda *s: torch.rand(s, generator=g) * 2 - 1       # noqa: E731
    obs, act = uni(b["rows"], b["nA"], b["Do"]), uni(b["rows"], b["nA"], b["k"])
    rows = (obs, act, bandit_reward(obs, act), uni(b["rows"], b["nA"], b["Do"]), torch.ones((b["rows"], b["nA"]), dtype=torch.bool))
    return rows, uni(b["held_out"], b["nA"], b["Do"])


def bandit_nets(seed=0, b=BANDIT, critic2=None):
    """(actor, critic) on the CPU, freshly initialised (own critics: Do + k -> 1), and a second critic: critic2="next" drawn right after
    the first, critic2="reseeded" at a seed of its own."""
    torch.manual_seed(9950 + seed)
    nets = [R._new(b["nA"], b["Do"], b["k"]), R._new(b["nA"], b["Do"] + b["k"], 1)]
    if critic2 == "reseeded":
        torch.manual_seed(9960 + seed)
    return tuple(nets + [R._new(b["nA"], b["Do"] + b["k"], 1)] if critic2 else nets)


def bandit_torch_run(N, compose, seed=0, b=BANDIT):
    """(initial reward, reward after N updates) of a torch composition on the CPU, batches drawn with a torch generator.  compose(seed) ->
    (the actor, update(u, batch, generator)): the composition's networks and one update of it."""
    rows, held = bandit_rows(seed, b)
    actor, update = compose(seed)
    g = torch.Generator().manual_seed(9990 + seed)
    with torch.no_grad():
        r0 = float(bandit_reward(held, actor(held)).mean())
    for u in range(N):
        idx = torch.randint(0, b["rows"], (b["B"],), generator=g)
        update(u, tuple(r[idx] for r in rows), g)
    with torch.no_grad():
        return r0, float(bandit_reward(held, actor(held)).mean())


def polyak_(targets, nets, tau):
    """The foreach Polyak lines of a torch composition."""
    with torch.no_grad():
        for t, n in zip(targets, nets):
            ts, ns = list(t.parameters()), list(n.parameters())
            torch._foreach_mul_(ts, 1.0 - tau)
            torch._foreach_add_(ts, ns, alpha=tau)


def bandit_learner_reward(make, nets, N, b=BANDIT):
    """(the captured learner, the held-out reward of its actor after N updates in calls of 10).  make(ring, *nets on the GPU) -> a learner."""
    rows, held = bandit_rows(b=b)
    learner = make(ring(rows, b["B"]), *(gpu_copy(n) for n in nets)).capture()
    assert N % 10 == 0
    for _ in range(N // 10):
        learner.update()
    with torch.no_grad():
        return learner, float(bandit_reward(held, learner.actor(held.cuda()).cpu()).mean())


def bandit_test(profile, torch_run, make, nets, what, b=BANDIT):
    """The learning check's body: N from the profile's bandit section; the torch composition re-run on the CPU closes at least half of
    the gap from its initial reward to 0; N captured updates of make(ring, *nets) close at least half of what it closes.  Prints the
    figures -> (the learner, N, the profile's section)."""
    rec = json.load(open(profile))["bandit"]
    N = rec["N"]
    r0, r_torch = torch_run(N)
    closed_torch = (r_torch - r0) / (0.0 - r0)
    assert abs(r0 - rec["initial_reward"]) < 1e-6 and closed_torch >= 0.5
    learner, after = bandit_learner_reward(make, nets, N, b)
    with torch.no_grad():
        held = bandit_rows(b=b)[1]
        before = float(bandit_reward(held, nets[0](held)).mean())
    closed = (after - before) / (0.0 - before)
    print(f"bandit, N = {N}: reward {before:.4f} -> {after:.4f} (closed {closed:.3f} of the gap); {what} -> {r_torch:.4f} "
          f"(closed {closed_torch:.3f}; recorded {rec['torch_closed']:.3f})")
    assert abs(before - r0) < 1e-6
    assert closed >= 0.5 * closed_torch
    return learner, N, rec


# ------------------------------------------------------------------------------------------------ the learner suites
def differing(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def step_arrays(x, which):
    """dict(p, m, v, target) of lists of ten numpy arrays: x's network `which` ("actor" / "critic" / "critic2"), its moments and its target."""
    net, state = getattr(x, which), getattr(x, "adam_" + which)
    cut = lambda row: AU.row_to_tensors(row.detach().cpu().numpy(), net.n_actions)     # noqa: E731
    return dict(p=AU.net_arrays(net), m=cut(state.m), v=cut(state.v), target=AU.net_arrays(getattr(x, "target_" + which)))


def grad_arrays(row, n_actions):
    """A gradient row of the device as {tensor: float64 array}."""
    from deep_rl_battlespace_amd.learner import split_grad
    return {p: g.double().cpu().numpy() for p, g in zip(PARAMS, split_grad(row, n_actions))}


def append_ratios(env, sid, rec):
    """Appends a whole-update test's measured ratios to the file the environment variable `env` names, if it names one."""
    path = os.environ.get(env)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"shape": sid, "ratios": rec}) + "\n")


def capture_runs_nothing(captured, snapshot):
    start = snapshot(captured)
    assert captured.capture() is captured
    assert differing(start, snapshot(captured)) == []


def replays_the_eager_updates(captured, eager, snapshot, calls, each=lambda u: None):
    """`calls` updates of the captured learner and of its eager twin leave the same bits after each; each(u) runs between the updates
    and the comparison."""
    for u in range(calls):
        captured.update()
        eager.update()
        each(u)
        a, b = snapshot(captured), snapshot(eager)
        assert differing(a, b) == [], (u, differing(a, b))


def allocates_nothing(captured):
    """Two more replays leave the bytes in use as they were."""
    torch.cuda.synchronize()
    gc.collect()                                                              # (as ppo_learner_util.allocates_nothing reads it)
    held = torch.cuda.memory_allocated()
    captured.update()
    captured.update()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held


class Suite:
    """What a learner's GPU suite builds its cases from.  learner: the class's name in deep_rl_battlespace_amd.learner; hand: its Hand;
    case(shape, seed) -> (actor, critic, ring rows, ...) on the CPU (ddpg_util.learner_case); critic2(shape, seed): the second critic
    of the twin learners; defaults: the keyword arguments every learner and Hand of the suite gets."""

    def __init__(self, learner, hand, case, defaults, critic2=None):
        self.learner_name, self.Hand, self.case, self.defaults, self.critic2 = learner, hand, case, defaults, critic2

    @staticmethod
    def central(shape):
        return "central" if shape[4] else "own"

    def nets(self, shape, seed=0):
        """(the shape's starting networks on the GPU: fresh copies, the rows of its ring)."""
        actor, critic, rows, *_ = self.case(shape, seed)
        second = (self.critic2(shape, seed),) if self.critic2 else ()
        return tuple(gpu_copy(n) for n in (actor, critic) + second), rows

    def learner(self, shape, prioritized=False, rows=None, seed=0, nets=None, **kw):
        from deep_rl_battlespace_amd import learner as L
        made, case_rows = self.nets(shape, seed)
        return getattr(L, self.learner_name)(ring(case_rows if rows is None else rows, shape[0], prioritized=prioritized), *(nets or made),
                                             critic_input=self.central(shape), **{**self.defaults, **kw})

    def hand(self, shape, prioritized=False, rows=None, seed=0, **kw):
        made, case_rows = self.nets(shape, seed)
        actor, critic, *second = made
        return self.Hand(ring(case_rows if rows is None else rows, shape[0], prioritized=prioritized), actor, critic, *second, shape[4],
                         **{**self.defaults, **kw})


def set_targets(x, targets, sync=False):
    """Target networks into x's (a Hand or a learner) and their blobs: re-packed in place, or through x.sync().  targets: {"actor" /
    "critic" / "critic2": the network whose parameters x's target of that name takes}."""
    blobs = dict(actor="_blob_ta", critic="_blob_tc", critic2="_blob_tc2")
    with torch.no_grad():
        for name, src in targets.items():
            t = getattr(x, "target_" + name)
            for p in PARAMS:
                getattr(t, p).copy_(getattr(src, p))
            if not sync:
                t.pack(out=getattr(x, blobs[name]))
    if sync:
        x.sync()


def blobs_are_packs(x):
    """Every blob x holds is the pack of the network it stands for (the second critic's where x has one)."""
    pairs = [(x.actor, x._blob_a), (x.critic, x._blob_c), (x.target_actor, x._blob_ta), (x.target_critic, x._blob_tc)]
    if hasattr(x, "critic2"):
        pairs += [(x.critic2, x._blob_c2), (x.target_critic2, x._blob_tc2)]
    for net, blob in pairs:
        assert torch.equal(net.pack().view(torch.int32), blob.view(torch.int32))


def sample_is(hand, idx, batch):
    """The ring sampled at fixed idx -> the batch on the device, which is `batch` (CPU) bit for bit."""
    dev_batch = batch_of(hand.buffer.sample(idx))
    for got, want in zip(dev_batch, batch):
        assert torch.equal(got.cpu(), want)
    return dev_batch


# ------------------------------------------------------------------------------------------------ the head suites
SENTINEL = np.int32(0x7FC0BEEF)           # a NaN with a payload: no arithmetic produces it
NORMAL_TOL = 1e-5                         # |z - z64| <= NORMAL_TOL * (1 + |z64|), tests/test_hip_gaussian_head.py's rule
NAN = float("nan")


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def same_bits(a, b):
    return all(x is None and y is None or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def numpy_of(res, names):
    return dict({k: getattr(res, k).double().cpu().numpy() for k in names}, stats=res.stats.cpu().numpy())


def put(G, inp):
    """{name: a buffer of G holding the CPU tensor}."""
    dev = {}
    for k, v in inp.items():
        dev[k] = G(k, tuple(v.shape), v.dtype)
        dev[k].copy_(v)
    return dev


def guarded_head(head, inp, weight=True, gamma=GAMMA, guarded=False, fill=7.0, td=True):
    """The head's binding on `inp` with every input, output and the workspace between guard slabs (guarded) and every output float
    starting as `fill` -> (the binding's result: the `out` tensors themselves, the strays).  td=False: without the optional td."""
    from deep_rl_battlespace_amd import learner as L
    from guard_util import Buffers
    B, nA = inp[head.qs[0]].shape
    G = Buffers(guarded)
    dev = put(G, inp)
    out = tuple(G(k, (B, nA, 4), torch.float32, init=fill) for k in head.grads) + \
        (G("td", (B, nA), torch.float32, init=fill) if td else None, G("stats", (8,), torch.float64, init=fill))
    ws = G("workspace", (getattr(L, head.entry + "_workspace_bytes")(B, nA) // 8,), torch.int64, init=-1)
    res = getattr(L, head.entry)(*(gamma if k == "gamma" else dev[k] for k in head.args), weight=dev["weight"] if weight else None, out=out,
                                 workspace=ws)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(res, out))
    return res, G.stray()


def sentinel_x(G, shape, width, name="x"):
    """A critic input [B, nA, width] of G whose every float is SENTINEL."""
    x = G(name, (shape[0], shape[1], width), torch.float32)
    x.view(torch.int32).fill_(int(SENTINEL))
    return x


# ------------------------------------------------------------------------------------------------ the measuring tools
CANDIDATES = (50, 100, 200, 400, 800)


def bandit_section(old, torch_run, learner_reward, config):
    """A profile's bandit section.  N is chosen with the torch composition alone: the smallest of CANDIDATES from which on it closes at
    least 60 % of the gap from its initial held-out reward to 0 (the tests ask half).  torch_run(N) -> (initial reward, reward);
    learner_reward(N): what N captured updates of the learner reach, run with a GPU -- without one the figures of an earlier GPU run at
    the same N are kept from `old`, the file's present content."""
    runs = {N: torch_run(N) for N in CANDIDATES}
    closed = {N: (r1 - r0) / (0.0 - r0) for N, (r0, r1) in runs.items()}
    N = next(n for n in CANDIDATES if all(closed[m] >= 0.6 for m in CANDIDATES if m >= n))
    r0, r1 = runs[N]
    bandit = dict(config, N=N, initial_reward=r0, torch_reward=r1, torch_closed=closed[N],
                  torch_closed_by_candidate={str(n): closed[n] for n in CANDIDATES})
    if torch.cuda.is_available():
        r = learner_reward(N)
        bandit.update(learner_reward=r, learner_closed=(r - r0) / (0.0 - r0))
    elif old.get("bandit", {}).get("N") == N:
        bandit.update({k: old["bandit"][k] for k in ("learner_reward", "learner_closed") if k in old["bandit"]})
    return bandit


def rounded(spread, digits=4):
    return {k: [round(float(x), digits) for x in v] for k, v in spread.items()}


def head_sections(head, shapes):
    """(head_spread, factors) of a twin head's profile: per case the yardstick's own spread and the exceptions the rule makes of it."""
    spread = {head_id(B, nA, w): rounded(head.spread(B, nA, w)) for B, nA in shapes for w in (True, False)}
    return spread, Y.exceptions_from(spread)


def sharpness(variants):
    """{misreading: its smallest distance from the reference over the tensors compared, in yardstick mean errors, rounded}."""
    return {name: round(min(dist[p] / yard[p] for p in dist)) for name, (dist, yard) in variants.items()}


def kept_kernel(old, argv=None):
    """The `kernel` part of a stepped section: the old file's, with the JSON lines of a --ratios FILE (what the GPU test appended) over it."""
    argv = sys.argv if argv is None else argv
    kernel = dict(old.get("stepped", {}).get("kernel", {}))
    if "--ratios" in argv:
        for line in open(argv[argv.index("--ratios") + 1]):
            rec = json.loads(line)
            kernel[rec["shape"]] = rec["ratios"]
    return kernel
