"""What the tests of the free-width optimiser step with Polyak targets (learner.mlp_adam_step, bsx_adam_step_mlp) share, on top of
tests/adam_util.py:

  SHAPES             the (A, D, n_actions) of the issue: the smallest, an odd A at the 1v1 critic's width, the 2v2 critic, the first width
                     beyond the old LDS bound (odd D, pad columns), the widest row (8 full strides of 1024 and a ragged ninth) and the
                     widest call (32 agents x 2 networks + log_std = 65 partials)
  polyak             the contract's Polyak line restated in float64: t = (1 - tau) t + tau p, tau the float32 value the device reads
  reference_step     adam_util.reference_step followed by polyak on the networks that have a target
  Case               one or two networks with their targets, Adam state, blobs, target blobs, log_std, hyper, counter, stats and workspace
                     on the GPU (through a guard_util.Buffers if given), run through mlp_adam_step
  TorchPath          torch's own float32 clip_grad_norm_ + Adam + target.mul_(1 - tau).add_(p, alpha=tau): the yardstick
"""
import numpy as np
import torch

import adam_util as U
import guard_util as GU

#          id             A   D  n_actions  second network (1 column) and log_std
SHAPES = {"a1-d1": (1, 1, 1, False), "a3-d9": (3, 9, 1, False), "a4-d24": (4, 24, 1, False), "a5-d51-na3": (5, 51, 3, False),
          "a2-d64-na4": (2, 64, 4, False), "a32-d64-two-nets-log-std": (32, 64, 1, True)}
TAU = float(np.float32(0.01))


def blob_floats(D):
    """Floats per agent of StackedActor.pack() at any width: W1A over D rounded up to even, and 10 884 more."""
    return 64 * (D + D % 2) + 10884


def polyak(targets, params, tau):
    """t = (1 - tau) t + tau p in float64 over two lists of arrays -> new arrays.  tau: a float32-representable Python float."""
    return [(1.0 - tau) * np.asarray(t, np.float64) + tau * np.asarray(p, np.float64) for t, p in zip(targets, params)]


def reference_step(params, grads, m, v, targets, t, hp, tau):
    """adam_util.reference_step over everything in the call, then the Polyak line.  targets: a list as long as params with None where
    a tensor has no target (a network without one, log_std) -> (params, m, v, targets, t + 1, norm, coef)."""
    P, M, V, t, norm, coef = U.reference_step(params, grads, m, v, t, hp)
    T = [None if x is None else polyak([x], [p], tau)[0] for x, p in zip(targets, P)]
    return P, M, V, T, t, norm, coef


def clone_net(net, device=None):
    """A StackedActor with the bits of `net`'s parameters, on `device` (default: net's)."""
    from deep_rl_battlespace_amd.rollout import StackedActor
    out = StackedActor(net.n_actors, net.obs_len, net.n_actions, device=device or net.w1.device)
    with torch.no_grad():
        for k in U.PARAMS:
            getattr(out, k).copy_(getattr(net, k).detach())
    return out


class Case:
    """nas: n_actions per network (one or two); targets: per network whether it has one; with_ls: the Gaussian head's log_std rides along.
    alloc: a guard_util.Buffers -- every buffer the step writes is then a view between guard bytes."""

    def __init__(self, A, D, nas, hp, tau=TAU, with_ls=False, targets=None, seed=0, alloc=None, group=1):
        from deep_rl_battlespace_amd import learner
        from deep_rl_battlespace_amd.rollout import StackedActor
        self.A, self.D, self.group = A, D, group
        alloc = alloc or GU.Buffers(False)
        targets = [True] * len(nas) if targets is None else list(targets)
        torch.manual_seed(300 + seed)
        self.nets = [StackedActor(A, D, na, device="cuda") for na in nas]
        self.targets = [StackedActor(A, D, na, device="cuda") if on else None for na, on in zip(nas, targets)]
        self.states, self.blobs, self.target_blobs = [], [], []
        for i, (net, tgt) in enumerate(zip(self.nets, self.targets)):
            for name, x in ((f"net{i}", net), (f"target{i}", tgt)):
                if x is None:
                    continue
                for k in U.PARAMS:                                          # the parameters as views of the allocator's buffers
                    p = getattr(x, k)
                    buf = alloc(f"{name}.{k}", p.shape, torch.float32)
                    buf.copy_(p.detach())
                    setattr(x, k, torch.nn.Parameter(buf))
            st = learner.AdamState(net)
            st.m, st.v = alloc(f"net{i}.m", st.m.shape, torch.float32), alloc(f"net{i}.v", st.v.shape, torch.float32)
            self.states.append(st)
            self.blobs.append(alloc(f"net{i}.blob", (A, blob_floats(D)), torch.float32, init=-7.25))
            self.target_blobs.append(alloc(f"target{i}.blob", (A, blob_floats(D)), torch.float32, init=-3.5) if tgt is not None else None)
        self.log_std = self.ls_state = None
        if with_ls:
            self.log_std = alloc("log_std", (A, 3), torch.float32, init=-0.5)
            self.ls_state = learner.AdamState(self.log_std)
            self.ls_state.m, self.ls_state.v = alloc("ls.m", (A, 3), torch.float32), alloc("ls.v", (A, 3), torch.float32)
        self.set_hyper(hp, tau)
        self.step = alloc("step", (1,), torch.int64)
        self.stats = alloc("stats", (4,), torch.float64, init=-1)
        nb = learner.mlp_adam_step_workspace_bytes(A, len(self.nets))
        self.ws = alloc("ws", ((nb + 7) // 8,), torch.int64)

    def set_hyper(self, hp, tau):
        from deep_rl_battlespace_amd import learner
        self.hyper = learner.adam_hyper(hp["lr"], (hp["beta1"], hp["beta2"]), hp["eps"], hp["max_grad_norm"], tau=tau)

    def tie(self):
        """Everything of the case tied in its group, as a learner with shared parameters starts."""
        from deep_rl_battlespace_amd import learner
        for x in self.nets + [t for t in self.targets if t is not None] + self.states + ([self.log_std, self.ls_state] if self.log_std is not None else []):
            for t in learner._tied_tensors(x):
                v = t.detach().view(self.A // self.group, self.group, *t.shape[1:])
                v.copy_(v[:, :1].clone().expand_as(v))

    def draw(self, gen, scale=1.0):
        rows = [U.random_rows(self.A, self.D, net.n_actions, gen, scale).cuda() for net in self.nets]
        g_ls = (scale * torch.randn((self.A, 3), generator=gen)).cuda() if self.log_std is not None else None
        return rows, g_ls

    def zeros(self):
        return [torch.zeros_like(st.m) for st in self.states], (torch.zeros_like(self.log_std) if self.log_std is not None else None)

    def run(self, rows, g_ls, with_targets=True, group=None):
        from deep_rl_battlespace_amd import learner
        kw = dict(targets=self.targets, target_blobs=self.target_blobs) if with_targets and any(t is not None for t in self.targets) else {}
        return learner.mlp_adam_step(self.nets, rows, self.states, self.blobs, self.hyper, self.step, log_std=self.log_std, g_log_std=g_ls,
                                     log_std_state=self.ls_state, stats=self.stats, workspace=self.ws,
                                     group=self.group if group is None else group, **kw)

    def tensors(self):
        """Everything the step writes, by name."""
        out = {"step": self.step, "stats": self.stats}
        for i, (net, st, blob, tgt, tb) in enumerate(zip(self.nets, self.states, self.blobs, self.targets, self.target_blobs)):
            out.update({f"net{i}.{k}": getattr(net, k).detach() for k in U.PARAMS})
            out.update({f"net{i}.m": st.m, f"net{i}.v": st.v, f"net{i}.blob": blob})
            if tgt is not None:
                out.update({f"target{i}.{k}": getattr(tgt, k).detach() for k in U.PARAMS})
                out[f"target{i}.blob"] = tb
        if self.log_std is not None:
            out.update({"log_std": self.log_std, "ls.m": self.ls_state.m, "ls.v": self.ls_state.v})
        return out

    def bits(self):
        torch.cuda.synchronize()
        return {k: v.clone().view(torch.int32 if v.element_size() == 4 else torch.int64) for k, v in self.tensors().items()}

    def load(self, other):
        """Take every tensor's bits from another case of the same shape (targets the other lacks are left alone)."""
        mine, theirs = self.tensors(), other.tensors()
        with torch.no_grad():
            for k, v in mine.items():
                if k in theirs:
                    v.copy_(theirs[k])
        self.hyper = other.hyper.clone()

    def groups(self):
        """Per network (params, m, v, targets or None) as lists of numpy arrays in ten-tensor shapes; log_std rides with network 0 (its
        target entry is None)."""
        out = []
        for i, (net, st, tgt) in enumerate(zip(self.nets, self.states, self.targets)):
            P = U.net_arrays(net)
            M, V = U.row_to_tensors(st.m.cpu().numpy(), net.n_actions), U.row_to_tensors(st.v.cpu().numpy(), net.n_actions)
            T = U.net_arrays(tgt) if tgt is not None else [None] * 10
            if i == 0 and self.log_std is not None:
                P.append(self.log_std.cpu().numpy().copy()); M.append(self.ls_state.m.cpu().numpy().copy()); V.append(self.ls_state.v.cpu().numpy().copy())
                T.append(None)
            out.append((P, M, V, T))
        return out


def same_bits(a, b):
    """Names of the tensors whose bits differ between two Case.bits() (over the names both have)."""
    return [k for k in a if k in b and not torch.equal(a[k], b[k])]


def blobs_are_packs(case, where):
    """Every blob equals net.pack() and every target blob target.pack(), bit for bit."""
    pairs = [(f"net{i}", n, b) for i, (n, b) in enumerate(zip(case.nets, case.blobs))]
    pairs += [(f"target{i}", t, b) for i, (t, b) in enumerate(zip(case.targets, case.target_blobs)) if t is not None]
    for name, net, blob in pairs:
        want = net.pack()
        assert blob.shape == want.shape
        bad = (blob.view(torch.int32) != want.view(torch.int32)).nonzero()
        assert bad.numel() == 0, (where, name, bad[:4].tolist())


def flat_split(case, rows, g_ls):
    """The call's gradients as one list per network in ten-tensor shapes (torch, GPU), log_std's with network 0."""
    out = []
    for i, (net, row) in enumerate(zip(case.nets, rows)):
        g = U.row_to_tensors(row, net.n_actions)
        if i == 0 and g_ls is not None:
            g.append(g_ls.clone())
        out.append(g)
    return out


class TorchPath:
    """torch's float32 clip_grad_norm_ + Adam + target.mul_(1 - tau).add_(p, alpha=tau) on the GPU over copies of a case's parameters
    and targets: the yardstick."""

    def __init__(self, case, hp, tau, t0=0):
        self.hp, self.tau = hp, tau
        self.params, self.targets = [], []
        for i, (net, tgt) in enumerate(zip(case.nets, case.targets)):
            ps = [getattr(net, k).detach().clone().requires_grad_() for k in U.PARAMS]
            ts = [getattr(tgt, k).detach().clone() for k in U.PARAMS] if tgt is not None else [None] * 10
            if i == 0 and case.log_std is not None:
                ps.append(case.log_std.clone().requires_grad_())
                ts.append(None)
            self.params.append(ps)
            self.targets.append(ts)
        self.flat = [p for ps in self.params for p in ps]
        self.opt = torch.optim.Adam(self.flat, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
        for p in self.flat:
            self.opt.state[p] = dict(step=torch.tensor(float(t0)), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))

    def set_counter(self, t):
        for p in self.flat:
            self.opt.state[p]["step"].fill_(float(t))

    def step(self, grads):
        for ps, gs in zip(self.params, grads):
            for p, g in zip(ps, gs):
                p.grad = g.clone()
        if self.hp["max_grad_norm"] > 0.0:
            torch.nn.utils.clip_grad_norm_(self.flat, self.hp["max_grad_norm"])
        self.opt.step()
        with torch.no_grad():
            for ps, ts in zip(self.params, self.targets):
                for p, t in zip(ps, ts):
                    if t is not None:
                        t.mul_(1.0 - self.tau).add_(p, alpha=self.tau)

    def groups(self):
        f = lambda x: x.detach().cpu().numpy()     # noqa: E731
        return [([f(p) for p in ps], [f(self.opt.state[p]["exp_avg"]) for p in ps], [f(self.opt.state[p]["exp_avg_sq"]) for p in ps],
                 [None if t is None else f(t) for t in ts]) for ps, ts in zip(self.params, self.targets)]


def start(case):
    """The float64 restatement's state at a case's present values: per network [P, M, V, T]."""
    return [[[None if x is None else np.asarray(x, np.float64) for x in grp] for grp in g] for g in case.groups()]


def advance(ref, grads, t, hp, tau):
    """One step of the float64 restatement over everything in the call at once (one global norm), then the Polyak line; ref (per
    network [P, M, V, T]) is advanced in place -> (t + 1, norm, coef)."""
    sizes = [len(g) for g in grads]
    flat = lambda j: [x for grp in ref for x in grp[j]]     # noqa: E731
    P, M, V, T, t, norm, coef = reference_step(flat(0), [g.cpu().numpy() for gs in grads for g in gs], flat(1), flat(2), flat(3), t, hp, tau)
    o = 0
    for i, k in enumerate(sizes):
        ref[i] = [P[o:o + k], M[o:o + k], V[o:o + k], T[o:o + k]]
        o += k
    return t, norm, coef
