"""The GPU-side harness of the optimiser step's tests (learner.adam_step, learner.adam_step(group=), learner.mlp_adam_step: one body,
learner.adam._adam_step, and one kernel path, bsx_adam_step_mlp).  tests/test_hip_adam_step.py, test_hip_adam_shared.py, test_hip_adam_mlp.py
and tools/measure_adam_mlp.py build on it; the float64 arithmetic stays on the host side, in adam_util.py, shared_step_util.py and
adam_mlp_util.py.

  Case               one or two networks as views of a guard_util.Buffers' buffers, optional Polyak targets, Adam state, blobs, target
                     blobs, log_std, hyper, counter, stats and workspace on the GPU, stepped through adam_step or mlp_adam_step
  TorchPath          torch's own float32 clip_grad_norm_ + Adam (+ target.mul_(1 - tau).add_(p, alpha=tau)) over one parameter per tied
                     group: the yardstick
  start / advance    the float64 restatement's state at a case's present values, and one step of it over everything in the call
  meets_the_bars     the bars every suite holds the step to: pooled mean |error| against the restatement at most 2x torch's, maximum at
                     most 4x; record prints the ratios and appends them to a file on request
  check_stats        the exact step, norm and coefficient within 1e-10 relative, the float32 lr
  same_bits / blobs_are_packs / members_equal_their_leader / flat_split / first_norm / clone_net   what the tests compare and draw with
  LEGS, STEPS        the five-step tests' three legs
"""
import json
import os

import numpy as np
import torch

import actor_ref_util as R
import adam_mlp_util as MU
import adam_util as U
import guard_util as GU
import shared_step_util as S
import yardstick_util as Y

STEPS = 5
#       leg                lr     counter set to (before step index)   what it shows
LEGS = {"lr3e-4-from-0": (3e-4, {}),                                 # the usual start: bias corrections far from 1
        "counter-1000-after-3": (3e-4, {3: 1000}),                   # ... and then near 1: b^t through a large t
        "lr0.05-counter-1000": (0.05, {0: 1000})}                    # a parameter-sized step: the step's own arithmetic shows

AGENT_AXIS = lambda k: k not in ("step", "stats")     # noqa: E731     (a name of Case.tensors(): all but these two have the agent axis)


def clone_net(net, device=None):
    """A StackedActor with the bits of `net`'s parameters, on `device` (default: net's)."""
    return R.to(net, device or net.w1.device)


class Case:
    """A agents, D inputs; nas: n_actions per network (one or two); with_ls: the Gaussian head's log_std rides along; targets: per network
    whether it has a Polyak target (default: every network with entry "mlp", none with "adam", which takes none); tau: the rate in
    hyper (default adam_mlp_util.TAU with "mlp" and adam_hyper's own 0 with "adam", which does not read it).
    entry: what run() calls -- "adam": learner.adam_step at an actor's shape (A = 2n, D = 3n + 2), "mlp": learner.mlp_adam_step.
    group: the agents per tied group run() passes.  tied: the case starts as a learner with shared parameters does -- networks, a
    per-agent log_std (-0.5 + 0.1 randn) and states tied with learner.tie_; without it log_std is -0.5 everywhere and nothing is tied
    (tie() ties later, at any A).  seed: torch.manual_seed's, drawn from in this order: the networks, the targets, a tied log_std.
    alloc: a guard_util.Buffers -- every buffer the step writes is then a view between guard bytes.  Blobs and target blobs start
    from a non-zero pattern."""

    def __init__(self, A, D, nas, hp, *, tau=None, with_ls=False, targets=None, group=1, tied=False, seed, alloc=None, entry="mlp"):
        from deep_rl_battlespace_amd import learner
        from deep_rl_battlespace_amd.rollout import StackedActor
        assert entry in ("adam", "mlp"), entry
        mlp = entry == "mlp"
        self.A, self.D, self.n, self.group, self.entry = A, D, A // 2, group, entry
        self.tau = (MU.TAU if mlp else 0.0) if tau is None else tau
        alloc = alloc or GU.Buffers(False)
        targets = [mlp] * len(nas) if targets is None else list(targets)
        actor_shape = A == 2 * self.n and D == 3 * self.n + 2
        assert mlp or (actor_shape and not any(targets)), (A, D, targets)
        nf = MU.blob_floats(D)
        if actor_shape and D <= 50:
            assert nf == learner.blob_floats(D), (D, nf, learner.blob_floats(D))
        torch.manual_seed(seed)
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
                    assert getattr(x, k).data_ptr() == buf.data_ptr()
            if tied:
                learner.tie_(net, group)
            st = learner.AdamState(net)
            st.m, st.v = alloc(f"net{i}.m", st.m.shape, torch.float32), alloc(f"net{i}.v", st.v.shape, torch.float32)
            self.states.append(learner.tie_(st, group) if tied else st)
            self.blobs.append(alloc(f"net{i}.blob", (A, nf), torch.float32, init=-7.25))
            self.target_blobs.append(alloc(f"target{i}.blob", (A, nf), torch.float32, init=-3.5) if tgt is not None else None)
        self.log_std = self.ls_state = None
        if with_ls:
            self.log_std = alloc("log_std", (A, 3), torch.float32, init=-0.5)
            if tied:
                self.log_std.copy_(-0.5 + 0.1 * torch.randn(A, 3, device="cuda"))
                learner.tie_(self.log_std, group)
            self.ls_state = learner.AdamState(self.log_std)
            self.ls_state.m, self.ls_state.v = alloc("ls.m", (A, 3), torch.float32), alloc("ls.v", (A, 3), torch.float32)
        self.set_hyper(hp)
        self.step = alloc("step", (1,), torch.int64)
        self.stats = alloc("stats", (4,), torch.float64, init=-1)
        nb = learner.mlp_adam_step_workspace_bytes(A, len(nas)) if mlp else learner.adam_step_workspace_bytes(self.n, len(nas))
        self.ws = alloc("ws", ((nb + 7) // 8,), torch.int64)

    def set_hyper(self, hp, tau=None):
        from deep_rl_battlespace_amd import learner
        self.tau = self.tau if tau is None else tau
        self.hyper = learner.adam_hyper(hp["lr"], (hp["beta1"], hp["beta2"]), hp["eps"], hp["max_grad_norm"], tau=self.tau)

    def tie(self):
        """Everything of the case tied in its group, as a learner with shared parameters starts."""
        from deep_rl_battlespace_amd import learner
        for x in self.nets + [t for t in self.targets if t is not None] + self.states + ([self.log_std, self.ls_state] if self.log_std is not None else []):
            for t in learner._tied_tensors(x):
                v = t.detach().view(self.A // self.group, self.group, *t.shape[1:])
                v.copy_(v[:, :1].clone().expand_as(v))

    def zeros(self):
        """Gradients of +0 in the shapes draw() gives."""
        return [torch.zeros_like(st.m) for st in self.states], (torch.zeros_like(self.log_std) if self.log_std is not None else None)

    def blobs_from_pack(self):
        for net, blob in zip(self.nets, self.blobs):
            blob.copy_(net.pack())

    def draw(self, gen, scale=1.0):
        """Fresh per-agent gradients on the GPU (every member of a group its own): one row per network, and log_std's."""
        rows = [U.random_rows(self.A, self.D, net.n_actions, gen, scale).cuda() for net in self.nets]
        g_ls = (scale * torch.randn((self.A, 3), generator=gen)).cuda() if self.log_std is not None else None
        return rows, g_ls

    def run(self, rows, g_ls, group="case", with_targets=True, **kw):
        """The entry's step on the case's tensors, with group = the case's own ("case"), without the argument ("default"), or with the
        value given, whatever it is; kw: keyword arguments of the entry, over the case's."""
        from deep_rl_battlespace_amd import learner
        args = dict(log_std=self.log_std, g_log_std=g_ls, log_std_state=self.ls_state, stats=self.stats, workspace=self.ws)
        if with_targets and any(t is not None for t in self.targets):
            args.update(targets=self.targets, target_blobs=self.target_blobs)
        if not (isinstance(group, str) and group == "default"):
            args["group"] = self.group if isinstance(group, str) and group == "case" else group
        step = learner.mlp_adam_step if self.entry == "mlp" else learner.adam_step
        return step(self.nets, rows, self.states, self.blobs, self.hyper, self.step, **dict(args, **kw))

    def tensors(self):
        """Everything the step writes, by name; all but step and stats have the leading agent axis."""
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

    def groups(self, leaders=False):
        """Per network (params, m, v) as lists of numpy arrays in ten-tensor shapes, of every agent or of the group LEADERS only;
        log_std rides with network 0.  A case with targets has a fourth column: the network's target, or None per tensor where there
        is none (a network without one, log_std)."""
        cut = lambda xs: [x[::self.group].copy() if leaders and x is not None else x for x in xs]     # noqa: E731
        out = []
        for i, (net, st, tgt) in enumerate(zip(self.nets, self.states, self.targets)):
            P = U.net_arrays(net)
            M, V = U.row_to_tensors(st.m.cpu().numpy(), net.n_actions), U.row_to_tensors(st.v.cpu().numpy(), net.n_actions)
            T = U.net_arrays(tgt) if tgt is not None else [None] * 10
            if i == 0 and self.log_std is not None:
                P.append(self.log_std.cpu().numpy().copy()); M.append(self.ls_state.m.cpu().numpy().copy()); V.append(self.ls_state.v.cpu().numpy().copy())
                T.append(None)
            out.append(tuple(cut(x) for x in ((P, M, V, T) if any(t is not None for t in self.targets) else (P, M, V))))
        return out


def same_bits(a, b, common=False):
    """Names of the tensors whose bits differ between two Case.bits().  The two hold the same names (asserted), or, with common=True
    (a case with targets beside one without), the names both have are compared."""
    assert common or sorted(a) == sorted(b), sorted(set(a) ^ set(b))
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


def members_equal_their_leader(case, bits, where):
    g = case.group
    for k, x in bits.items():
        if AGENT_AXIS(k):
            v = x.view(case.A // g, g, -1)
            assert torch.equal(v, v[:, :1].expand_as(v)), (where, k)


def flat_split(case, rows, g_ls):
    """The call's gradients as one list per network in ten-tensor shapes (torch, GPU), log_std's with network 0."""
    out = []
    for i, (net, row) in enumerate(zip(case.nets, rows)):
        g = U.row_to_tensors(row, net.n_actions)
        if i == 0 and g_ls is not None:
            g.append(g_ls.clone())
        out.append(g)
    return out


def first_norm(A, D, nas, with_ls, seed, group=1):
    """The float64 norm of the first gradients Case.draw gives from a generator seeded with `seed` -- of their float32 group sums."""
    gen = torch.Generator().manual_seed(seed)
    gs = [U.random_rows(A, D, na, gen) for na in nas] + ([torch.randn((A, 3), generator=gen)] if with_ls else [])
    sums = [torch.from_numpy(S.group_sum32(g.numpy(), group)) for g in gs]
    return float(np.sqrt(sum(float((x.double() ** 2).sum()) for x in sums)))


class TorchPath:
    """torch's float32 clip_grad_norm_ + Adam on the GPU over ONE parameter per group (copies of a case's leaders; every agent at
    group = 1), then target.mul_(1 - tau).add_(p, alpha=tau) where a target exists: the yardstick.  Its gradients are the members' rows
    added in float32 in agent order.  tau: default the case's; t0: the steps taken so far."""

    def __init__(self, case, hp, tau=None, t0=0):
        self.hp, self.g, self.tau = hp, case.group, case.tau if tau is None else tau
        self.with_targets = any(t is not None for t in case.targets)
        self.params, self.targets = [], []
        for i, (net, tgt) in enumerate(zip(case.nets, case.targets)):
            ps = [getattr(net, k).detach()[::self.g].clone().requires_grad_() for k in U.PARAMS]
            ts = [getattr(tgt, k).detach()[::self.g].clone() for k in U.PARAMS] if tgt is not None else [None] * 10
            if i == 0 and case.log_std is not None:
                ps.append(case.log_std[::self.g].clone().requires_grad_())
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
            for p, x in zip(ps, gs):
                v = x.view(x.shape[0] // self.g, self.g, *x.shape[1:])
                acc = v[:, 0].clone()
                for k in range(1, self.g):
                    acc += v[:, k]
                p.grad = acc
        if self.hp["max_grad_norm"] > 0.0:
            torch.nn.utils.clip_grad_norm_(self.flat, self.hp["max_grad_norm"])
        self.opt.step()
        with torch.no_grad():
            for ps, ts in zip(self.params, self.targets):
                for p, t in zip(ps, ts):
                    if t is not None:
                        t.mul_(1.0 - self.tau).add_(p, alpha=self.tau)

    def groups(self):
        """Case.groups(leaders=True)'s columns."""
        f = lambda x: None if x is None else x.detach().cpu().numpy()     # noqa: E731
        cols = lambda ps, ts: ([f(p) for p in ps], [f(self.opt.state[p]["exp_avg"]) for p in ps],     # noqa: E731
                               [f(self.opt.state[p]["exp_avg_sq"]) for p in ps], [f(t) for t in ts])
        return [cols(ps, ts)[:4 if self.with_targets else 3] for ps, ts in zip(self.params, self.targets)]


def start(case):
    """The float64 restatement's state at a case's present values: per network [P, M, V] or [P, M, V, T], every agent's."""
    return [[[None if x is None else np.asarray(x, np.float64) for x in col] for col in net] for net in case.groups()]


def advance(ref, grads, t, hp, tau=None, group=1):
    """One step of the float64 restatement over everything in the call at once (one global norm); with group > 1 the tied step
    (shared_step_util: the rows summed per group, a group counted once in the norm); with tau the Polyak line on the tensors that
    have a target.  ref (start's) is advanced in place -> (t + 1, norm, coef)."""
    sizes = [len(g) for g in grads]
    flat = lambda j: [x for net in ref for x in net[j]]     # noqa: E731
    G = [g.cpu().numpy() for gs in grads for g in gs]
    if group > 1:
        P, M, V, t, norm, coef = S.shared_reference_step(flat(0), G, flat(1), flat(2), t, hp, group)
    else:
        P, M, V, t, norm, coef = U.reference_step(flat(0), G, flat(1), flat(2), t, hp)
    cols = [P, M, V]
    if len(ref[0]) == 4:
        cols.append([None if x is None else MU.polyak([x], [p], tau)[0] for x, p in zip(flat(3), P)])
    o = 0
    for i, k in enumerate(sizes):
        ref[i] = [c[o:o + k] for c in cols]
        o += k
    return t, norm, coef


def record(name, leg, ratios, what="adam_step", env=None, key="config"):
    """Print the measured ratios; with `env` naming an environment variable that holds a file's path, append them to it as one JSON
    line under `key`.  BSX_ADAM_RATIOS_OUT / "config": how profiles/adam_step.json's accuracy table is made; BSX_ADAM_MLP_RATIOS_OUT /
    "shape": tools/measure_adam_mlp.py folds the lines into profiles/adam_step_mlp.json."""
    print(f"{what} {name} {leg}: " + ", ".join(f"{k} {m:.3f}/{x:.3f}" for k, (m, x) in sorted(ratios.items())))
    path = os.environ.get(env) if env else None
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({key: name, "leg": leg, "ratios": {k: [round(m, 4), round(x, 4)] for k, (m, x) in ratios.items()}}) + "\n")


def meets_the_bars(case, yard, ref, name, leg, which=("p", "m", "v", "target"), env=None, key="config"):
    """Per network and for each of parameters, m, v and targets, pooled over the group leaders' ten tensors (log_std with network 0's
    p, m, v): mean |error| against the float64 restatement at most 2x that of torch's own float32 path on the same inputs, maximum at
    most 4x (yardstick_util's pooled bars: a NaN fails).  Tensors without a reference (no target) are left out, and a column without any."""
    ratios, failed = {}, []
    for i, (mine, torchs, want) in enumerate(zip(case.groups(leaders=True), yard.groups(), ref)):
        for j, what in enumerate(("p", "m", "v", "target")[:len(want)]):
            keep = [k for k, x in enumerate(want[j]) if x is not None]
            if what not in which or not keep:
                continue
            pick = lambda xs: [xs[k] for k in keep]     # noqa: E731
            lead = [x[::case.group] for x in pick(want[j])]
            tm, tx = Y.errors(pick(torchs[j]), lead)
            assert tm > 0.0 and tx > 0.0
            ratios[f"net{i}.{what}"] = Y.error_ratios(pick(mine[j]), lead, pick(torchs[j]))
            if not Y.within(ratios[f"net{i}.{what}"]):
                failed.append((i, what, ratios[f"net{i}.{what}"], tm, tx))
    record(name, leg, ratios, ("mlp_adam_step" if case.entry == "mlp" else "adam_step") + (" shared" if case.group > 1 else ""), env, key)
    assert not failed, failed


def check_stats(case, stats, t, norm, coef, hp):
    """stats holds the exact step (and so does `step`), the norm and the clip coefficient within 1e-10 relative of float64 (an N-term
    float64 sum of exact squares is off by at most (N - 1) 2^-53, N <= 5.7e5) and the float32 lr."""
    got = stats.cpu().numpy()
    assert got[0] == t and int(case.step) == t, (got, int(case.step), t)
    assert abs(got[1] - norm) <= 1e-10 * norm and abs(got[2] - coef) <= 1e-10 * coef and got[3] == hp["lr"], (got, norm, coef)
