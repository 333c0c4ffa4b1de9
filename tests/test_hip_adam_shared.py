"""The tied optimiser step on the GPU (learner.adam_step(group=g), csrc/bsx_adam_step.hip: bsx_adam_step_shared): the equivalence the
contract pins -- bit for bit the untied step on (group sum at the leaders, +0 at the followers) --, members that stay identical, the
float64 restatement of tests/shared_step_util.py with torch's own float32 clip_grad_norm_ + Adam over the shared parameters as the
yardstick, a gradient that only a follower holds, the all-zero group, poisoned pad columns, guard words, determinism, group = 1.

Shapes: n = 1 with g = 2 (everyone: the smallest call), n = 2 with g = 2 (one policy per team), n = 3 with g = 3 and g = 6 (D = 11, odd:
the blob's pad row; a 3-column actor and log_std), n = 4 with g = 2 (two groups per team), n = 16 with g = 16 and g = 32 with log_std:
the 65-partial call, the longest sum.  Two networks in every call."""
import ctypes

import numpy as np
import pytest
import torch

import adam_util as U
import guard_util as GU
import shared_step_util as S

pytestmark = pytest.mark.gpu

#        id                  n   g  n_actions log_std
CONFIGS = {"n1-g2": (1, 2, 4, False), "n2-g2": (2, 2, 4, False), "n3-g3-gaussian": (3, 3, 3, True), "n3-g6-gaussian": (3, 6, 3, True),
           "n4-g2": (4, 2, 4, False), "n16-g16-gaussian": (16, 16, 3, True), "n16-g32-gaussian": (16, 32, 3, True)}
STEPS = 5


class Case:
    """A policy and a value network tied in groups of g, their Adam state, blobs (pre-filled with a non-zero pattern), log_std, hyper,
    counter, stats and workspace on the GPU.  alloc: a guard_util.Buffers -- every buffer the step writes is then a view between guard
    bytes."""

    def __init__(self, config, hp, seed=0, alloc=None):
        from deep_rl_battlespace_amd import learner
        from deep_rl_battlespace_amd.rollout import StackedActor
        n, g, na, with_ls = CONFIGS[config]
        self.n, self.g, self.A, self.D = n, g, 2 * n, 3 * n + 2
        A, D = self.A, self.D
        alloc = alloc or GU.Buffers(False)
        torch.manual_seed(200 + seed)
        self.nets = [StackedActor(A, D, na, device="cuda"), StackedActor(A, D, 1, device="cuda")]
        self.states, self.blobs = [], []
        for i, net in enumerate(self.nets):
            for k in U.PARAMS:                                              # the parameters as views of the allocator's buffers
                p = getattr(net, k)
                buf = alloc(f"net{i}.{k}", p.shape, torch.float32)
                buf.copy_(p.detach())
                setattr(net, k, torch.nn.Parameter(buf))
            learner.tie_(net, g)
            st = learner.AdamState(net)
            st.m, st.v = alloc(f"net{i}.m", st.m.shape, torch.float32), alloc(f"net{i}.v", st.v.shape, torch.float32)
            self.states.append(st)
            self.blobs.append(alloc(f"net{i}.blob", (A, learner.blob_floats(D)), torch.float32, init=-7.25))
        self.log_std = self.ls_state = None
        if with_ls:
            self.log_std = alloc("log_std", (A, 3), torch.float32, init=-0.5)
            self.log_std.copy_(-0.5 + 0.1 * torch.randn(A, 3, device="cuda"))
            learner.tie_(self.log_std, g)
            self.ls_state = learner.AdamState(self.log_std)
            self.ls_state.m, self.ls_state.v = alloc("ls.m", (A, 3), torch.float32), alloc("ls.v", (A, 3), torch.float32)
        self.set_hyper(hp)
        self.step = alloc("step", (1,), torch.int64)
        self.stats = alloc("stats", (4,), torch.float64, init=-1)
        nb = learner.adam_step_workspace_bytes(n, 2)
        self.ws = alloc("ws", ((nb + 7) // 8,), torch.int64)

    def set_hyper(self, hp):
        from deep_rl_battlespace_amd import learner
        self.hyper = learner.adam_hyper(hp["lr"], (hp["beta1"], hp["beta2"]), hp["eps"], hp["max_grad_norm"])

    def zeros(self):
        return [torch.zeros_like(st.m) for st in self.states], (torch.zeros_like(self.log_std) if self.log_std is not None else None)

    def blobs_from_pack(self):
        for net, blob in zip(self.nets, self.blobs):
            blob.copy_(net.pack())

    def draw(self, gen, scale=1.0):
        """Fresh per-agent gradients on the GPU (every member its own): one row per network, and log_std's."""
        rows = [U.random_rows(self.A, self.D, net.n_actions, gen, scale).cuda() for net in self.nets]
        g_ls = (scale * torch.randn((self.A, 3), generator=gen)).cuda() if self.log_std is not None else None
        return rows, g_ls

    def run(self, rows, g_ls, group="case", **kw):
        """adam_step with group = the case's g ("case"), without the argument ("default"), or with the value given."""
        from deep_rl_battlespace_amd import learner
        if group == "case":
            group = self.g
        kw = dict(dict(log_std=self.log_std, g_log_std=g_ls, log_std_state=self.ls_state, stats=self.stats, workspace=self.ws), **kw)
        if not (isinstance(group, str) and group == "default"):
            kw["group"] = group
        return learner.adam_step(self.nets, rows, self.states, self.blobs, self.hyper, self.step, **kw)

    def tensors(self):
        """Everything the step writes, by name; all but step and stats have the leading agent axis."""
        out = {"step": self.step, "stats": self.stats}
        for i, (net, st, blob) in enumerate(zip(self.nets, self.states, self.blobs)):
            out.update({f"net{i}.{k}": getattr(net, k).detach() for k in U.PARAMS})
            out.update({f"net{i}.m": st.m, f"net{i}.v": st.v, f"net{i}.blob": blob})
        if self.log_std is not None:
            out.update({"log_std": self.log_std, "ls.m": self.ls_state.m, "ls.v": self.ls_state.v})
        return out

    def bits(self):
        torch.cuda.synchronize()
        return {k: v.clone().view(torch.int32 if v.element_size() == 4 else torch.int64) for k, v in self.tensors().items()}

    def leader_groups(self):
        """Per network (params, m, v) of the LEADERS as lists of numpy arrays in ten-tensor shapes; log_std rides with the policy network."""
        out, g = [], self.g
        for i, (net, st) in enumerate(zip(self.nets, self.states)):
            P = [x[::g] for x in U.net_arrays(net)]
            M = [x[::g] for x in U.row_to_tensors(st.m.cpu().numpy(), net.n_actions)]
            V = [x[::g] for x in U.row_to_tensors(st.v.cpu().numpy(), net.n_actions)]
            if i == 0 and self.log_std is not None:
                P.append(self.log_std.cpu().numpy()[::g].copy()); M.append(self.ls_state.m.cpu().numpy()[::g].copy())
                V.append(self.ls_state.v.cpu().numpy()[::g].copy())
            out.append((P, M, V))
        return out


AGENT_AXIS = lambda k: k not in ("step", "stats")     # noqa: E731


def _same_bits(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def _blobs_are_packs(case, where):
    for i, (net, blob) in enumerate(zip(case.nets, case.blobs)):
        want = net.pack()
        bad = (blob.view(torch.int32) != want.view(torch.int32)).nonzero()
        assert blob.shape == want.shape and bad.numel() == 0, (where, i, bad[:4].tolist())


def _members_equal_their_leader(case, bits, where):
    g = case.g
    for k, x in bits.items():
        if AGENT_AXIS(k):
            v = x.view(case.A // g, g, -1)
            assert torch.equal(v, v[:, :1].expand_as(v)), (where, k)


def _host_leaders_rows(rows, g_ls, g):
    """The untied call's gradients: the float32 group sum, added on the host in agent order, at the leaders and +0 at the followers."""
    out = [torch.from_numpy(S.leaders_rows(r.cpu().numpy(), g)).cuda() for r in rows]
    return out, (torch.from_numpy(S.leaders_rows(g_ls.cpu().numpy(), g)).cuda() if g_ls is not None else None)


def _first_norm(config, seed):
    """The float64 norm of the first drawn gradients' group sums."""
    probe = Case(config, U.hyper32())
    rows, g_ls = probe.draw(torch.Generator().manual_seed(seed))
    sums = [S.group_sum32(x.cpu().numpy(), probe.g).astype(np.float64) for x in rows + ([g_ls] if g_ls is not None else [])]
    return float(np.sqrt(sum(float((x * x).sum()) for x in sums)))


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_five_tied_steps_are_the_untied_step_on_the_group_sums_bit_for_bit_and_members_stay_identical(config, clip):
    """Twins from one seed.  `tied` takes the per-agent rows and group = g; `plain` takes, through the untied adam_step, the rows
    that hold the float32 group sum (added on the host, in agent order from the leader on) at every leader and +0 at every follower.
    After each of five steps with fresh gradients (steps 2 and 4 a tenth of the others: max_grad_norm, half the first norm, bites on 1,
    3, 5): the leaders' parameters, moments and blob rows, `step` and all of stats are bit-equal between the two; in `tied` every
    member equals its leader in every tensor and every blob is pack() of its parameters."""
    hp = U.hyper32(lr=1e-3, max_grad_norm=0.5 * _first_norm(config, 61) if clip else 0.0)
    tied, plain = Case(config, hp, seed=1), Case(config, hp, seed=1)
    g = tied.g
    assert _same_bits(tied.bits(), plain.bits()) == []
    gen = torch.Generator().manual_seed(61)
    coefs = []
    for s in range(STEPS):
        rows, g_ls = tied.draw(gen, 0.1 if s in (1, 3) else 1.0)
        tied.run(rows, g_ls)
        plain.run(*_host_leaders_rows(rows, g_ls, g), group=1)
        a, b = tied.bits(), plain.bits()
        for k in a:
            if AGENT_AXIS(k):
                assert torch.equal(a[k][::g], b[k][::g]), (s, k)
            else:
                assert torch.equal(a[k], b[k]), (s, k, a[k], b[k])
        _members_equal_their_leader(tied, a, s)
        _blobs_are_packs(tied, (config, s))
        assert int(tied.step) == s + 1
        coefs.append(float(tied.stats[2]))
    assert [c < 1.0 for c in coefs] == ([True, False, True, False, True] if clip else [False] * 5), coefs
    moved = _same_bits(tied.bits(), Case(config, hp, seed=1).bits())
    assert sorted(moved) == sorted(tied.tensors()), moved                 # everything moved: no tensor was compared at its start value


class TorchShared:
    """torch's float32 clip_grad_norm_ + Adam on the GPU over ONE parameter per group (copies of a case's leaders): the yardstick.
    Its gradients are the members' rows added in float32 in agent order."""

    def __init__(self, case, hp, t0):
        self.hp, self.g = hp, case.g
        self.params = []
        for i, net in enumerate(case.nets):
            ps = [getattr(net, k).detach()[::case.g].clone().requires_grad_() for k in U.PARAMS]
            if i == 0 and case.log_std is not None:
                ps.append(case.log_std[::case.g].clone().requires_grad_())
            self.params.append(ps)
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

    def groups(self):
        f = lambda x: x.detach().cpu().numpy()     # noqa: E731
        return [([f(p) for p in ps], [f(self.opt.state[p]["exp_avg"]) for p in ps], [f(self.opt.state[p]["exp_avg_sq"]) for p in ps])
                for ps in self.params]


def _flat_split(case, rows, g_ls):
    out = []
    for i, (net, row) in enumerate(zip(case.nets, rows)):
        x = U.row_to_tensors(row, net.n_actions)
        if i == 0 and g_ls is not None:
            x.append(g_ls.clone())
        out.append(x)
    return out


#       leg                lr     counter set to (before step index)     (the legs of the untied step's test)
LEGS = {"lr3e-4-from-0": (3e-4, {}), "counter-1000-after-3": (3e-4, {3: 1000}), "lr0.05-counter-1000": (0.05, {0: 1000})}


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_five_tied_steps_match_the_float64_restatement_as_well_as_torch_does(config, leg):
    """The untied step's test (tests/test_hip_adam_step.py) with its bars, for shared parameters: after five clipped steps, per network
    and for each of parameters, m, v, pooled over the leaders' ten tensors (log_std with the policy network): mean |error| against
    shared_step_util.shared_reference_step at most 2x that of torch's own float32 path on the same inputs, maximum at most 4x.  torch
    steps one parameter per group with the float32 sum of the members' rows, added in agent order.  stats holds the exact step and the
    float64 norm and coefficient of the restatement within 1e-10 relative."""
    lr, counter = LEGS[leg]
    hp = U.hyper32(lr=lr, max_grad_norm=0.5 * _first_norm(config, 67))
    case = Case(config, hp, seed=2)
    g = case.g
    yard = TorchShared(case, hp, 0)
    wide = lambda grp: [[np.repeat(np.asarray(x, np.float64), g, axis=0) for x in part] for part in grp]     # noqa: E731
    ref = [wide(grp) for grp in case.leader_groups()]                   # per network [P, M, V] with the agent axis
    sizes = [len(r[0]) for r in ref]
    t, coefs = 0, []
    gen = torch.Generator().manual_seed(67)
    for s in range(STEPS):
        if s in counter:
            t = counter[s]
            case.step.fill_(t)
            yard.set_counter(t)
        rows, g_ls = case.draw(gen, 0.1 if s in (1, 3) else 1.0)
        grads = _flat_split(case, rows, g_ls)
        stats = case.run(rows, g_ls)
        yard.step(grads)
        flat = lambda j: [x for r in ref for x in r[j]]     # noqa: E731
        P, M, V, t, norm, coef = S.shared_reference_step(flat(0), [x.cpu().numpy() for xs in grads for x in xs], flat(1), flat(2), t, hp, g)
        o = 0
        for i, k in enumerate(sizes):
            ref[i] = [P[o:o + k], M[o:o + k], V[o:o + k]]
            o += k
        coefs.append(coef)
        got = stats.cpu().numpy()
        assert got[0] == t and int(case.step) == t
        # the kernel's norm is over the float32 group sums, the restatement's over float64 sums: they differ by the sums' rounding
        sums = [S.group_sum32(x.cpu().numpy(), g).astype(np.float64) for xs in grads for x in xs]
        norm32 = float(np.sqrt(sum(float((x * x).sum()) for x in sums)))
        coef32 = min(1.0, hp["max_grad_norm"] / (norm32 + 1e-6))
        assert abs(got[1] - norm32) <= 1e-10 * norm32 and abs(got[2] - coef32) <= 1e-10 * coef32 and got[3] == hp["lr"], (got, norm32, coef32)
        assert abs(norm32 - norm) <= 1e-6 * norm
    assert [c < 1.0 for c in coefs] == [True, False, True, False, True], coefs
    _blobs_are_packs(case, (config, leg))
    ratios, failed = {}, []
    for i, (mine, torchs, want) in enumerate(zip(case.leader_groups(), yard.groups(), ref)):
        for j, what in enumerate(("p", "m", "v")):
            lead = [x[::g] for x in want[j]]
            (em, ex), (tm, tx) = U.pooled_errors(mine[j], lead), U.pooled_errors(torchs[j], lead)
            assert tm > 0.0 and tx > 0.0
            ratios[f"net{i}.{what}"] = (em / tm, ex / tx)
            if em > 2.0 * tm or ex > 4.0 * tx:
                failed.append((i, what, em, tm, ex, tx))
    print(f"adam_step shared {config} {leg}: " + ", ".join(f"{k} {m:.3f}/{x:.3f}" for k, (m, x) in sorted(ratios.items())))
    assert not failed, failed


@pytest.mark.parametrize("config,where,agent", [("n3-g3-gaussian", 0, 1), ("n3-g3-gaussian", 1, 5), ("n3-g3-gaussian", None, 4),
                                                ("n16-g16-gaussian", 1, 31), ("n16-g32-gaussian", None, 17), ("n4-g2", 0, 3)])
def test_a_gradient_that_only_a_follower_holds_reaches_the_norm_and_moves_its_whole_group_identically(config, where, agent):
    """One call in which the only non-zero gradient is the row of one FOLLOWER (network `where`, or log_std's row with None), moments
    +0, max_grad_norm half that row's float64 norm.  Its workgroup contributes no partial of its own, yet stats holds that row's norm
    (1e-10 relative) and the coefficient bites; every member of its group moves, identically, in the tensors the row belongs to; every
    other group and every other tensor keeps every bit (the blobs start as pack())."""
    case = Case(config, U.hyper32(lr=0.01))
    g = case.g
    assert agent % g != 0
    case.blobs_from_pack()
    drawn, drawn_ls = case.draw(torch.Generator().manual_seed(71 + agent))
    rows, g_ls = case.zeros()
    if where is None:
        g_ls[agent] = drawn_ls[agent]
        alone, mine = g_ls[agent], ("log_std", "ls.m", "ls.v")
    else:
        rows[where][agent] = drawn[where][agent]
        alone, mine = rows[where][agent], tuple(f"net{where}.{k}" for k in U.PARAMS + ("m", "v", "blob"))
    norm = float(np.sqrt(float((alone.double() ** 2).sum())))
    hp = U.hyper32(lr=0.01, max_grad_norm=0.5 * norm)
    case.set_hyper(hp)
    before = case.bits()
    stats = case.run(rows, g_ls).cpu().numpy()
    after = case.bits()
    coef = hp["max_grad_norm"] / (norm + 1e-6)
    assert stats[0] == 1 and abs(stats[1] - norm) <= 1e-10 * norm and abs(stats[2] - coef) <= 1e-10 * coef and stats[2] < 1.0, (stats, norm, coef)
    members = list(range(agent // g * g, agent // g * g + g))
    others = [a for a in range(case.A) if a not in members]
    for k in before:
        if not AGENT_AXIS(k):
            continue
        if k in mine:
            assert torch.equal(before[k][others], after[k][others]), k
            for a in members:
                assert not torch.equal(before[k][a], after[k][a]), (k, a)
        else:
            assert torch.equal(before[k], after[k]), k
    _members_equal_their_leader(case, after, config)
    _blobs_are_packs(case, config)


@pytest.mark.parametrize("max_grad_norm", [0.0, 1.0])
@pytest.mark.parametrize("config", ["n4-g2", "n3-g3-gaussian"])
def test_a_group_whose_sum_and_moments_are_zero_keeps_every_bit(config, max_grad_norm):
    """What a scripted opponent's team is to the learner.  Group 1 (where there are three groups or more): every member's gradient +0.
    The last group: the members' gradients cancel in the stated order (r, -r, then +0s: (r + -r) + 0 = +0) -- it is the SUM that
    decides, not the rows.  Both keep parameters, moments and blob rows bit for bit, with clipping on and off; the other groups move."""
    case = Case(config, U.hyper32(lr=0.01, max_grad_norm=max_grad_norm))
    g, A = case.g, case.A
    case.blobs_from_pack()
    before = case.bits()
    rows, g_ls = case.draw(torch.Generator().manual_seed(73))
    last = A - g
    zeroed = list(range(g, 2 * g)) if A // g >= 3 else []
    for x in rows + ([g_ls] if g_ls is not None else []):
        x[zeroed] = 0.0
        x[last + 1] = -x[last]
        x[last + 2:] = 0.0
    case.run(rows, g_ls)
    after = case.bits()
    assert (float(case.stats[2]) < 1.0) == (max_grad_norm > 0.0) and float(case.stats[1]) > 0.0
    assert all(bool((x[last] != 0).any()) for x in rows)
    frozen = zeroed + list(range(last, A))
    moving = [a for a in range(A) if a not in frozen]
    assert moving
    for k in before:
        if AGENT_AXIS(k):
            assert torch.equal(before[k][frozen], after[k][frozen]), k
            for a in moving:
                assert not torch.equal(before[k][a], after[k][a]), (k, a)


@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("config", ["n3-g3-gaussian", "n3-g6-gaussian"])
def test_poisoned_pad_columns_of_every_member_are_neither_read_nor_written(config, poison):
    """Twins from one seed, B with every pad element (columns n_actions..3 of w3 / b3) of EVERY member's gradient rows at NaN (or 1e30)
    and of its moments at 7.25.  After each of two clipped steps every tensor of B equals A's bit for bit outside the moments' pads --
    the norm and the coefficient among them --, B's pads still hold 7.25, A's +0, and every blob is pack()."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    a, b = Case(config, hp, seed=3), Case(config, hp, seed=3)
    masks = [torch.from_numpy(U.pad_mask(a.D, net.n_actions)).cuda() for net in a.nets]
    assert all(int(m.sum()) for m in masks)
    sentinel = torch.tensor(7.25).view(torch.int32).item()
    for st, mask in zip(b.states, masks):
        st.m[:, mask] = 7.25
        st.v[:, mask] = 7.25
    moments = {f"net{i}.{x}": mask for i, mask in enumerate(masks) for x in "mv"}
    gen = torch.Generator().manual_seed(79)
    for s in range(2):
        rows, g_ls = a.draw(gen)
        poisoned = [r.clone() for r in rows]
        for r, mask in zip(poisoned, masks):
            r[:, mask] = poison
        a.run(rows, g_ls)
        b.run(poisoned, g_ls.clone())
        x, y = a.bits(), b.bits()
        assert float(a.stats[2]) < 1.0 and int(a.step) == s + 1
        for k in x:
            if k in moments:
                mask = moments[k]
                assert torch.equal(x[k][:, ~mask], y[k][:, ~mask]), (s, k)
                assert bool((y[k][:, mask] == sentinel).all()) and bool((x[k][:, mask] == 0).all()), (s, k)
            else:
                assert torch.equal(x[k], y[k]), (s, k)
        _blobs_are_packs(b, (config, s))


@pytest.mark.parametrize("config", ["n1-g2", "n3-g6-gaussian", "n16-g16-gaussian", "n16-g32-gaussian"])
def test_two_tied_calls_from_copies_of_one_state_give_identical_bits_and_leave_the_guards_alone(config):
    hp = U.hyper32(max_grad_norm=5.0)
    alloc = GU.Buffers(True)
    a, b = Case(config, hp, alloc=alloc), Case(config, hp)
    gen = torch.Generator().manual_seed(83)
    for _ in range(2):
        rows, g_ls = a.draw(gen)
        a.run(rows, g_ls)
        b.run([r.clone() for r in rows], g_ls.clone() if g_ls is not None else None)
    assert _same_bits(a.bits(), b.bits()) == []
    assert int(a.step) == 2 and float(a.stats[2]) < 1.0
    assert alloc.stray() == []
    _blobs_are_packs(a, config)
    _members_equal_their_leader(a, a.bits(), config)


def _c_entry(case, rows, g_ls, group):
    """bsx_adam_step_shared itself, on a case's tensors."""
    from deep_rl_battlespace_amd import _lib as L
    io = L.BsxAdamIo()
    io.nets = len(case.nets)
    for i, (net, row, st, blob) in enumerate(zip(case.nets, rows, case.states, case.blobs)):
        for q, k in enumerate(U.PARAMS):
            io.net[i].p[q] = getattr(net, k).data_ptr()
        io.net[i].grad, io.net[i].m, io.net[i].v, io.net[i].blob, io.net[i].n_actions = row.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), blob.data_ptr(), net.n_actions
    if g_ls is not None:
        io.log_std, io.g_log_std, io.m_ls, io.v_ls = case.log_std.data_ptr(), g_ls.data_ptr(), case.ls_state.m.data_ptr(), case.ls_state.v.data_ptr()
    io.hyper, io.step = case.hyper.data_ptr(), case.step.data_ptr()
    rc = L.load().bsx_adam_step_shared(ctypes.byref(io), case.n, group, case.ws.data_ptr(), case.stats.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("config", ["n3-g3-gaussian", "n16-g32-gaussian"])
def test_group_one_gives_the_untied_steps_bits(config):
    """Three ways to step untied networks (made different per agent first): adam_step without the argument, adam_step(group=1), and
    the C entry bsx_adam_step_shared with group = 1 -- identical bits after two clipped steps; the C entry with the case's group on
    the same inputs does differ."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    cases = [Case(config, hp, seed=4) for _ in range(4)]
    for c in cases:
        torch.manual_seed(5)
        with torch.no_grad():
            for net in c.nets:
                for k in U.PARAMS:
                    getattr(net, k).add_(0.01 * torch.randn_like(getattr(net, k)))
    gen = torch.Generator().manual_seed(89)
    for _ in range(2):
        rows, g_ls = cases[0].draw(gen)
        cases[0].run(rows, g_ls, group="default")
        cases[1].run(rows, g_ls, group=1)
        assert _c_entry(cases[2], rows, g_ls, 1) == 0
        assert _c_entry(cases[3], rows, g_ls, cases[3].g) == 0
    bits = [c.bits() for c in cases]
    assert _same_bits(bits[0], bits[1]) == [] and _same_bits(bits[0], bits[2]) == []
    assert "net0.w1" in _same_bits(bits[0], bits[3])
    _blobs_are_packs(cases[2], config)


def test_the_binding_refuses_bad_groups_by_name_and_launches_nothing():
    case = Case("n4-g2", U.hyper32())
    rows, g_ls = case.draw(torch.Generator().manual_seed(97))
    before = case.bits()
    for bad in (0, -1, 3, 5, 9, 16):
        with pytest.raises(ValueError, match="group"):
            case.run(rows, g_ls, group=bad)
    for bad in ("team", None, 2.0, True):
        with pytest.raises(ValueError, match="group"):
            case.run(rows, g_ls, group=bad)
    assert _same_bits(before, case.bits()) == []
    for good in (2, 4, 8, 1):
        case.run(rows, g_ls, group=good)
    assert int(case.step) == 4
