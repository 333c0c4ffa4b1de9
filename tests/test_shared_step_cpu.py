"""The tied optimiser step without a GPU: the entry point is declared, exported and bound and refuses bad groups on the host in the
documented order; share_group / tie_ / is_tied on CPU tensors; what sharing MEANS -- autograd's gradient of a shared parameter is the sum of
the per-agent gradients of the untied network -- in float64; and the float64 restatement the GPU tests measure against
(tests/shared_step_util.py) against torch's float64 Adam over a genuinely shared parameter list."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_util as U
import shared_step_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_the_entry_is_declared_exported_and_bound_and_the_abi_version_stays():
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import _lib as L
    from deep_rl_battlespace_amd import learner
    header = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    assert re.search(r"int\s+bsx_adam_step_shared\(const BsxAdamIo\* io, int n, int group, void\* workspace, double\* stats, void\* stream\);", header)
    assert L.ABI_VERSION == 14 and re.search(r"#define\s+BSX_ABI_VERSION\s+14\b", header)
    lib = L.load()
    assert lib.bsx_abi_version() == 14
    fn = lib.bsx_adam_step_shared
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6 and fn.argtypes[1] is ctypes.c_int and fn.argtypes[2] is ctypes.c_int
    for name in ("share_group", "tie_", "is_tied"):
        assert getattr(bsx, name) is getattr(learner, name) and name in bsx.__all__


def test_the_c_entry_refuses_bad_groups_before_any_launch_in_the_documented_order():
    """Fake addresses only: every call is refused before anything reaches HIP.  The group rule comes after the n / nets rules and
    before the per-network ones; argument rules before alignment rules; a valid group falls through to the rules of bsx_adam_step."""
    from deep_rl_battlespace_amd import _lib as L
    lib = L.load()
    A16, A4 = 4096, 4096 + 4
    ARG, ALIGN = -1, -2

    def call(n, group, nets=2, na=(4, 1), grad=A16, ws=A16):
        st = L.BsxAdamIo()
        st.nets = nets
        for i in range(2):
            for q in range(10):
                st.net[i].p[q] = A16
            for f in ("grad", "m", "v", "blob"):
                setattr(st.net[i], f, A16)
            st.net[i].n_actions = na[i]
        st.net[0].grad = grad
        st.hyper = st.step = A16
        return lib.bsx_adam_step_shared(ctypes.byref(st), n, group, ws, A16, None)

    bad = [(2, 0), (2, -1), (2, -2), (4, 3), (3, 2), (6, 4), (2, 3), (2, 5), (4, 9), (16, 33), (1, 3), (16, 5), (6, 12 + 1)]
    good = [(1, 1), (1, 2), (2, 2), (2, 4), (3, 3), (3, 6), (4, 2), (4, 4), (4, 8), (16, 16), (16, 32), (16, 8), (6, 3), (6, 2), (5, 1)]
    for n, g in bad:
        assert call(n, g) == ARG, (n, g)
        assert call(n, g, grad=A4) == ARG, (n, g)                     # ... before any alignment rule
    # a valid group is not what refuses: the only fault left is an alignment one, and that is what comes back
    for n, g in good:
        assert call(n, g, grad=A4) == ALIGN, (n, g)
        assert call(n, g, ws=A4) == ALIGN, (n, g)
    # the order: n / nets first (a group that would be valid for another n says nothing), then the group, then the per-network rules
    assert call(0, 1) == ARG and call(17, 34) == ARG and call(2, 2, nets=3) == ARG
    assert call(2, 2, na=(2, 1)) == ARG and call(2, 2, grad=None) == ARG
    assert call(2, 3, na=(2, 1), grad=A4) == ARG
    st = L.BsxAdamIo()
    assert lib.bsx_adam_step_shared(None, 2, 2, A16, A16, None) == ARG
    assert lib.bsx_adam_step_shared(ctypes.byref(st), 2, 2, A16, A16, None) == ARG    # (null hyper / step)


def test_share_group_resolves_names_and_validates_ints():
    from deep_rl_battlespace_amd.learner import share_group
    for n in (1, 2, 3, 4, 16):
        assert share_group(None, n) == 1 and share_group("team", n) == n and share_group("all", n) == 2 * n
        assert share_group(1, n) == 1 and share_group(2 * n, n) == 2 * n
        assert all(isinstance(share_group(s, n), int) for s in (None, "team", "all"))
    assert share_group(2, 4) == 2 and share_group(4, 4) == 4 and share_group(3, 6) == 3 and share_group(8, 16) == 8
    for share, n in ((0, 2), (-1, 2), (-2, 2), (3, 4), (2, 3), (5, 2), (3, 1), (33, 16), (4, 6), ("red", 2), ("", 2), (2.0, 2), (True, 2),
                     ([2], 2), (torch.tensor(2), 2)):
        with pytest.raises(ValueError):
            share_group(share, n)
    with pytest.raises(ValueError, match="n must be"):
        share_group(None, 0)


def test_tie_and_is_tied_on_cpu_tensors_networks_and_moments():
    from deep_rl_battlespace_amd.learner import AdamState, is_tied, tie_
    from deep_rl_battlespace_amd.rollout import StackedActor
    torch.manual_seed(3)
    # a tensor: log_std [A, 3], n = 2, groups of 2
    ls = torch.randn(4, 3)
    want = ls.clone()
    want[1], want[3] = want[0], want[2]
    assert not is_tied(ls, 2) and is_tied(ls, 1)
    assert tie_(ls, 2) is ls and torch.equal(ls, want) and is_tied(ls, 2) and not is_tied(ls, 4)
    assert tie_(ls, 1) is ls and torch.equal(ls, want)
    tie_(ls, 4)
    assert torch.equal(ls, want[:1].expand(4, 3)) and is_tied(ls, 4) and is_tied(ls, 2)
    # a network: every one of the ten parameters, in place (the Parameters stay the same objects), no graph recorded
    net = StackedActor(6, 11, 3)
    before = {k: getattr(net, k) for k in U.PARAMS}
    old = {k: v.detach().clone() for k, v in before.items()}
    assert not is_tied(net, 3)
    assert tie_(net, 3) is net and is_tied(net, 3) and not is_tied(net, 6)
    for k in U.PARAMS:
        p = getattr(net, k)
        assert p is before[k] and p.requires_grad and p.grad_fn is None
        for a in range(6):
            assert torch.equal(p[a], old[k][a // 3 * 3]), (k, a)
    one = net.b3.detach().clone()
    with torch.no_grad():
        net.b3[4, 0, 1] += 1.0
    assert not is_tied(net, 3)
    with torch.no_grad():
        net.b3.copy_(one)
    assert is_tied(net, 3)
    # moments
    st = AdamState(net)
    st.m.normal_(); st.v.uniform_()
    assert not is_tied(st, 3)
    m0 = st.m.clone()
    assert tie_(st, 3) is st and is_tied(st, 3) and torch.equal(st.m[4], m0[3]) and torch.equal(st.v[1], st.v[0])
    # refusals: a group that does not fit the leading axis, a non-int group, something that has no agent axis
    for bad in (0, 4, 5, -1):
        with pytest.raises(ValueError):
            tie_(net, bad)
        with pytest.raises(ValueError):
            is_tied(st, bad)
    with pytest.raises(ValueError):
        tie_(ls, "team")
    with pytest.raises(ValueError):
        is_tied(ls, None)
    with pytest.raises(ValueError):
        tie_(torch.zeros(3, 3), 1)
    with pytest.raises(ValueError):
        tie_(torch.zeros(()), 1)
    with pytest.raises(TypeError):
        tie_([ls], 2)
    with pytest.raises(TypeError):
        is_tied(None, 2)


def test_the_binding_refuses_a_bad_group_by_name_before_it_needs_a_device():
    from deep_rl_battlespace_amd import learner
    from deep_rl_battlespace_amd.rollout import StackedActor
    net = StackedActor(4, 8, 4)
    st = learner.AdamState(net)
    row, blob = torch.zeros_like(st.m), torch.zeros(4, learner.blob_floats(8))
    hyper, step = learner.adam_hyper(device="cpu"), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        learner.adam_step([net], [row], [st], [blob], hyper, step, group=2)


@pytest.mark.parametrize("n,g", [(2, 2), (3, 6)])
def test_the_gradient_of_a_shared_parameter_is_the_sum_of_its_members_gradients(n, g):
    """float64, CPU.  A StackedActor whose parameters are `expand`ed views of one leader set per group, against the untied network
    holding the same values: for a scalar loss over all agents' outputs, autograd's gradient with respect to the leader set equals the
    sum of the untied per-agent gradients over each group -- what the tied step adds up."""
    from deep_rl_battlespace_amd.rollout import StackedActor
    A, D, na, E = 2 * n, 3 * n + 2, 4, 7
    torch.manual_seed(5 + n)
    untied = StackedActor(A, D, na, dtype=torch.float64)
    from deep_rl_battlespace_amd.learner import is_tied, tie_
    tie_(untied, g)
    assert is_tied(untied, g)
    tied = StackedActor(A, D, na, dtype=torch.float64)
    leaders = {}
    for k in U.PARAMS:
        p = getattr(untied, k).detach()
        lead = p[::g].clone().requires_grad_()
        leaders[k] = lead
        delattr(tied, k)
        setattr(tied, k, lead.unsqueeze(1).expand(A // g, g, *p.shape[1:]).reshape(A, *p.shape[1:]))
        assert torch.equal(getattr(tied, k), p)
    obs = torch.randn(E, A, D, dtype=torch.float64)
    weight = torch.randn(E, A, na, dtype=torch.float64)
    loss = lambda net: (weight * net(obs)).sum() + (net(obs, squash=False) ** 2).mean()     # noqa: E731
    la, lb = loss(untied), loss(tied)
    assert float(la.detach()) == float(lb.detach())
    la.backward()
    lb.backward()
    for k in U.PARAMS:
        per_agent = getattr(untied, k).grad
        want = per_agent.view(A // g, g, *per_agent.shape[1:]).sum(dim=1)
        got = leaders[k].grad
        assert got.shape == want.shape and float(want.abs().max()) > 0.0
        assert _rel(got.numpy(), want.numpy()) <= 1e-12, k
        if g > 1:                                                  # ... and is not any single member's gradient
            assert _rel(got.numpy(), per_agent[::g].numpy()) > 1e-3, k


@pytest.mark.parametrize("A,g", [(4, 2), (6, 6), (6, 3), (2, 1)])
def test_the_float64_restatement_is_torch_adam_over_a_genuinely_shared_parameter_list(A, g):
    """Five clipped steps.  torch's side holds ONE parameter per group (leading axis A / g) whose .grad is the sum of the members' rows;
    the restatement takes the per-agent rows and gives every member its group's result.  The groups are ones share_group accepts."""
    from deep_rl_battlespace_amd.learner import share_group
    assert share_group(g, A // 2) == g
    gen = torch.Generator().manual_seed(7)
    D, na = 3 * (A // 2) + 2, 3
    shapes = [(D, 64)] + [(1, 64)] * 3 + [(64, 64)] + [(1, 64)] * 3 + [(64, na), (1, na), (3,)]
    lead = [torch.randn((A // g, *s), generator=gen, dtype=torch.float64) * 0.1 for s in shapes]
    params = [torch.nn.Parameter(x.clone()) for x in lead]
    hp = U.hyper32(lr=3e-4, max_grad_norm=20.0)
    opt = torch.optim.Adam(params, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    wide = lambda x: np.repeat(x.numpy(), g, axis=0)     # noqa: E731
    P = [wide(x) for x in lead]
    M, V, t = [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P], 0
    coefs = []
    for step in range(5):
        scale = 0.1 if step in (1, 3) else 1.0
        row = U.random_rows(A, D, na, gen, scale).double().numpy()
        grads = U.row_to_tensors(row, na) + [scale * torch.randn((A, 3), generator=gen, dtype=torch.float64).numpy()]
        for p, x in zip(params, grads):
            p.grad = torch.from_numpy(x.reshape(A // g, g, *x.shape[1:]).sum(axis=1))
        norm_t = float(torch.nn.utils.clip_grad_norm_(params, hp["max_grad_norm"]))
        opt.step()
        P, M, V, t, norm, coef = S.shared_reference_step(P, grads, M, V, t, hp, g)
        coefs.append(coef)
        assert abs(norm - norm_t) <= 1e-12 * norm_t and t == step + 1
        for i, p in enumerate(params):
            st = opt.state[p]
            assert P[i].shape[0] == A
            assert _rel(P[i], wide(p.detach())) <= 1e-12, (step, i)
            assert _rel(M[i], wide(st["exp_avg"])) <= 1e-12 and _rel(V[i], wide(st["exp_avg_sq"])) <= 1e-12, (step, i)
            for a in range(A):                                   # members hold their leader's result
                assert np.array_equal(P[i][a], P[i][a // g * g]) and np.array_equal(M[i][a], M[i][a // g * g])
    assert [c < 1.0 for c in coefs] == [True, False, True, False, True], coefs
    if g == 1:                                                   # no sharing: adam_util.reference_step itself
        P1, M1, V1, *_ = U.reference_step([wide(x) for x in lead], grads, [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P], 0, hp)
        P2, M2, V2, *_ = S.shared_reference_step([wide(x) for x in lead], grads, [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P], 0, hp, 1)
        assert all(np.array_equal(a, b) for a, b in zip(P1 + M1 + V1, P2 + M2 + V2))


def test_the_host_group_sum_adds_in_agent_order_in_float32_and_so_does_the_torch_paths_install():
    """1 + 2^-24 + 2^-24: left to right in float32 both halves of an ulp are lost (ties to even), any other order or a wider
    accumulator gives 1 + 2^-23.  PPOLearner's torch path (install: the group sum on the leaders' .grad, +0 on the followers') adds
    in the same order: its rows equal leaders_rows bit for bit, on this example and on random rows."""
    import types
    from deep_rl_battlespace_amd.learner import PPOLearner
    row = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [5.0]], dtype=np.float32)
    assert S.group_sum32(row[:3].reshape(3, 1), 3).tolist() == [[1.0]]
    assert float(np.float32(row[1, 0] + row[2, 0]) + row[0, 0]) == 1.0 + 2.0 ** -23
    rows = S.leaders_rows(np.concatenate([row[:2], row[2:]]), 2)
    assert rows.dtype == np.float32 and rows[1, 0] == 0.0 and rows[3, 0] == 0.0 and not np.signbit(rows[1, 0])
    assert rows[0, 0] == np.float32(1.0) and rows[2, 0] == np.float32(5.0)
    gen = torch.Generator().manual_seed(13)
    for A, g, x in ((3, 3, torch.from_numpy(row[:3].copy())), (6, 3, U.random_rows(6, 11, 3, gen)), (4, 2, torch.randn(4, 3, generator=gen)),
                    (8, 8, U.random_rows(8, 14, 4, gen)), (4, 1, torch.randn(4, 3, generator=gen))):
        got = PPOLearner._group_sum(types.SimpleNamespace(group=g), x)
        assert got.dtype == torch.float32 and got.shape == x.shape
        assert np.array_equal(got.numpy().view(np.uint32), S.leaders_rows(x.numpy(), g).view(np.uint32)), (A, g)
    assert float(PPOLearner._group_sum(types.SimpleNamespace(group=3), torch.from_numpy(row[:3].copy()))[0, 0]) == 1.0
