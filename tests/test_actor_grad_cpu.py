"""CPU-side checks of the actor's fused training pass (bsx_actor_grad*, learner.fused_apply / categorical_log_prob): the header, the
library and the binding agree on the three entry points; sizes follow their formulas; every refusal comes before any launch, in the
documented order (fake addresses only: no call here reaches a kernel); the conditions the GPU tests' float64 bounds rest on -- the share
of rows left out for ReLU kinks, the spread of the float32 yardstick under row permutations -- hold on the reference alone, at every team
size from 1 to 16 and on the two many-row inputs; the row counts of the multi-round cases still make the workgroups go round more than
once, and the wide teams still have D > 32, by the library's own workspace size; a gradient row
splits into the ten parameter shapes where torch.cat would put them; the learner-side categorical head equals torch.distributions."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import actor_grad_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN = -1, -2
P, M = 4096, 4096 + 8          # a 256-byte aligned fake address and one aligned to 8 bytes only (neither is dereferenced)
MAX_E, MAX_N = 1 << 30, 16
NAMES = ("bsx_actor_grad_floats", "bsx_actor_grad_workspace_bytes", "bsx_actor_grad")


def _lib():
    from deep_rl_battlespace_amd import _lib as L
    return L


def test_entry_points_are_declared_exported_and_bound_and_the_abi_version_stays():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert name in L.SIGNATURES
        assert hasattr(L.load(), name)
    assert re.search(r"#define BSX_ABI_VERSION (\d+)", hdr).group(1) == "14" and L.load().bsx_abi_version() == 14 and L.ABI_VERSION == 14
    assert len(L.SIGNATURES["bsx_actor_grad"][1]) == 9
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import learner
    assert bsx.fused_apply is learner.fused_apply and bsx.categorical_log_prob is learner.categorical_log_prob


def test_grad_floats_is_the_formula_for_every_team_size():
    L = _lib(); lib = L.load()
    from deep_rl_battlespace_amd import learner
    for n in range(1, MAX_N + 1):
        D, g = 3 * n + 2, L.c_int(-1)
        assert lib.bsx_actor_grad_floats(D, ctypes.byref(g)) == 0
        assert g.value == 64 * D + 4096 + 6 * 64 + 260 == learner.grad_floats(D)
    g = L.c_int(-1)
    for bad in (0, -1, 3 * MAX_N + 3):
        assert lib.bsx_actor_grad_floats(bad, ctypes.byref(g)) == ARG and g.value == -1
    assert lib.bsx_actor_grad_floats(5, None) == ARG


def test_workspace_bytes_is_positive_monotone_in_rows_bounded_and_refuses_what_the_contract_says():
    L = _lib(); lib = L.load()
    b = L.c_size_t(0)
    for n in (1, 2, 4, 10, 11, MAX_N):
        last = 0
        G = 64 * (3 * n + 2) + 4740
        for R in (1, 31, 32, 33, 127, 128, 129, 5000, 65536, 2097152, MAX_E):
            assert lib.bsx_actor_grad_workspace_bytes(R, n, ctypes.byref(b)) == 0
            assert b.value > 0 and b.value >= last and b.value % (4 * 2 * n * G) == 0
            assert b.value <= 512 * G * 4                      # at most 512 partial rows over all agents: 16 MB
            last = b.value
    b = L.c_size_t(7)
    for R, n in ((0, 1), (-5, 1), (MAX_E + 1, 1), (10, 0), (10, MAX_N + 1)):
        assert lib.bsx_actor_grad_workspace_bytes(R, n, ctypes.byref(b)) == ARG and b.value == 7
    assert lib.bsx_actor_grad_workspace_bytes(10, 1, None) == ARG


def test_the_workspace_is_the_mlp_entrys_at_2n_agents_and_3n_plus_2_inputs_and_both_refuse_the_same_sizes():
    """bsx_actor_grad_workspace_bytes(R, n) delegates to bsx_mlp_grad_workspace_bytes(R, 2n, 3n + 2): the same bytes at every (n, rows)
    the GPU tests run -- CASES at their dense row count, LARGE -- and at one row; BSX_E_ARG from both for a team size or a row count
    out of range.  Size queries: no GPU is touched."""
    L = _lib(); lib = L.load()
    sizes = {(c[1], 5001 - 2 * c[1]) for c in U.CASES} | set(U.LARGE) | {(n, 1) for n in range(1, MAX_N + 1)}
    for n, rows in sorted(sizes):
        a, b = L.c_size_t(0), L.c_size_t(1)
        assert lib.bsx_actor_grad_workspace_bytes(rows, n, ctypes.byref(a)) == 0
        assert lib.bsx_mlp_grad_workspace_bytes(rows, 2 * n, 3 * n + 2, ctypes.byref(b)) == 0
        assert a.value == b.value > 0, (n, rows)
    for n, rows in ((0, 10), (MAX_N + 1, 10), (1, 0)):
        a, b = L.c_size_t(7), L.c_size_t(7)
        assert lib.bsx_actor_grad_workspace_bytes(rows, n, ctypes.byref(a)) == ARG and a.value == 7
        assert lib.bsx_mlp_grad_workspace_bytes(rows, 2 * n, 3 * n + 2, ctypes.byref(b)) == ARG and b.value == 7


def test_actor_grad_refuses_before_any_launch_in_the_documented_order():
    lib = _lib().load()

    def grad(w=P, obs=P, go=P, R=10, n=1, squash=1, grad=P, ws=P):
        return lib.bsx_actor_grad(w, obs, go, R, n, squash, grad, ws, None)

    cases = [(ARG, dict(obs=None)), (ARG, dict(go=None)), (ARG, dict(grad=None)), (ARG, dict(ws=None)), (ARG, dict(squash=2)), (ARG, dict(squash=-1)),
             (ARG, dict(w=None)), (ARG, dict(R=0)), (ARG, dict(R=-1)), (ARG, dict(R=MAX_E + 1)), (ARG, dict(n=0)), (ARG, dict(n=MAX_N + 1)),
             (ALIGN, dict(w=M)), (ALIGN, dict(go=M)), (ALIGN, dict(obs=P + 2)), (ALIGN, dict(grad=P + 2)), (ALIGN, dict(ws=P + 1))]
    # two rules broken at once: which check comes first is part of the contract (every BSX_E_ARG before every BSX_E_ALIGN)
    cases += [(ARG, dict(obs=None, w=M)), (ARG, dict(squash=2, go=M)), (ARG, dict(R=0, w=M)), (ARG, dict(n=0, ws=P + 1)), (ARG, dict(w=None, go=M)),
              (ALIGN, dict(w=M, go=M)), (ALIGN, dict(go=M, obs=P + 2, grad=P + 2))]
    for want, kw in cases:
        assert grad(**kw) == want, kw


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_the_rows_left_out_for_relu_kinks_stay_below_the_cap(case):
    """go = 0 on the rows with a hidden unit within 1e-4 of its kink (float64 reference): at most 5 % of every agent's rows, so that the
    gradients the GPU tests compare are still those of (nearly) the whole batch."""
    actor, obs, go, g64, g32, share = U.reference(case)
    print(U.case_id(case), "largest per-agent share", float(share.max()))
    assert float(share.max()) <= U.KINK_CAP, share
    assert obs.shape[0] == 5001 - 2 * case[1] and actor.n_actions == case[2]
    zero_rows = (go == 0).all(-1).double().mean(0).numpy()
    assert np.allclose(zero_rows, share)
    assert all(np.isfinite(g64[k]).all() and np.abs(g64[k]).max() > 0 for k in U.PARAMS)
    recorded = json.load(open(U.PROFILE))
    assert U.case_id(case) in recorded["cases"]


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_the_factors_cover_what_row_order_alone_does_to_the_float32_yardstick(case):
    """The bound of the GPU tests is a multiple of the float32 yardstick's own error; the yardstick under 8 row permutations (the same
    network, the same rows, another summation order) must itself stay inside that multiple, or the bound would reject a correct float32
    implementation.  (2, 4) is the project's pair (actor_ref_util.F32_FACTORS); b3 has 4 A values or fewer and moves by more: its factors
    are twice its recorded spread (profiles/actor_grad_float64.json)."""
    spread = U.permutation_spread(case, 8)
    f = U.factors()
    for k in U.PARAMS:
        print(U.case_id(case), k, "max moved by %.2f, mean by %.2f" % spread[k])
        assert spread[k][0] < f[k][1] and spread[k][1] < f[k][0], (k, spread[k], f[k])
        if k != "b3":
            assert f[k] == (2.0, 4.0)


@pytest.mark.parametrize("n,rows", U.LARGE, ids=lambda v: str(v))
def test_the_many_row_inputs_meet_the_same_two_conditions(n, rows):
    """The (n, rows) pairs of actor_grad_util.LARGE: the kink share below the cap and the yardstick's spread inside the factors, as above."""
    ref = U.reference_large(n, rows)
    actor, obs, go, g64, g32, share = ref
    print("large", n, rows, "largest per-agent share", float(share.max()))
    assert obs.shape == (rows, 2 * n, 3 * n + 2) and float(share.max()) <= U.KINK_CAP, share
    assert np.allclose((go == 0).all(-1).double().mean(0).numpy(), share)
    assert bool((obs[::7] == -1.0).all()) and all(np.isfinite(g64[k]).all() and np.abs(g64[k]).max() > 0 for k in U.PARAMS)
    spread = U.permutation_spread(ref, 8)
    f = U.factors()
    for k in U.PARAMS:
        print("large", n, rows, k, "max moved by %.2f, mean by %.2f" % spread[k])
        assert spread[k][0] < f[k][1] and spread[k][1] < f[k][0], (k, spread[k], f[k])


def test_the_multi_round_cases_still_go_round_twice_and_the_wide_teams_still_take_the_two_tile_kernel():
    """bsx_actor_grad caps the workgroups per agent, and a workgroup takes four 32-row tiles per round: P workgroups per agent (read back
    from the workspace size: bytes / (2n G 4)) make ceil(ceil(R / 32) / (4 P)) rounds.  The cases the GPU tests count on for the round loop
    (accumulators kept across rounds, LDS images overwritten, a last round that is mostly beyond R) must have rounds >= 2 at their row
    counts, and the cases they count on for the two-tile dW1 kernel D = 3n + 2 > 32: a later change of the cap has to move these row
    counts with it."""
    rounds = {}
    for case in U.CASES:
        rows, n = 5001 - 2 * case[1], case[1]
        P, rounds[case] = U.plan(rows, 2 * n, 3 * n + 2)
        assert 1 <= P <= 512 // (2 * n)
        print(U.case_id(case), "rows", rows, "workgroups per agent", P, "rounds", rounds[case])
    assert {c[1] for c in U.MULTI_ROUND} == {8, 10, 11, 13, 16}
    assert all(rounds[c] >= 2 for c in U.MULTI_ROUND)
    assert all(rounds[c] == 3 for c in U.CASES if c[1] == 16) and sum(c[1] == 16 for c in U.CASES) == 2
    assert all(rounds[c] == 1 for c in U.CASES if c[1] <= 5)                       # the one-round path keeps its cases too
    wide = [c for c in U.CASES if c[1] >= 11]
    assert len(wide) == 5 and all(3 * c[1] + 2 > 32 for c in wide) and {3 * c[1] + 2 for c in U.CASES if 5 <= c[1] <= 10} == {17, 26, 32}
    for n, rows in U.LARGE:
        P, r = U.plan(rows, 2 * n, 3 * n + 2)
        print("large", n, rows, "workgroups per agent", P, "rounds", r)
        assert r == 2 and P == 512 // (2 * n)
    assert U.plan(33000, 2, 5)[0] == 256                                           # the merge kernel's widest input
    # the ragged, appended-rows, layout and graph legs at 16 a side (tests/test_hip_actor_grad.py)
    assert U.plan(2048, 32, 50) == (16, 1) and U.plan(2049, 32, 50) == (16, 2) and U.plan(2081, 32, 50) == (16, 2) and U.plan(2100, 32, 50) == (16, 2)
    assert U.plan(257, 22, 35)[1] == 1 and U.plan(300, 32, 50)[1] == 1


def test_a_gradient_row_splits_where_cat_of_the_flattened_parameters_puts_it():
    from deep_rl_battlespace_amd import learner
    from deep_rl_battlespace_amd.rollout import StackedActor
    for n, na in ((1, 4), (2, 3), (1, 1), (4, 4), (11, 3)):
        A, D = 2 * n, 3 * n + 2
        G = learner.grad_floats(D)
        row = torch.arange(A * G, dtype=torch.float32).reshape(A, G)
        parts = learner.split_grad(row, na)
        full = StackedActor(A, D, 4)                               # the row's layout: the ten tensors of a 4-column network, flattened
        assert torch.cat([getattr(full, k).detach().reshape(A, -1) for k in learner.PARAMS], dim=1).shape == (A, G)
        o = 0
        actor = StackedActor(A, D, na)
        for k, g in zip(learner.PARAMS, parts):
            p4 = getattr(full, k)
            seg = row[:, o:o + p4[0].numel()].reshape(p4.shape)
            o += p4[0].numel()
            assert g.shape == getattr(actor, k).shape, (k, g.shape)
            assert torch.equal(g, seg[..., :g.shape[-1]]), k
            assert g.data_ptr() == seg.data_ptr()                  # a view: no gather
        assert o == G
    with pytest.raises(ValueError):
        learner.split_grad(torch.zeros((2, 5061)), 4)


def test_categorical_log_prob_is_the_categorical_distribution_of_the_squashed_scores():
    from deep_rl_battlespace_amd.learner import categorical_log_prob
    from deep_rl_battlespace_amd.rollout import StackedActor
    torch.manual_seed(3)
    n, T, E = 2, 3, 50
    A, D = 2 * n, 3 * n + 2
    actor = StackedActor(A, D, 4)
    with torch.no_grad():
        actor.w3.mul_(60.0)
    obs = torch.rand((T, E, A, D)) * 2 - 1
    actions = torch.randint(0, 4, (T, E, A))
    for tau in (1.0, 0.5):
        logp, ent = categorical_log_prob(actor, obs, actions, temperature=tau)
        assert logp.shape == ent.shape == (T, E, A)
        with torch.no_grad():
            dist = torch.distributions.Categorical(logits=actor(obs.reshape(-1, A, D)).reshape(T, E, A, 4) / tau)
        torch.testing.assert_close(logp, dist.log_prob(actions), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(ent, dist.entropy(), rtol=1e-6, atol=1e-6)
        every = torch.stack([categorical_log_prob(actor, obs, torch.full_like(actions, k), temperature=tau)[0] for k in range(4)], -1)
        torch.testing.assert_close(every.exp().sum(-1), torch.ones((T, E, A)), rtol=0, atol=1e-6)
    logp.sum().backward()                                          # differentiable in the actor's parameters
    assert all(getattr(actor, k).grad is not None for k in U.PARAMS)
    with pytest.raises(ValueError):
        categorical_log_prob(actor, obs, actions, temperature=0.0)


def test_the_fused_paths_refuse_cpu_tensors():
    from deep_rl_battlespace_amd.learner import categorical_log_prob, fused_apply
    from deep_rl_battlespace_amd.rollout import StackedActor, gaussian_log_prob
    n, E = 1, 7
    A, D = 2 * n, 3 * n + 2
    obs = torch.rand((E, A, D))
    with pytest.raises(ValueError, match="CUDA"):
        fused_apply(StackedActor(A, D, 4), obs)
    with pytest.raises(ValueError, match="CUDA"):
        fused_apply(StackedActor(A, D, 1), obs, squash=False)
    with pytest.raises(ValueError, match="CUDA"):
        categorical_log_prob(StackedActor(A, D, 4), obs, torch.zeros((E, A), dtype=torch.int64), fused=True)
    with pytest.raises(ValueError, match="CUDA"):
        gaussian_log_prob(StackedActor(A, D, 3), torch.zeros((A, 3)), obs, torch.zeros((E, A, 4)), fused=True)
    # the default path is untouched by the new argument
    a3 = StackedActor(A, D, 3)
    lp0, en0 = gaussian_log_prob(a3, torch.zeros((A, 3)), obs, torch.zeros((E, A, 4)))
    lp1, en1 = gaussian_log_prob(a3, torch.zeros((A, 3)), obs, torch.zeros((E, A, 4)), fused=False)
    assert torch.equal(lp0, lp1) and torch.equal(en0, en1)
