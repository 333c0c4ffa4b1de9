"""CPU-side checks of the fused MLP on any input width and of its input gradient (bsx_mlp_forward, bsx_mlp_grad*, learner.fused_mlp /
mlp_grad): the header, the library and the binding agree on the three entry points and the ABI version stays; the workspace follows its
formula and is bsx_actor_grad's at (2n, 3n + 2); every refusal comes before any launch, in the header's order (fake addresses only: no
call here reaches a kernel); the rows the GPU tests leave out for ReLU kinks stay below the cap on every case of the table and on the
DDPG step, for the generator that is committed; the last case still makes its workgroups go round twice."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mlp_grad_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN = -1, -2
P, Q = 4096, 4096 + 8          # a 256-byte aligned fake address and one aligned to 8 bytes only (neither is dereferenced)
MAX_E, MAX_A, MAX_D = 1 << 30, 32, 64
NAMES = ("bsx_mlp_forward", "bsx_mlp_grad_workspace_bytes", "bsx_mlp_grad")


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
    assert re.search(r"#define BSX_MLP_MAX_D (\d+)", hdr).group(1) == "64" and L.MLP_MAX_D == 64
    assert len(L.SIGNATURES["bsx_mlp_forward"][1]) == 8 and len(L.SIGNATURES["bsx_mlp_grad"][1]) == 11
    # the entries that stay: their signatures are the ones they had
    assert len(L.SIGNATURES["bsx_actor_grad"][1]) == 9 and len(L.SIGNATURES["bsx_actor_forward"][1]) == 12
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import learner
    assert bsx.fused_mlp is learner.fused_mlp and bsx.mlp_grad is learner.mlp_grad
    assert "fused_mlp" in bsx.__all__ and "mlp_grad" in bsx.__all__


def test_workspace_bytes_follows_the_formula_and_is_the_actor_entrys_at_2n_and_3n_plus_2():
    L = _lib(); lib = L.load()
    b, b0 = L.c_size_t(0), L.c_size_t(0)
    rows = (1, 31, 32, 33, 127, 128, 129, 2048, 2049, 2100, 65536, 2097152, MAX_E)
    for A in (1, 2, 3, 4, 7, 31, 32):
        for D in (1, 5, 9, 32, 33, 64):
            G = 64 * D + 4096 + 6 * 64 + 260
            for Rr in rows:
                want = min(-(-(-(-Rr // 32)) // 4), max(1, 512 // A))           # ceil(ceil(R / 32) / 4), capped
                assert lib.bsx_mlp_grad_workspace_bytes(Rr, A, D, ctypes.byref(b)) == 0
                assert b.value == 4 * A * want * G, (Rr, A, D)
    for n in range(1, 17):
        for Rr in rows:
            assert lib.bsx_actor_grad_workspace_bytes(Rr, n, ctypes.byref(b0)) == 0
            assert lib.bsx_mlp_grad_workspace_bytes(Rr, 2 * n, 3 * n + 2, ctypes.byref(b)) == 0
            assert b.value == b0.value, (Rr, n)
    b = L.c_size_t(7)
    for Rr, A, D in ((0, 2, 9), (-5, 2, 9), (MAX_E + 1, 2, 9), (10, 0, 9), (10, MAX_A + 1, 9), (10, 2, 0), (10, 2, MAX_D + 1), (10, -1, 9), (10, 2, -1)):
        assert lib.bsx_mlp_grad_workspace_bytes(Rr, A, D, ctypes.byref(b)) == ARG and b.value == 7
    assert lib.bsx_mlp_grad_workspace_bytes(10, 2, 9, None) == ARG
    assert M.plan(2100, 32, 54) == (16, 2) and M.plan(2048, 32, 54) == (16, 1)      # the two-round case of the table
    assert M.plan(129, 3, 33) == (2, 1) and M.plan(1, 1, 1) == (1, 1)


def test_mlp_grad_refuses_before_any_launch_in_the_headers_order():
    lib = _lib().load()

    def grad(w=P, x=P, go=P, R=10, A=2, D=9, squash=1, grad=P, gx=P, ws=P):
        return lib.bsx_mlp_grad(w, x, go, R, A, D, squash, grad, gx, ws, None)

    cases = [(ARG, dict(x=None)), (ARG, dict(go=None)), (ARG, dict(grad=None)), (ARG, dict(ws=None)), (ARG, dict(squash=2)), (ARG, dict(squash=-1)),
             (ARG, dict(w=None)), (ARG, dict(R=0)), (ARG, dict(R=-1)), (ARG, dict(R=MAX_E + 1)), (ARG, dict(A=0)), (ARG, dict(A=MAX_A + 1)),
             (ARG, dict(D=0)), (ARG, dict(D=MAX_D + 1)),
             (ALIGN, dict(w=Q)), (ALIGN, dict(go=Q)), (ALIGN, dict(x=P + 2)), (ALIGN, dict(grad=P + 2)), (ALIGN, dict(gx=P + 2)), (ALIGN, dict(ws=P + 1))]
    # the same with no grad_x: a null grad_x is an argument, not a refusal -- checked through the refusals that come after it
    cases += [(ALIGN, dict(gx=None, ws=P + 1)), (ARG, dict(gx=None, D=MAX_D + 1))]
    # two rules broken at once: every BSX_E_ARG before every BSX_E_ALIGN
    cases += [(ARG, dict(x=None, w=Q)), (ARG, dict(squash=2, go=Q)), (ARG, dict(R=0, w=Q)), (ARG, dict(A=0, ws=P + 1)), (ARG, dict(D=65, gx=P + 2)),
              (ARG, dict(w=None, go=Q)), (ALIGN, dict(w=Q, go=Q)), (ALIGN, dict(go=Q, x=P + 2, gx=P + 2))]
    for want, kw in cases:
        assert grad(**kw) == want, kw


def test_mlp_forward_refuses_before_the_launch_in_the_headers_order():
    lib = _lib().load()

    def fwd(w=P, x=P, y=P, raw=P, R=10, A=2, D=9):
        return lib.bsx_mlp_forward(w, x, y, raw, R, A, D, None)

    cases = [(ARG, dict(x=None)), (ARG, dict(y=None)), (ARG, dict(w=None)), (ARG, dict(R=0)), (ARG, dict(R=MAX_E + 1)), (ARG, dict(A=0)),
             (ARG, dict(A=MAX_A + 1)), (ARG, dict(D=0)), (ARG, dict(D=MAX_D + 1)),
             (ALIGN, dict(w=Q)), (ALIGN, dict(y=Q)), (ALIGN, dict(x=P + 2)), (ALIGN, dict(raw=P + 2)),
             (ALIGN, dict(raw=None, x=P + 1)), (ARG, dict(raw=None, A=33)),
             (ARG, dict(x=None, w=Q)), (ARG, dict(D=65, y=Q)), (ARG, dict(w=None, y=Q)), (ALIGN, dict(w=Q, raw=P + 2))]
    for want, kw in cases:
        assert fwd(**kw) == want, kw


def test_the_entries_that_stay_keep_their_ranges():
    L = _lib(); lib = L.load()
    g = L.c_int(-1)
    assert lib.bsx_actor_blob_floats(51, ctypes.byref(g)) == ARG and lib.bsx_actor_grad_floats(51, ctypes.byref(g)) == ARG and g.value == -1
    assert lib.bsx_actor_grad(P, P, P, 10, 17, 1, P, P, None) == ARG
    assert lib.bsx_actor_forward(P, P, P, 10, 17, 0, None, 0, 0, None, 0, None) == ARG


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_the_rows_left_out_for_relu_kinks_stay_below_the_cap(case):
    net, x, go, share = M.build(case)
    A, D, na, sq, rows, var = case
    print(M.case_id(case), "largest per-agent share", float(share.max()))
    assert float(share.max()) <= M.KINK_CAP, share
    assert x.shape == (rows, A, D) and go.shape == (rows, A, na) and float(x.min()) >= -1.0 and float(x.max()) <= 1.0
    assert np.allclose((go == 0).all(-1).double().mean(0).numpy(), share)
    off = any(bool((getattr(net, k) != v).any()) for k, v in (("g1", 1.0), ("g2", 1.0), ("h1", 0.0), ("h2", 0.0)))
    assert off == (var == "gains")


def test_the_ddpg_step_leaves_out_at_most_the_cap_and_its_reference_reaches_every_tensor():
    actor, critic, obs, act, target, w, share = M.ddpg_case()
    print("ddpg rows left out", share)
    assert share <= M.KINK_CAP and np.isclose(float((w == 0).double().mean()), share)
    assert obs.shape == (96, 2, 5) and actor.n_actions == 4 and critic.obs_len == 9 and critic.n_actions == 1
    ga, gc = M.ddpg_grads(actor, critic, obs, act, target, w, torch.float64)
    assert all(np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0 for g in (ga, gc) for k in M.PARAMS)


def test_the_recorded_factors_are_the_rule_applied_to_the_recorded_spread_of_the_yardstick():
    """profiles/mlp_input_grad.json: every factor other than the project's (2, 4) must follow from a spread of the float32 yardstick
    itself that the same file records (mlp_grad_util.exceptions_from); nothing else may widen a bound."""
    import json
    rec = json.load(open(M.PROFILE))
    sp = {k: v for k, v in rec["yardstick_spread"].items() if k != "what"}
    assert set(sp) == {"torch_gpu", "unit_permutation", "row_permutation"}
    assert all(M.case_id(c) in s for s in sp.values() for c in M.CASES)
    assert rec["factors"]["default"] == [M.FM, M.FX] == [2.0, 4.0]
    assert rec["factors"]["exceptions"] == M.exceptions_from(sp)
    assert all(set(t) <= {"b3"} for cid, t in rec["factors"]["exceptions"].items() if cid == "*")
    assert M.factor_rule(3.99, 1.99) == (2.0, 4.0) and M.factor_rule(4.0, 1.0) == (2.0, 8.0) and M.factor_rule(1.0, 3.0) == (6.0, 4.0)
    # what the card measured stays on record next to them, missed bounds included
    assert all(M.case_id(c) in rec["kernel"] for c in M.CASES) and "timing" in rec


def test_fused_mlp_and_mlp_grad_refuse_cpu_tensors():
    from deep_rl_battlespace_amd.learner import fused_mlp, mlp_grad
    from deep_rl_battlespace_amd.rollout import StackedActor
    net, x = StackedActor(3, 7, 1), torch.rand((4, 3, 7))
    with pytest.raises(ValueError, match="CUDA"):
        fused_mlp(net, x, squash=False)
    with pytest.raises(ValueError, match="CUDA"):
        mlp_grad(net, net.pack(), x, torch.zeros((4, 3, 1)), squash=False)
