"""The actor's fused training pass on the MI355X (bsx_actor_grad, learner.fused_apply): every parameter gradient against float64 autograd at
a small multiple of what float32 autograd itself loses on the same inputs (tests/actor_grad_util.py: ReLU kinks left out by construction,
factors from profiles/actor_grad_float64.json), at team sizes from 1 to 16 -- both dW1 forms of the kernel, D <= 32 (up to exactly 32) and
D > 32 -- and at row counts that make a workgroup go round its tile loop once, twice and three times, the many-row regime at the
workgroup cap among them; the layout of the gradient row; ragged row counts between guard slabs, on both sides of the first second
round; the same bits on every call and from a captured graph, at 2 and at 16 a side; a PPO loss on a continuous and a discrete rollout
record, fused path against torch path; the learner-side log-probabilities against the rollout's recorded ones."""
import functools
import math

import numpy as np
import pytest
import torch

import actor_grad_util as U
import actor_ref_util as R
import ppo_learner_util as L
import yardstick_util as Y
from actor_grad_util import _logp, _ppo, _ppo_ladder, _ppo_own_error, _to
from guard_util import Buffers

pytestmark = pytest.mark.gpu

LOGP_TOL = 1e-4                   # recorded logp against the float32 torch head: tests/test_hip_gaussian_head.py (assert_close(logp, want_lp, atol=1e-4))
RAGGED = (1, 31, 32, 33, 63, 65, 255, 257)
# (rows, n).  n = 16: 16 workgroups per agent, so 2 048 rows are the last one-round size and 2 049 is ONE valid row in round 2 (every
# other lane of that round reads row R - 1 with grad_out = 0); n = 11: the two-tile dW1 kernel below and above a workgroup's 128 rows
RAGGED_CASES = [(r, n) for n in (1, 4) for r in RAGGED] + [(r, 16) for r in (1, 33, 2047, 2048, 2049, 2081)] + [(31, 11), (257, 11)]


def _fused_grads(actor_cpu, obs_cpu, go_cpu, squash):
    from deep_rl_battlespace_amd.learner import fused_apply
    actor, obs, go = _to(actor_cpu), obs_cpu.to("cuda").contiguous(), go_cpu.to("cuda")
    y = fused_apply(actor, obs, squash=squash)
    (y * go).sum().backward()
    torch.cuda.synchronize()
    return actor, obs, y.detach(), {k: getattr(actor, k).grad.double().cpu().numpy() for k in U.PARAMS}


# ---------------------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_gradients_stay_within_the_float32_yardstick_of_float64_autograd(case):
    from deep_rl_battlespace_amd.rollout import FusedActor
    actor_cpu, obs_cpu, go, g64, g32, share = U.reference(case)
    assert float(share.max()) <= U.KINK_CAP
    n, na, squash = case[1], case[2], case[3]
    actor, obs, y, got = _fused_grads(actor_cpu, obs_cpu, go, squash)
    assert y.shape == (obs.shape[0], 2 * n, na)
    # the forward is the rollout's own float32 kernel: FusedActor's bits
    fa = FusedActor(actor, n)
    scores = torch.full((*obs.shape[:2], 4), 7.0, device="cuda")
    if squash:
        fa.forward_into(obs, scores, seq=1)
        assert torch.equal(y, scores[..., :na])
        assert na == 4 or bool((scores[..., na:] == 0).all())
    else:
        out = torch.full(obs.shape[:2], 7.0, device="cuda")
        fa.forward_into(obs, scores, seq=1, value=dict(weights=actor.pack(), out=out))
        assert torch.equal(y[..., 0], out)
    U.check(got, g64, g32, "KERNEL " + U.case_id(case))


@pytest.mark.parametrize("n,rows", U.LARGE)
def test_many_rows_at_the_workgroup_cap_keep_the_float64_bound_over_two_rounds(n, rows):
    """The regime the kernel was written for, at the smallest size that reaches it: 512 / (2n) workgroups per agent, each going round
    twice (tests/test_actor_grad_cpu.py derives both from the workspace size), the second round nearly empty; at n = 1 the merge kernel
    adds 256 partial rows per agent.  The same reference, yardstick and factors as above."""
    actor_cpu, obs_cpu, go, g64, g32, share = U.reference_large(n, rows)
    assert float(share.max()) <= U.KINK_CAP and U.plan(rows, 2 * n, 3 * n + 2) == (512 // (2 * n), 2)
    actor, obs, y, got = _fused_grads(actor_cpu, obs_cpu, go, True)
    assert y.shape == (rows, 2 * n, 4)
    U.check(got, g64, g32, f"LARGE n={n} rows={rows}")


# ---------------------------------------------------------------------------------------------------- 2. layout
def _one_column_of_one_agent(n, Rr, agent, col):
    actor_cpu, obs = R.fresh(n)
    obs = obs[:Rr].contiguous()
    go = torch.zeros((Rr, 2 * n, 4))
    go[:, agent, col] = torch.randn(Rr, generator=torch.Generator().manual_seed(1))
    actor, _, _, got = _fused_grads(actor_cpu, obs, go, True)
    for k in U.PARAMS:
        g = got[k]
        others = np.delete(g, agent, axis=0)
        assert not others.any(), k                                  # exactly 0, not small
        assert np.abs(g[agent]).max() > 0, k
    for k in ("w3", "b3"):
        assert not np.delete(got[k][agent], col, axis=-1).any(), k
    g64 = U.autograd_grads(actor_cpu, obs, go, True, torch.float64)
    for k in U.PARAMS:
        assert np.abs(got[k] - g64[k]).max() <= 1e-5 * np.abs(g64[k]).max(), k
    return got


def test_one_column_of_one_agent_reaches_only_that_agents_row_and_that_head_column():
    _one_column_of_one_agent(4, 300, 5, 2)


def test_one_column_of_one_agent_of_sixteen_a_side_reaches_only_its_row_and_all_fifty_input_rows_of_w1():
    """D = 50: the two-tile dW1 kernel; w1's rows k = 32 .. 49 come from the waves' upper tiles and are held to float64 like the rest."""
    got = _one_column_of_one_agent(16, 300, 21, 2)
    assert got["w1"].shape == (32, 50, 64) and bool((np.abs(got["w1"][21]).max(-1) > 0).all())


# ---------------------------------------------------------------------------------------------------- 3. ragged sizes, guards
def _raw_call(actor, obs, go4, squash=1, guarded=True):
    """bsx_actor_grad on guarded buffers: (grad [A, G] clone, names of the buffers with a damaged guard, workspace bytes)."""
    from deep_rl_battlespace_amd import _lib
    from deep_rl_battlespace_amd.learner import grad_floats
    lib = _lib.load()
    Rr, A, D = obs.shape
    n = A // 2
    nb = _lib.c_size_t()
    _lib.check(lib.bsx_actor_grad_workspace_bytes(Rr, n, _lib.ctypes.byref(nb)), "bsx_actor_grad_workspace_bytes")
    B = Buffers(guarded)
    o = B("obs", (Rr, A, D), torch.float32); o.copy_(obs)
    g = B("grad_out", (Rr, A, 4), torch.float32); g.copy_(go4)
    out = B("grad", (A, grad_floats(D)), torch.float32, init=7.0)
    ws = B("workspace", (nb.value // 4,), torch.float32, init=7.0)
    blob = actor.pack()
    _lib.check(lib.bsx_actor_grad(blob.data_ptr(), o.data_ptr(), g.data_ptr(), Rr, n, squash, out.data_ptr(), ws.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream), "bsx_actor_grad")
    torch.cuda.synchronize()
    return out.clone(), B.stray(), nb.value


@pytest.mark.parametrize("rows,n", RAGGED_CASES)
def test_ragged_row_counts_keep_their_guards_and_the_float64_bound(rows, n):
    from deep_rl_battlespace_amd.learner import split_grad
    case = ("fresh" if n <= 4 else "trained_like", n, 4, True)
    actor_cpu, obs, go, g64, g32, _ = U.reference(case, rows)
    assert obs.shape[0] == rows
    actor = _to(actor_cpu)
    grad, stray, _ = _raw_call(actor, obs.to("cuda"), go.to("cuda"))
    assert not stray, stray
    got = {k: g.double().cpu().numpy() for k, g in zip(U.PARAMS, split_grad(grad, 4))}
    U.check(got, g64, g32, f"RAGGED rows={rows} n={n}")


@pytest.mark.parametrize("n", [1, 4, 16])
def test_rows_appended_with_zero_gradient_change_no_bit_when_the_grid_is_the_same(n):
    # 9 and 10 tiles: three workgroups per agent either way; n = 16: 65 and 66 tiles on 16 workgroups, the appended rows in round 2
    rows, more = (2049, 2100) if n == 16 else (257, 300)
    actor_cpu, obs_all = R.fresh(n)
    actor = _to(actor_cpu)
    go = torch.randn((more, 2 * n, 4), generator=torch.Generator().manual_seed(2))
    go[rows:] = 0.0
    a, stray_a, ws_a = _raw_call(actor, obs_all[:rows].to("cuda"), go[:rows].to("cuda"))
    b, stray_b, ws_b = _raw_call(actor, obs_all[:more].to("cuda"), go.to("cuda"))
    assert ws_a == ws_b                                             # the same number of partial rows: the same partition of the tiles
    assert not stray_a and not stray_b
    assert torch.equal(a, b)
    assert bool((a != 7.0).all())                                   # grad is overwritten everywhere


# ---------------------------------------------------------------------------------------------------- 4. determinism, graphs
def _same_bits_eagerly_and_from_a_graph(n, Rr):
    from deep_rl_battlespace_amd.learner import fused_apply, fused_grad, split_grad
    from deep_rl_battlespace_amd.rollout import FusedActor
    actor_cpu, obs = R.fresh(n, outputs=3)
    actor, obs = _to(actor_cpu), obs[:Rr].to("cuda").contiguous()
    go = torch.randn((Rr, 2 * n, 3), device="cuda")

    def step():
        for k in U.PARAMS:
            getattr(actor, k).grad = None
        y = fused_apply(actor, obs)
        (y * go).sum().backward()
        return y.detach()
    y1 = step().clone(); g1 = [getattr(actor, k).grad.clone() for k in U.PARAMS]
    y2 = step().clone(); g2 = [getattr(actor, k).grad.clone() for k in U.PARAMS]
    torch.cuda.synchronize()
    assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    # the same step as a captured graph: pack, forward and the backward call, enqueued on the capturing stream
    fa = FusedActor(actor, n)
    scores = torch.zeros((Rr, 2 * n, 4), device="cuda")

    def calls():
        fa.refresh()
        fa.forward_into(obs, scores, seq=1)
        return fused_grad(actor, fa.weights, obs, go, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        calls()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        row = calls()
    for _ in range(2):
        row.zero_(); scores.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(scores[..., :3], y1)
        for k, a, b in zip(U.PARAMS, split_grad(row, 3), g1):
            assert torch.equal(a, b), k
    # the backward reads the blob the forward packed: parameters moved in between do not reach it
    for k in U.PARAMS:
        getattr(actor, k).grad = None
    y = fused_apply(actor, obs)
    with torch.no_grad():
        for k in U.PARAMS:
            getattr(actor, k).mul_(1.5)
    (y * go).sum().backward()
    torch.cuda.synchronize()
    for k, b in zip(U.PARAMS, g1):
        assert torch.equal(getattr(actor, k).grad, b), k


def test_the_same_inputs_give_the_same_bits_eagerly_and_from_a_captured_graph():
    _same_bits_eagerly_and_from_a_graph(2, 1000)


def test_sixteen_a_side_over_two_rounds_gives_the_same_bits_eagerly_and_from_a_captured_graph():
    assert U.plan(2100, 32, 50)[1] == 2
    _same_bits_eagerly_and_from_a_graph(16, 2100)


def test_fused_apply_refuses_what_it_documents():
    from deep_rl_battlespace_amd.learner import fused_apply
    from deep_rl_battlespace_amd.rollout import StackedActor
    A, D = 2, 5
    obs = torch.rand((9, A, D), device="cuda")
    actor = StackedActor(A, D, 4, device="cuda")
    with pytest.raises(ValueError, match="float32"):
        fused_apply(actor, obs.double())
    with pytest.raises(ValueError, match="float32"):
        fused_apply(StackedActor(A, D, 4, device="cuda", dtype=torch.float64), obs)
    with pytest.raises(ValueError, match="require"):
        fused_apply(actor, obs.clone().requires_grad_())
    with pytest.raises(ValueError, match="64"):
        fused_apply(StackedActor(A, D, 4, fc1_dims=32, device="cuda"), obs)
    with pytest.raises(ValueError, match="value head"):
        fused_apply(actor, obs, squash=False)
    with pytest.raises(ValueError, match="CUDA"):
        fused_apply(actor, obs.cpu())
    with pytest.raises(ValueError):
        fused_apply(actor, obs[:, :, :4])
    assert fused_apply(actor, obs.reshape(3, 3, A, D)).shape == (3, 3, A, 4)


# ---------------------------------------------------------------------------------------------------- 5. end to end: a PPO loss
@functools.lru_cache(maxsize=None)
def _record(kind):
    """ppo_learner_util's small rollout (n = 1, E = 96, T = 8, with GAE): the records a PPO update reads, on the CPU (read-only), and the
    networks that produced them."""
    ro = L.small_rollout(kind)
    return ro.actor, ro.value_actor, ro.log_std, L.record(ro)


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_ppo_loss_and_gradients_fused_against_torch_on_a_rollout_record(kind):
    actor0, critic, ls, rec = _record(kind)
    # the learner is a step of actor_grad_util's ladder away from the policy that played; the same kept rows in every path
    actor, critic, ls_cpu, keep, fig = _ppo_ladder(actor0, critic, ls, rec, kind)
    kept, clipped = fig["kept"], fig["clipped"]
    assert kept >= 0.9 * fig["masked"] and kept >= 500 and 0.05 * kept <= clipped <= 0.6 * kept
    L64, a64, c64, l64, _ = _ppo(actor, critic, ls_cpu, rec, keep, kind, False, "cpu", torch.float64)
    L32, a32, c32, l32, _ = _ppo(actor, critic, ls_cpu, rec, keep, kind, False, "cpu", torch.float32)
    # what the torch path itself loses on this record: the float32 loss in the given order and under 8 others, against float64
    Lt, bound, e_ls = _ppo_own_error(actor, critic, ls_cpu, rec, keep, kind, L64, l64)
    Lf, af, cf, lf, _ = _ppo(actor, critic, ls_cpu, rec, keep, kind, True, "cuda", torch.float32)
    print(kind, f"loss float64 {L64:.9g} fused {Lf:.9g} torch {Lt:.9g}; |fused - torch| {abs(Lf - Lt):.3e}, |fused - f64| {abs(Lf - L64):.3e}, "
                f"torch's own error (max of 9 row orders, at least half a float32 spacing) {bound / Y.FACTORS[1]:.3e}")
    # both are float32 evaluations of the same loss, each off float64 by about torch's own error: yardstick_util.scalar_bound of it
    assert abs(Lf - Lt) <= bound and abs(Lf - L64) <= bound
    U.check(af, a64, a32, f"PPO {kind} actor")
    U.check(cf, c64, c32, f"PPO {kind} critic")
    if ls is not None:
        print(kind, f"log_std gradient: |fused - f64| {np.abs(lf - l64).max():.3e}, torch's own error {e_ls:.3e}, max |g| {np.abs(l64).max():.3e}")
        assert np.abs(lf - l64).max() <= Y.FACTORS[1] * e_ls


@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_fused_log_probabilities_match_the_rollouts_recorded_ones(kind):
    actor, critic, ls, rec = _record(kind)
    obs, act = rec["obs"].to("cuda"), rec["act"].to("cuda")
    with torch.no_grad():
        logp_f, ent_f = _logp(actor, ls, obs, act, kind, True)
        logp_t, ent_t = _logp(actor, ls, obs, act, kind, False)
    m = rec["mask"].to("cuda")
    assert int(m.sum()) > 500
    torch.testing.assert_close(logp_f[m], rec["logp"].to("cuda")[m], rtol=0, atol=LOGP_TOL)
    torch.testing.assert_close(logp_f, logp_t, rtol=0, atol=LOGP_TOL)
    torch.testing.assert_close(ent_f, ent_t, rtol=0, atol=LOGP_TOL)
    assert math.isfinite(float(logp_f.sum()))
