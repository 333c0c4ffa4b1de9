"""The fused MLP on any input width and its input gradient on the MI355X (bsx_mlp_forward / bsx_mlp_grad, learner.fused_mlp / mlp_grad):
the ten parameter gradients and grad_x against float64 autograd at (2, 4) times what float32 autograd itself loses on the same inputs
(tests/mlp_grad_util.py: ReLU kinks left out by construction; a larger factor only where profiles/mlp_input_grad.json records that the
yardstick itself moves by as much: one-row cases, and b3 under row order), on the table of shapes from one row of one input to 32 agents over two
rounds; exact zeros where grad_out is zero; the bits of bsx_actor_forward / bsx_actor_grad at (2n, 3n + 2), with and without grad_x,
from the raw entries and from fused_apply and fused_mlp (one path in learner/mlp.py: both are held to the raw actor entries, not to each
other), and the one buffer set they share on a network; guard slabs around grad_x at ragged sizes; the same bits on every call and from a captured graph; one DDPG step whose
actor gradients come through the critic's input gradient; the documented refusals."""
import numpy as np
import pytest
import torch

import actor_ref_util as R
import mlp_grad_util as M
from guard_util import Buffers

pytestmark = pytest.mark.gpu

# |y - float64| of the forward on freshly initialised networks: three times the 6e-7 the float32 actor kernel is documented to lose at
# most on a head sum with such weights (rollout.FusedActor; tests/test_hip_actor_float64.py) -- a check that the forward read the right
# columns at every width, not a precision claim of its own
Y_TOL = 2e-6


def _to(net, device="cuda", dtype=torch.float32):
    a = R._new(net.n_actors, net.obs_len, net.n_actions, dtype=dtype, device=device)
    with torch.no_grad():
        for k in M.PARAMS:
            getattr(a, k).copy_(getattr(net, k).detach().to(device=device, dtype=dtype))
    return a


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_parameter_and_input_gradients_stay_within_the_float32_yardstick_of_float64_autograd(case):
    from deep_rl_battlespace_amd.learner import fused_mlp
    A, D, na, squash, rows, var = case
    net_cpu, x_cpu, go, g64, g32, share = M.reference(case)
    assert float(share.max()) <= M.KINK_CAP
    if rows == 2100:
        assert M.plan(rows, A, D) == (16, 2)                       # 16 workgroups x 128 rows = 2048 < 2100: a second round
    net, x = _to(net_cpu), x_cpu.to("cuda").requires_grad_()
    y = fused_mlp(net, x, squash=squash)
    assert y.shape == (rows, A, na)
    (y * go.to("cuda")).sum().backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        y64 = R.to_float64(net_cpu)(x_cpu.double(), squash=squash)
    print(M.case_id(case), "forward |y - float64| max", float((y.detach().double().cpu() - y64).abs().max()))
    assert float((y.detach().double().cpu() - y64).abs().max()) <= Y_TOL
    got = {k: getattr(net, k).grad.double().cpu().numpy() for k in M.PARAMS}
    got["x"] = x.grad.double().cpu().numpy()
    assert got["x"].shape == (rows, A, D)
    dead = (go == 0).all(-1).numpy()                               # rows with grad_out = 0: an exact zero of either sign
    assert not got["x"][dead].any()
    assert dead.all() or np.abs(got["x"][~dead]).max() > 0
    M.check(got, g64, g32, "KERNEL " + M.case_id(case), cid=M.case_id(case))


# ---------------------------------------------------------------------------------------------------- 2. the bits at (2n, 3n + 2)
def _raw_grad(lib, L, blob, x, go4, squash, A, D, how):
    """grad [A, G] (and grad_x) of one raw call: how = "actor" (bsx_actor_grad), "mlp" (bsx_mlp_grad, grad_x NULL), "mlp_dx"."""
    from deep_rl_battlespace_amd.learner import grad_floats
    Rr, nb = x.shape[0], L.c_size_t()
    L.check(lib.bsx_mlp_grad_workspace_bytes(Rr, A, D, L.ctypes.byref(nb)), "bsx_mlp_grad_workspace_bytes")
    ws = torch.full((nb.value // 4,), 7.0, device="cuda")
    grad = torch.full((A, grad_floats(D)), 7.0, device="cuda")
    gx = torch.full((Rr, A, D), 7.0, device="cuda") if how == "mlp_dx" else None
    if how == "actor":
        L.check(lib.bsx_actor_grad(blob.data_ptr(), x.data_ptr(), go4.data_ptr(), Rr, A // 2, squash, grad.data_ptr(), ws.data_ptr(), _stream()),
                "bsx_actor_grad")
    else:
        L.check(lib.bsx_mlp_grad(blob.data_ptr(), x.data_ptr(), go4.data_ptr(), Rr, A, D, squash, grad.data_ptr(),
                                 gx.data_ptr() if gx is not None else None, ws.data_ptr(), _stream()), "bsx_mlp_grad")
    torch.cuda.synchronize()
    return grad, gx


@pytest.mark.parametrize("n,rows", [(1, 129), (2, 129), (16, 129), (16, 2100)])
def test_at_2n_agents_and_3n_plus_2_inputs_the_entries_give_the_actor_entries_bits(n, rows):
    """bsx_actor_grad delegates to bsx_mlp_grad with grad_x = NULL, so the backward's `plain` comparison holds the delegation (the team
    size to (A, D)) and `with_dx` the second kernel; what anchors the kernels themselves are the float64 tests of this file and of
    tests/test_hip_actor_grad.py."""
    from deep_rl_battlespace_amd import _lib as L
    lib = L.load()
    A, D = 2 * n, 3 * n + 2
    torch.manual_seed(20 + n)
    net = R._new(A, D, 4, device="cuda")
    critic = R._new(A, D, 1, device="cuda")
    x = torch.rand((rows, A, D), device="cuda") * 2 - 1
    go4 = torch.randn((rows, A, 4), device="cuda")
    blob = net.pack()
    # the backward: the parameter row with and without grad_x
    for squash in (1, 0):
        want, _ = _raw_grad(lib, L, blob, x, go4, squash, A, D, "actor")
        plain, _ = _raw_grad(lib, L, blob, x, go4, squash, A, D, "mlp")
        with_dx, gx = _raw_grad(lib, L, blob, x, go4, squash, A, D, "mlp_dx")
        assert torch.equal(plain, want) and torch.equal(with_dx, want)
        assert bool((want != 7.0).all()) and bool((gx != 7.0).all())
    # the forward: y, and raw against the value path
    y0, y1 = torch.full((rows, A, 4), 7.0, device="cuda"), torch.full((rows, A, 4), 7.0, device="cuda")
    v0, v1 = torch.full((rows, A), 7.0, device="cuda"), torch.full((rows, A), 7.0, device="cuda")
    nz = L.BsxActorNoise()
    nz.value_weights, nz.value = blob.data_ptr(), v0.data_ptr()
    L.check(lib.bsx_actor_forward(blob.data_ptr(), x.data_ptr(), y0.data_ptr(), rows, n, L.ACTOR_F32, L.ctypes.byref(nz), 0, 0, None, 0, _stream()),
            "bsx_actor_forward")
    L.check(lib.bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y1.data_ptr(), v1.data_ptr(), rows, A, D, _stream()), "bsx_mlp_forward")
    y2 = torch.full((rows, A, 4), 7.0, device="cuda")
    L.check(lib.bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y2.data_ptr(), None, rows, A, D, _stream()), "bsx_mlp_forward")
    torch.cuda.synchronize()
    assert torch.equal(y1, y0) and torch.equal(v1, v0) and torch.equal(y2, y0) and bool((y0 != 7.0).all()) and bool((v0 != 7.0).all())
    # the autograd functions: outputs and the ten parameter gradients, each against the raw actor entries
    _both_functions_give_the_raw_actor_entries_bits(net, x, True)
    _both_functions_give_the_raw_actor_entries_bits(critic, x, False)


def _both_functions_give_the_raw_actor_entries_bits(net, x, squash):
    """fused_apply and fused_mlp (x not requiring grad) on `net`: the output and the ten .grad tensors are, bit for bit, what direct
    ctypes calls of bsx_actor_forward and bsx_actor_grad give on the same blob, x and padded grad_out."""
    from deep_rl_battlespace_amd import _lib as L
    from deep_rl_battlespace_amd.learner import fused_apply, fused_mlp, split_grad
    lib = L.load()
    (rows, A, D), na = x.shape, net.n_actions
    go = torch.randn((rows, A, na), device="cuda")
    go4 = torch.zeros((rows, A, 4), device="cuda")
    go4[..., :na] = go
    blob = net.pack()
    y0, v0 = torch.full((rows, A, 4), 7.0, device="cuda"), torch.full((rows, A), 7.0, device="cuda")
    nz = L.BsxActorNoise()
    nz.value_weights, nz.value = blob.data_ptr(), v0.data_ptr()
    L.check(lib.bsx_actor_forward(blob.data_ptr(), x.data_ptr(), y0.data_ptr(), rows, A // 2, L.ACTOR_F32, L.ctypes.byref(nz), 0, 0, None, 0,
                                  _stream()), "bsx_actor_forward")
    row, _ = _raw_grad(lib, L, blob, x, go4, int(squash), A, D, "actor")
    want_y, want = (y0[..., :na] if squash else v0.unsqueeze(-1)), split_grad(row, na)
    assert bool((y0 != 7.0).all()) and bool((v0 != 7.0).all()) and bool((row != 7.0).all())
    for f in (fused_apply, fused_mlp):
        for k in M.PARAMS:
            getattr(net, k).grad = None
        y = f(net, x, squash=squash)
        (y * go).sum().backward()
        torch.cuda.synchronize()
        assert y.shape == (rows, A, na) and torch.equal(y.detach(), want_y), f.__name__
        for k, w in zip(M.PARAMS, want):
            assert torch.equal(getattr(net, k).grad, w), (f.__name__, k)
        assert x.grad is None


# (1, 129): D = 5, one dW1 tile and a ragged last tile; (11, 129): D = 35, the first two-tile (MT1 = 2) size of an actor
@pytest.mark.parametrize("squash,outputs", [(True, 4), (False, 1)])
@pytest.mark.parametrize("n,rows", [(1, 129), (11, 129)])
def test_fused_apply_and_fused_mlp_give_the_bits_of_the_raw_actor_entries(n, rows, squash, outputs):
    A, D = 2 * n, 3 * n + 2
    torch.manual_seed(60 + n + outputs)
    net = R._new(A, D, outputs, device="cuda")
    _both_functions_give_the_raw_actor_entries_bits(net, torch.rand((rows, A, D), device="cuda") * 2 - 1, squash)


def test_a_network_used_through_both_functions_holds_one_buffer_set_and_allocates_once():
    """fused_apply, fused_mlp without and fused_mlp with an input gradient on ONE 1v1 actor: one cache with one key, the same workspace
    and gradient row throughout, grad_x from the third on, and nothing new from a fourth call."""
    from deep_rl_battlespace_amd.learner import _buffers, fused_apply, fused_mlp
    A, D, rows = 2, 5, 33
    torch.manual_seed(9)
    net = R._new(A, D, 4, device="cuda")
    x, go = torch.rand((rows, A, D), device="cuda") * 2 - 1, torch.randn((rows, A, 4), device="cuda")
    xg = x.clone().requires_grad_()

    def step(f, xx):
        for k in M.PARAMS:
            getattr(net, k).grad = None
        xx.grad = None
        (f(net, xx) * go).sum().backward()
        torch.cuda.synchronize()
        assert len([a for a in vars(net) if a.startswith("_bsx") and a.endswith("buffers")]) == 1
        (key, buf), = _buffers(net).by_key.items()                 # one cache with one key
        return key, buf["ws"].data_ptr(), buf["grad"].data_ptr(), (buf["gx"].data_ptr() if buf["gx"] is not None else None)
    first, second, third = step(fused_apply, x), step(fused_mlp, x), step(fused_mlp, xg)
    assert first[0] == (rows, A, D, "cuda:0") and first[3] is None
    assert second == first
    assert third[:3] == first[:3] and third[3] is not None and xg.grad is not None and bool(xg.grad.any())
    held = torch.cuda.memory_allocated()
    assert step(fused_mlp, xg) == third and torch.cuda.memory_allocated() == held


# ---------------------------------------------------------------------------------------------------- 3. guards
@pytest.mark.parametrize("rows", [1, 33, 129])
@pytest.mark.parametrize("A,D", [(2, 5), (3, 33)])
def test_grad_x_is_written_everywhere_and_nothing_around_it_is(rows, A, D):
    from deep_rl_battlespace_amd import _lib as L
    from deep_rl_battlespace_amd.learner import grad_floats
    lib = L.load()
    torch.manual_seed(rows + D)
    net = R._new(A, D, 4, device="cuda")
    nb = L.c_size_t()
    L.check(lib.bsx_mlp_grad_workspace_bytes(rows, A, D, L.ctypes.byref(nb)), "bsx_mlp_grad_workspace_bytes")
    B = Buffers(True)
    x = B("x", (rows, A, D), torch.float32); x.copy_(torch.rand((rows, A, D), device="cuda") * 2 - 1)
    go = B("grad_out", (rows, A, 4), torch.float32); go.copy_(torch.randn((rows, A, 4), device="cuda"))
    grad = B("grad", (A, grad_floats(D)), torch.float32, init=float("nan"))
    gx = B("grad_x", (rows, A, D), torch.float32, init=float("nan"))
    ws = B("workspace", (nb.value // 4,), torch.float32, init=7.0)
    blob = net.pack()
    L.check(lib.bsx_mlp_grad(blob.data_ptr(), x.data_ptr(), go.data_ptr(), rows, A, D, 1, grad.data_ptr(), gx.data_ptr(), ws.data_ptr(), _stream()),
            "bsx_mlp_grad")
    torch.cuda.synchronize()
    assert not B.stray(), B.stray()                                # no float beyond R A D (nor before), in any buffer of the call
    assert not bool(torch.isnan(gx).any()) and not bool(torch.isnan(grad).any())   # and every float of grad_x and grad is written
    # the values between the guards are the gradient: float64 autograd, to 1e-5 of the largest entry
    xx = x.detach().cpu().double().requires_grad_()
    (R.to_float64(net)(xx) * go.cpu().double()).sum().backward()
    assert float((gx.cpu().double() - xx.grad).abs().max()) <= 1e-5 * float(xx.grad.abs().max())


# ---------------------------------------------------------------------------------------------------- 4. determinism, graphs
@pytest.mark.parametrize("A,D,rows", [(2, 9, 129), (32, 54, 2100)])
def test_mlp_grad_gives_the_same_bits_twice_and_from_a_captured_graph_and_allocates_once(A, D, rows):
    from deep_rl_battlespace_amd.learner import mlp_grad
    torch.manual_seed(3)
    net = R._new(A, D, 1, device="cuda")
    x = torch.rand((rows, A, D), device="cuda") * 2 - 1
    go = torch.randn((rows, A, 1), device="cuda")
    blob = net.pack()
    row, gx = mlp_grad(net, blob, x, go, squash=False)
    r1, x1 = row.clone(), gx.clone()
    row2, gx2 = mlp_grad(net, blob, x, go, squash=False)
    torch.cuda.synchronize()
    assert row2.data_ptr() == row.data_ptr() and gx2.data_ptr() == gx.data_ptr()     # the cached buffers: nothing new from the second call on
    assert torch.equal(row2, r1) and torch.equal(gx2, x1)
    row3, gx3 = mlp_grad(net, blob, x, go, squash=False, input_grad=False)
    torch.cuda.synchronize()
    assert gx3 is None and row3.data_ptr() == row.data_ptr() and torch.equal(row3, r1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mlp_grad(net, blob, x, go, squash=False)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grow, ggx = mlp_grad(net, blob, x, go, squash=False)
    assert grow.data_ptr() == row.data_ptr() and ggx.data_ptr() == gx.data_ptr() and len(net._bsx_mlp_buffers.by_key) == 1
    for _ in range(2):
        grow.zero_(); ggx.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(grow, r1) and torch.equal(ggx, x1)


# ---------------------------------------------------------------------------------------------------- 5. one DDPG step
def test_one_ddpg_step_actor_gradients_through_grad_x_and_critic_gradients_against_float64():
    from deep_rl_battlespace_amd.learner import fused_mlp
    actor, critic, obs, act, target, w, share = M.ddpg_case()
    assert share <= M.KINK_CAP
    a64, c64 = M.ddpg_grads(actor, critic, obs, act, target, w, torch.float64)
    a32, c32 = M.ddpg_grads(actor, critic, obs, act, target, w, torch.float32)
    af, cf = M.ddpg_grads(actor, critic, obs, act, target, w, torch.float32, "cuda", lambda net, x, squash: fused_mlp(net, x, squash=squash))
    M.check(af, a64, a32, "DDPG actor", M.PARAMS, cid="ddpg")
    M.check(cf, c64, c32, "DDPG critic", M.PARAMS, cid="ddpg")


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_fused_mlp_and_mlp_grad_refuse_what_they_document():
    from deep_rl_battlespace_amd.learner import fused_mlp, mlp_grad
    from deep_rl_battlespace_amd.rollout import StackedActor
    A, D = 3, 9
    x = torch.rand((7, A, D), device="cuda")
    net = StackedActor(A, D, 4, device="cuda")
    with pytest.raises(ValueError, match="float32"):
        fused_mlp(net, x.double())
    with pytest.raises(ValueError, match="float32"):
        fused_mlp(StackedActor(A, D, 4, device="cuda", dtype=torch.float64), x)
    with pytest.raises(ValueError, match="64"):
        fused_mlp(StackedActor(A, D, 4, fc1_dims=32, device="cuda"), x)
    with pytest.raises(ValueError, match="value head"):
        fused_mlp(net, x, squash=False)
    with pytest.raises(ValueError, match="CUDA"):
        fused_mlp(net, x.cpu())
    with pytest.raises(ValueError, match="CUDA"):
        fused_mlp(StackedActor(A, D, 4), x)
    with pytest.raises(ValueError):
        fused_mlp(net, x[:, :, :8])
    with pytest.raises(ValueError):
        fused_mlp(net, x[:0])
    with pytest.raises(ValueError, match="agents"):
        fused_mlp(StackedActor(33, D, 4, device="cuda"), torch.rand((7, 33, D), device="cuda"))
    with pytest.raises(ValueError, match="inputs"):
        fused_mlp(StackedActor(A, 65, 4, device="cuda"), torch.rand((7, A, 65), device="cuda"))
    with pytest.raises(ValueError, match="outputs"):
        fused_mlp(StackedActor(A, D, 2, device="cuda"), x)
    # what fused_apply refuses and fused_mlp takes: any A and D, leading axes, an x that requires grad
    y = fused_mlp(net, x.reshape(7, 1, A, D).clone().requires_grad_())
    assert y.shape == (7, 1, A, 4) and y.requires_grad
    blob, go = net.pack(), torch.zeros((7, A, 4), device="cuda")
    with pytest.raises(ValueError):
        mlp_grad(net, blob, x.reshape(7, 1, A, D), go)
    with pytest.raises(ValueError):
        mlp_grad(net, blob[:, :-4], x, go)
    with pytest.raises(ValueError):
        mlp_grad(net, blob, x, go[..., :3])
    with pytest.raises(ValueError, match="value head"):
        mlp_grad(net, blob, x, go, squash=False)
    row, gx = mlp_grad(net, blob, x, go)
    torch.cuda.synchronize()
    assert not bool(row.any()) and not bool(gx.any())              # grad_out = 0: exact zeros everywhere
