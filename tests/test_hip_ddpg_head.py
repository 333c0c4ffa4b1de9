"""The DDPG head kernels on the MI355X (csrc/bsx_ddpg_head.hip: learner.ddpg_inputs, ddpg_put_actions, ddpg_action_grad, td_head): the
three copies bit for bit against their restatements between guard slabs, with every float the contract leaves alone still poisoned;
the TD head against the float64 restatement at a small multiple of what torch float32 autograd itself loses on the same inputs
(tests/ddpg_util.py); finished rows, gamma = 0, the weight's forms; the same bits on every call and from a captured graph."""
import numpy as np
import pytest
import torch

import ddpg_util as D
import offpolicy_util as O
from guard_util import Buffers

pytestmark = pytest.mark.gpu

COPY_SHAPES = D.SHAPES[:-1] + ((300, 16, 1, 3, 0),)     # (the head's larger shape has nothing for the copies: a second workgroup does)


_bits, _same_bits = O.bits, O.same_bits


def _same(t, want):
    return np.array_equal(_bits(t), np.ascontiguousarray(want).view(np.int32))


# ---------------------------------------------------------------------------------------------------- 1. the three copies
@pytest.mark.parametrize("shape", COPY_SHAPES, ids=D.shape_id)
def test_the_three_copy_kernels_move_exactly_the_bits_of_their_contract_between_guard_slabs(shape):
    from deep_rl_battlespace_amd import learner as L
    B, nA, Do, k, central = shape
    Dc = D.width(nA, Do, k, central)
    obs, obs_next, act = D.batch_arrays(shape)
    G = Buffers(True)
    dev = {}
    for name, a in (("obs", obs), ("obs_next", obs_next), ("act", act)):
        dev[name] = G(name, a.shape, torch.float32)
        dev[name].copy_(torch.from_numpy(a))
    nan = float("nan")
    xs = tuple(G(name, (B, nA, Dc), torch.float32, init=nan) for name in ("x_cur", "x_next", "x_pi"))
    poison = [np.full((B, nA, Dc), np.nan, np.float32) for _ in range(3)]
    # (the poison's bits: torch.full's NaN and numpy's are the same quiet NaN, 0x7fc00000)
    assert all(_same(x, p) for x, p in zip(xs, poison))
    out = L.ddpg_inputs(dev["obs"], dev["obs_next"], dev["act"], central=bool(central), out=xs)
    assert all(a is b for a, b in zip(out, xs))
    want = D.ref_inputs(obs, obs_next, act, central, *poison)
    for name, x, w in zip(("x_cur", "x_next", "x_pi"), xs, want):
        assert _same(x, w), name
    assert not np.isnan(want[0]).any() and np.isnan(want[1]).any() and (central or np.isnan(want[2]).any())
    g = np.random.default_rng(11)
    y4 = g.standard_normal((B, nA, 4)).astype(np.float32)
    y4d = G("y4", (B, nA, 4), torch.float32)
    y4d.copy_(torch.from_numpy(y4))
    L.ddpg_put_actions(y4d, xs[1], Do, k, central=bool(central), own_only=False)
    x_next = D.ref_put_actions(y4, want[1], Do, k, central, False)
    assert _same(xs[1], x_next) and not np.isnan(x_next).any()
    L.ddpg_put_actions(y4d, xs[2], Do, k, central=bool(central), own_only=True)
    x_pi = D.ref_put_actions(y4, want[2], Do, k, central, True)
    assert _same(xs[2], x_pi) and not np.isnan(x_pi).any()
    # own_only on a poisoned x touches the own slot alone; without it every slot; never an observation column
    for own_only in (True, False):
        xp = G(f"x_poison{int(own_only)}", (B, nA, Dc), torch.float32, init=nan)
        L.ddpg_put_actions(y4d, xp, Do, k, central=bool(central), own_only=own_only)
        wantp = D.ref_put_actions(y4, poison[0], Do, k, central, own_only)
        assert _same(xp, wantp)
        assert int(np.isnan(wantp).sum()) == B * nA * (Dc - (k if (own_only or not central) else nA * k))
    gx = g.standard_normal((B, nA, Dc)).astype(np.float32)
    gxd = G("gx", (B, nA, Dc), torch.float32)
    gxd.copy_(torch.from_numpy(gx))
    g_a4 = G("g_a4", (B, nA, 4), torch.float32, init=nan)
    assert L.ddpg_action_grad(gxd, Do, k, central=bool(central), out=g_a4) is g_a4
    ga = D.ref_action_grad(gx, Do, k, central)
    assert _same(g_a4, ga)
    if k == 3:
        assert not _bits(g_a4)[..., 3].any()                      # +0: no bit set
    torch.cuda.synchronize()
    assert not G.stray(), G.stray()
    # the inputs are read only
    assert _same(dev["obs"], obs) and _same(dev["obs_next"], obs_next) and _same(dev["act"], act) and _same(y4d, y4) and _same(gxd, gx)


def test_central_and_own_leave_the_same_bits_for_a_team_of_one():
    from deep_rl_battlespace_amd import learner as L
    own, central = D.SHAPES[1], D.SHAPES[2]
    assert own[:4] == central[:4] and own[1] == 1 and (own[4], central[4]) == (0, 1)
    B, nA, Do, k, _ = own
    obs, obs_next, act = (torch.from_numpy(a).cuda() for a in D.batch_arrays(own))
    y4, gx = torch.randn((B, nA, 4), device="cuda"), torch.randn((B, nA, Do + k), device="cuda")
    res = []
    for c in (False, True):
        xs = tuple(torch.full((B, nA, Do + k), 3.0, device="cuda") for _ in range(3))
        L.ddpg_inputs(obs, obs_next, act, central=c, out=xs)
        L.ddpg_put_actions(y4, xs[1], Do, k, central=c, own_only=False)
        L.ddpg_put_actions(y4, xs[2], Do, k, central=c, own_only=True)
        res.append([*xs, L.ddpg_action_grad(gx, Do, k, central=c)])
    # (x_pi's action columns after inputs alone differ by contract -- central fills them, own leaves them --: put_actions has run here)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res))


# ---------------------------------------------------------------------------------------------------- 2. the TD head
def _head(inp, *args, **kw):
    return O.guarded_head(D.HEAD, inp, *args, **kw)


@pytest.mark.parametrize("weight", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_the_td_head_stays_within_the_float32_yardstick_of_the_float64_contract_between_guard_slabs(shape, weight):
    """Every shape of the table, the larger one included (two tiles per workgroup, five rounds of the merge).  Two fills: an output
    float that keeps both was not written."""
    B, nA = shape[:2]
    inp, ref, yard, e_stats = D.HEAD.case(B, nA, weight)
    fills = []
    for fill in (7.0, -3.0):
        res, stray = _head(inp, weight, guarded=True, fill=fill)
        assert not stray, stray
        fills.append([t.clone() for t in res])
    assert _same_bits(*fills)
    D.HEAD.check(O.numpy_of(res, D.HEAD.names), ref, yard, e_stats, f"TD {D.shape_id(shape)} {'weighted' if weight else 'plain'}",
                 D.HEAD.factors(B, nA, weight))
    assert not _bits(res.g_q)[..., 1:].any() and not _bits(res.g_pi)[..., 1:].any()           # columns 1 .. 3: +0


def test_finished_rows_and_gamma_zero_give_the_reward_exactly_and_keep_q_next_out():
    B, nA = D.SHAPES[3][:2]
    inp, *_ = D.HEAD.case(B, nA)
    allover = dict(inp, done=torch.ones_like(inp["done"]), q_next=torch.full_like(inp["q_next"], float("nan")))
    res, _ = _head(allover)
    assert torch.equal(res.td.cpu().view(torch.int32), inp["rew"].view(torch.int32))
    assert bool(torch.isfinite(res.g_q).all()) and bool(torch.isfinite(res.stats).all()) and float(res.stats[5]) == 1.0
    zero, _ = _head(inp, gamma=0.0)
    assert torch.equal(zero.td.cpu().view(torch.int32), inp["rew"].view(torch.int32))
    # the same gradients either way: with y = rew, q_next and done play no part
    other, _ = _head(dict(allover, q_next=inp["q_next"]))
    assert _same_bits(res[:3], other[:3])
    # a finished row among running ones: its q_next stays out, NaN included; the running rows keep their bits
    some = dict(inp, q_next=torch.where(inp["done"] != 0, torch.tensor(float("nan")), inp["q_next"]))
    a, b = _head(inp), _head(some)
    assert int((inp["done"] != 0).sum()) > 20 and _same_bits(a[0], b[0])


def test_no_weight_is_a_weight_of_ones_bit_for_bit_and_a_weight_of_zero_gives_zero_gradients():
    B, nA = D.SHAPES[4][:2]
    inp, *_ = D.HEAD.case(B, nA)
    none, _ = _head(inp, weight=False)
    ones, _ = _head(dict(inp, weight=torch.ones_like(inp["weight"])))
    assert _same_bits(none, ones)
    w = inp["weight"].clone()
    w[::3] = 0.0
    res, _ = _head(dict(inp, weight=w))
    gq, gpi = _bits(res.g_q)[::3], _bits(res.g_pi)[::3]
    assert not (gq & 0x7fffffff).any() and not (gpi & 0x7fffffff).any()                        # +-0
    assert (_bits(res.g_q)[1::3][..., 0] & 0x7fffffff).all() and bool((res.g_pi[1::3, :, 0] < 0).all())
    no_td, _ = _head(inp, td=False)                                                            # td is optional
    full, _ = _head(inp)
    assert no_td.td is None and _same_bits((no_td.g_q, no_td.g_pi, no_td.stats), (full.g_q, full.g_pi, full.stats))


@pytest.mark.parametrize("shape", (D.SHAPES[3], D.LARGE), ids=D.shape_id)
def test_the_same_bits_on_two_calls_and_from_a_captured_graph(shape):
    from deep_rl_battlespace_amd.learner import td_head, td_head_workspace_bytes
    B, nA = shape[:2]
    inp, *_ = D.HEAD.case(B, nA)
    first, _ = _head(inp)
    second, _ = _head(inp, fill=-3.0)
    assert _same_bits(first, second)
    dev = {k: v.cuda() for k, v in inp.items()}
    out = (torch.zeros((B, nA, 4), device="cuda"), torch.zeros((B, nA, 4), device="cuda"), torch.zeros((B, nA), device="cuda"),
           torch.zeros(8, dtype=torch.float64, device="cuda"))
    ws = torch.empty(td_head_workspace_bytes(B, nA) // 8, dtype=torch.int64, device="cuda")
    call = lambda: td_head(dev["q"], dev["q_next"], dev["rew"], dev["done"], D.GAMMA, weight=dev["weight"], out=out, workspace=ws)   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in out:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in out)                                                 # a capture runs nothing
    held = torch.cuda.memory_allocated()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held and _same_bits(first, out)
