"""The TD3 kernels on the MI355X (csrc/bsx_td3_head.hip: learner.td3_head, td3_smooth_actions): the twin head against its float64
restatement at a small multiple of what torch float32 autograd itself loses on the same inputs (tests/td3_util.py), between guard
slabs, the same bits on every call; its reduction to bsx_td_head bit for bit; finished rows and a NaN in either target critic; the
smoothing with injected normals bit for bit against its numpy restatement with every other float of x untouched, and with the
Philox normals of philox_util under the salt of its own."""
import numpy as np
import pytest
import torch

import ddpg_util as D
import offpolicy_util as O
import philox_util as PU
import td3_util as T
from guard_util import Buffers

pytestmark = pytest.mark.gpu

SEED, SEQ, SEQ_BASE = 0x1234ABCD5678, 7, (1 << 33) + 1000
NORMAL_TOL, NAN, SENTINEL = O.NORMAL_TOL, O.NAN, O.SENTINEL       # (the bar on the normals here: + one float32 rounding)
_bits, _same_bits = O.bits, O.same_bits


# ---------------------------------------------------------------------------------------------------- 1. the twin head
def _head(inp, *args, **kw):
    return O.guarded_head(T.HEAD, inp, *args, **kw)


@pytest.mark.parametrize("weight", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("BnA", T.HEAD_SHAPES, ids=lambda s: "B%d-nA%d" % s)
def test_the_twin_head_stays_within_the_float32_yardstick_of_the_float64_contract_between_guard_slabs(BnA, weight):
    """Every shape of the issue, the larger one included (two tiles per workgroup, five rounds of the merge), at the project's (2, 4) --
    but for the one-element shape, where profiles/td3_float64.json records the yardstick's own spread (td3_util.HEAD.spread) and the
    factor the rule makes of it.  Two fills: an output float that keeps both was not written; the two calls leave the same bits."""
    inp, ref, yard, e_stats = T.HEAD.case(*BnA, weight)
    fills = []
    for fill in (7.0, -3.0):
        res, stray = _head(inp, weight, guarded=True, fill=fill)
        assert not stray, stray
        fills.append([t.clone() for t in res])
    assert _same_bits(*fills)
    T.HEAD.check(O.numpy_of(res, T.HEAD.names), ref, yard, e_stats, "TD3 " + O.head_id(*BnA, weight), T.HEAD.factors(*BnA, weight))
    assert all(not _bits(getattr(res, k))[..., 1:].any() for k in ("g_q1", "g_q2", "g_pi"))       # columns 1 .. 3: +0


@pytest.mark.parametrize("weight", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("BnA", T.HEAD_SHAPES, ids=lambda s: "B%d-nA%d" % s)
def test_the_twin_heads_per_element_outputs_are_the_contracts_bits(BnA, weight):
    """g_q1, g_q2, g_pi and td against td3_util.contract32, the header's contract operation by operation in float32: the same bits at
    every shape, not only within the yardstick (the statistics are sums and stay with the test above)."""
    inp, *_ = T.HEAD.case(*BnA, weight)
    res, _ = _head(inp, weight)
    want = T.contract32(inp, weight=weight)
    for k in T.HEAD.names:
        assert np.array_equal(_bits(getattr(res, k)), want[k].astype(np.float32).view(np.int32)), k


@pytest.mark.parametrize("weight", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("BnA", (T.HEAD_SHAPES[2], T.HEAD_SHAPES[-1]), ids=lambda s: "B%d-nA%d" % s)
def test_with_the_second_critic_a_copy_of_the_first_the_head_is_bsx_td_heads_bit_for_bit(BnA, weight):
    from deep_rl_battlespace_amd.learner import td_head
    inp, *_ = T.HEAD.case(*BnA)
    res, _ = _head(dict(inp, q2=inp["q1"], q2_next=inp["q1_next"]), weight)
    dev = {k: v.cuda() for k, v in inp.items()}
    one = td_head(dev["q1"], dev["q1_next"], dev["rew"], dev["done"], D.GAMMA, weight=dev["weight"] if weight else None)
    torch.cuda.synchronize()
    assert _same_bits((res.g_q1, res.g_pi, res.td, res.g_q2), (one.g_q, one.g_pi, one.td, one.g_q))
    assert float(res.stats[7]) == 0.0 and float(one.stats[7]) == 0.0
    assert torch.equal(res.stats[2:7], one.stats[2:7]) and float(res.stats[0]) == float(one.stats[0])
    assert abs(float(res.stats[1]) - 2.0 * float(one.stats[1])) <= 1e-12 * float(res.stats[1])  # (w d) d twice, summed in float64


def test_a_finished_row_keeps_both_q_next_out_and_a_nan_in_either_target_critic_reaches_a_running_row():
    B, nA = T.HEAD_SHAPES[2]
    inp, *_ = T.HEAD.case(B, nA)
    over = inp["done"] != 0
    assert 20 < int(over.sum()) < B * nA - 20
    nan = torch.tensor(NAN)
    base, _ = _head(inp)
    # finished rows: NaN in both q_next, nothing moves
    out, _ = _head(dict(inp, q1_next=torch.where(over, nan, inp["q1_next"]), q2_next=torch.where(over, nan, inp["q2_next"])))
    assert _same_bits(base, out) and bool(torch.isfinite(out.stats).all())
    allover = dict(inp, done=torch.ones_like(inp["done"]), q1_next=torch.full_like(inp["q1_next"], NAN), q2_next=torch.full_like(inp["q2_next"], NAN))
    res, _ = _head(allover)
    assert torch.equal(res.td.cpu().view(torch.int32), inp["rew"].view(torch.int32)) and float(res.stats[5]) == 1.0
    # a running row: a NaN in q1_next ALONE, or in q2_next ALONE, makes td NaN (np.minimum's rule; fminf would return the other one)
    for which in ("q1_next", "q2_next"):
        res, _ = _head(dict(inp, **{which: torch.full_like(inp[which], NAN)}))
        td = res.td.cpu()
        assert bool(torch.isnan(td[~over]).all()), which
        assert torch.equal(td[over].view(torch.int32), base.td.cpu()[over].view(torch.int32)), which
    # the smaller of the two, either way round, and infinities
    swapped, _ = _head(dict(inp, q1_next=inp["q2_next"], q2_next=inp["q1_next"]))
    assert _same_bits((base.td,), (swapped.td,))
    inf, _ = _head(dict(inp, q1_next=torch.full_like(inp["q1_next"], float("inf"))))
    want, _ = _head(dict(inp, q1_next=inp["q2_next"]))
    assert _same_bits((inf.td,), (want.td,))


# ---------------------------------------------------------------------------------------------------- 2. the smoothing
def _x(G, shape, name="x"):
    return O.sentinel_x(G, shape, D.width(*shape[1:]), name)


# each (B, nA, Do) of ddpg_util.SHAPES with own and with central critics at k = 3 and 4, wherever the critic's input fits its 64 columns
SMOOTH_SHAPES = tuple(sorted({(B, nA, Do, k, c) for B, nA, Do, _, _ in D.SHAPES for k in (3, 4) for c in (0, 1) if D.width(nA, Do, k, c) <= 64}))


@pytest.mark.parametrize("shape", SMOOTH_SHAPES, ids=D.shape_id)
def test_the_smoothing_with_injected_normals_is_its_restatement_bit_for_bit_and_writes_nothing_else(shape):
    """Between guard slabs; x starts as a sentinel bit pattern and every float outside the written slots keeps it; with a central
    critic the action columns of the nA rows of a batch row are the same bits."""
    from deep_rl_battlespace_amd.learner import td3_smooth_actions
    B, nA, Do, k, central = shape
    g = np.random.default_rng(31 + k)
    y4 = np.tanh(2.0 * g.standard_normal((B, nA, 4))).astype(np.float32)
    z = g.standard_normal((B, nA, 4)).astype(np.float32)
    G = Buffers(True)
    y4d, zd = G("y4", y4.shape, torch.float32), G("z", z.shape, torch.float32)
    y4d.copy_(torch.from_numpy(y4)); zd.copy_(torch.from_numpy(z))
    for sigma, clip in ((T.SIGMA, T.CLIP), (1.0, 0.5)):
        x = _x(G, shape, f"x sigma {sigma}")
        x0 = x.cpu().numpy()
        assert td3_smooth_actions(y4d, x, Do, k, sigma=sigma, clip=clip, seed=SEED, z=zd, central=bool(central)) is x
        torch.cuda.synchronize()
        assert not G.stray(), G.stray()
        want = T.ref_smooth(y4, z, x0, Do, k, central, sigma, clip)
        got = x.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (sigma, clip)
        W = nA * Do if central else Do
        assert (got.view(np.int32)[..., :W] == SENTINEL).all() and not (got.view(np.int32)[..., W:] == SENTINEL).any()
        if central:
            assert all(np.array_equal(got.view(np.int32)[:, 0, W:], got.view(np.int32)[:, i, W:]) for i in range(1, nA))
        again = _x(Buffers(False), shape)
        td3_smooth_actions(y4d, again, Do, k, sigma=sigma, clip=clip, seed=SEED, z=zd, central=bool(central))
        assert _same_bits((x,), (again,))
    assert np.array_equal(_bits(y4d), y4.view(np.int32)) and np.array_equal(_bits(zd), z.view(np.int32))       # the inputs are read only
    # sigma = 0 is ddpg_put_actions(own_only=False) of the clamped rows: tanh outputs lie in [-1, 1], so of y4 itself
    from deep_rl_battlespace_amd.learner import ddpg_put_actions
    a, b = _x(Buffers(False), shape), _x(Buffers(False), shape)
    td3_smooth_actions(y4d, a, Do, k, sigma=0.0, clip=0.5, seed=SEED, z=zd, central=bool(central))
    ddpg_put_actions(y4d, b, Do, k, central=bool(central), own_only=False)
    assert _same_bits((a,), (b,))


def _philox_actions(B, nA, sigma, clip, seq_base, seed=SEED, seq=SEQ, k=4):
    """The action columns [B, nA, k] the kernel writes from y4 = 0 with its own Philox normals (own critics: one slot per row)."""
    from deep_rl_battlespace_amd.learner import td3_smooth_actions
    Do = 2
    y4 = torch.zeros((B, nA, 4), device="cuda")
    x = torch.full((B, nA, Do + k), 9.0, device="cuda")
    base = torch.tensor([seq_base], dtype=torch.int64, device="cuda")
    td3_smooth_actions(y4, x, Do, k, sigma=sigma, clip=clip, seed=seed, seq=seq, seq_base=base, central=False)
    torch.cuda.synchronize()
    assert bool((x[..., :Do] == 9.0).all()) and int(base) == seq_base
    return x[..., Do:].double().cpu().numpy()


def test_the_smoothings_own_draws_are_philox_normals_under_a_salt_of_their_own():
    """sigma = 1, clip = 100, y4 = 0, B nA = 4133: a' = clamp(z, -1, 1), so the action columns are philox_util.normals4(seed, seq +
    seq_base, b nA + j, 0x20000000) clamped to [-1, 1] -- a clamp moves no two numbers apart, so the bar on z (NORMAL_TOL's rule, plus
    the float32 rounding of 0 + z) holds on them as it stands -- and far from the draws at each of the four other salts."""
    B, nA = 4133, 1
    got = _philox_actions(B, nA, 1.0, 100.0, SEQ_BASE)
    z = T.philox_normals(SEED, SEQ + SEQ_BASE, B, nA)
    err = np.abs(got - np.clip(z, -1.0, 1.0)) / (1.0 + np.abs(z))
    print(f"max |a' - clamp(z64)| / (1 + |z64|) = {err.max():.3e} (bar {NORMAL_TOL + 2.0 ** -22:.3e})")
    assert float(err.max()) <= NORMAL_TOL + 2.0 ** -22
    inside = np.abs(z) < 0.999
    assert 0.6 < inside.mean() < 0.75 and float((np.abs(got - z)[inside] / (1.0 + np.abs(z[inside]))).max()) <= NORMAL_TOL + 2.0 ** -22
    grows = np.arange(B * nA, dtype=np.uint64)
    for other in T.OTHER_SALTS:
        assert np.abs(got - PU.normals4(SEED, SEQ + SEQ_BASE, grows, other).reshape(B, nA, 4)).mean() > 0.5, hex(other)
    # the key is (b nA + j): the same draws whatever the team's size, and three columns are the first three of four
    assert np.array_equal(_philox_actions(4133 // 3, 3, 1.0, 100.0, SEQ_BASE).reshape(-1, 4), got.reshape(-1, 4)[:4133 // 3 * 3])
    assert np.array_equal(_philox_actions(B, nA, 1.0, 100.0, SEQ_BASE, k=3), got[..., :3])
    # seq and the device word add up
    assert np.array_equal(_philox_actions(B, nA, 1.0, 100.0, SEQ_BASE + SEQ, seq=0), got)


def test_the_noise_is_clipped_and_another_sequence_word_draws_other_noise():
    """sigma = 1, clip = 0.5, y4 = 0: every |a'| <= 0.5, a positive share sits exactly at +-0.5 (P(|z| > 0.5) = 0.617), and
    another seq_base gives other draws."""
    B, nA = 4133, 1
    got = _philox_actions(B, nA, 1.0, 0.5, SEQ_BASE)
    at = np.abs(got) == 0.5
    print(f"share at +-0.5: {at.mean():.4f}")
    assert (np.abs(got) <= 0.5).all() and 0.55 < at.mean() < 0.68 and (got == 0.5).any() and (got == -0.5).any()
    z = T.philox_normals(SEED, SEQ + SEQ_BASE, B, nA)
    assert np.array_equal(at, np.abs(z) > 0.5) or np.abs(at.astype(int) - (np.abs(z) > 0.5).astype(int)).sum() <= 2   # (a z within 1e-5 of 0.5)
    other = _philox_actions(B, nA, 1.0, 0.5, SEQ_BASE + 1)
    assert (other != got).mean() > 0.5 and (np.abs(other) <= 0.5).all()
    assert np.array_equal(_philox_actions(B, nA, 1.0, 0.5, SEQ_BASE), got)                          # and the same word the same bits
