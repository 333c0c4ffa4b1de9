"""The QMIX head on the MI355X (csrc/bsx_qmix_head.hip: learner.qmix_head, qmix_inputs): g4, gh, q and td BIT FOR BIT against the header's
contract restated in numpy float32 (tests/qmix_util.py: contract32 -- every operation is specified, so the bar is exact), on clean inputs
and on rows built to hit the contract's corners, for every embed, double Q on and off, Huber off and delta = 1, weighted and plain; the
statistics within yardstick_util.scalar_bound of float64; between guard slabs; the same bits on every call; td=None accepted;
qmix_inputs as bit copies.  The same at the shapes where a workgroup takes two or three tiles (qmix_util.LARGE_SHAPES), at every embed,
with every partial row of the workspace written."""
import numpy as np
import pytest
import torch

import offpolicy_util as O
import qmix_util as X

pytestmark = pytest.mark.gpu

_bits = O.bits


@pytest.mark.parametrize("shape,form", X.head_cases(), ids=[X.head_case_id(c) for c in X.head_cases()])
def test_the_heads_outputs_are_the_contracts_bits_and_its_statistics_float64s_between_guard_slabs(shape, form):
    """Clean inputs.  Two fills: an output float that keeps both was not written; the two calls leave the same bits.  Every partial row
    of the workspace -- 513 or 683 of them at qmix_util.LARGE_SHAPES -- is written."""
    B, nA, embed = shape
    inp, ref, e_stats = X.head_case_of(shape, form)
    fills = []
    for fill in (7.0, -3.0):
        kept = {}
        res, stray = X.guarded_head(inp, embed, form, guarded=True, fill=fill, keep=kept)
        assert not stray, stray
        fills.append([t.clone() for t in res])
        ws = kept["workspace"]
        assert ws.shape[0] == X.PLANS.get(shape, (0, 0, ws.shape[0]))[2] and not bool((ws == -1).any())    # the -1 fill is gone from every row
    assert O.same_bits(*fills)
    want = X.contract32(inp, embed, **X._kw(form))
    for k in X.OUTS:
        got = _bits(getattr(res, k))
        assert np.array_equal(got, want[k].view(np.int32)), (k, int((got != want[k].view(np.int32)).sum()), got.size)
    what = "QMIX " + X.shape_id(shape) + " " + X.form_id(form)
    bad = X.stats_out_of_bounds(res.stats.cpu().numpy(), ref["stats"], e_stats, what)
    assert not bad, (what, bad)
    assert ((_bits(res.g4) != 0).sum(-1) <= 1).all()                              # one column per row; the other three are +0
    assert not _bits(res.gh)[:, -1, 1:].any()                                     # b2's row: columns 1 .. 3 are +0
    assert all(np.array_equal(_bits(getattr(res, k)), np.repeat(_bits(getattr(res, k))[:, :1], nA, 1)) for k in ("q", "td"))


@pytest.mark.parametrize("shape,form", X.head_cases(), ids=[X.head_case_id(c) for c in X.head_cases()])
def test_on_the_corner_rows_the_heads_outputs_are_the_contracts_bits(shape, form):
    """qmix_util.corner_inputs: ties and a NaN in act, a finished team whose next rows are NaN or infinite (they stay out), ONE plane
    finished, |d| exactly delta, pre exactly 0 and far below 0 (inputs beyond [-1, 1]), hypernet values +0 and -0, a NaN d under Huber,
    ties and NaN in the rows double Q picks by.  The same bits wherever the contract gives a number, a NaN wherever it gives a NaN; +0
    in the three other columns of g4 and beside b2."""
    B, nA, embed = shape
    inp, fitted = X.corner_inputs(B, nA, embed)
    res, stray = X.guarded_head(inp, embed, form, guarded=True)
    assert not stray, stray
    want = X.contract32(inp, embed, **X._kw(form))
    for k in X.OUTS:
        assert X.same_bits_or_nan(getattr(res, k).cpu().numpy(), want[k]), (k, fitted)
    g4 = res.g4.cpu().numpy()
    a = np.argmax(inp["act"].numpy(), -1)
    others = np.ones(g4.shape, bool)
    np.put_along_axis(others, a[..., None], False, -1)
    assert not g4.view(np.int32)[others].any()                                    # +0, not -0, not NaN, beside a NaN too
    assert not _bits(res.gh)[:, -1, 1:].any()
    again, _ = X.guarded_head(inp, embed, form)
    assert all(X.same_bits_or_nan(getattr(again, k).cpu().numpy(), getattr(res, k).cpu().numpy()) for k in X.OUTS)
    assert np.array_equal(again.stats.cpu().numpy().view(np.int64), res.stats.cpu().numpy().view(np.int64))
    if B >= len(X.CORNERS):
        st = res.stats.cpu().numpy()
        assert st[0] == B and np.isnan(st[1]) and np.isfinite(st[5:]).all()         # the NaN d reaches the loss, not the counts


@pytest.mark.parametrize("form", (X.FORMS[0], X.FORMS[3], X.FORMS[5], X.FORMS[6]), ids=X.form_id)
def test_td_none_is_accepted_and_changes_nothing_else(form):
    shape = X.HEAD_SHAPES[2]
    inp, *_ = X.head_case(shape, form)
    with_td, _ = X.guarded_head(inp, shape[2], form)
    without, stray = X.guarded_head(inp, shape[2], form, guarded=True, td=False)
    assert not stray and without.td is None
    assert O.same_bits((with_td.g4, with_td.gh, with_td.q), (without.g4, without.gh, without.q)) and torch.equal(with_td.stats, without.stats)


def test_finished_planes_keep_their_next_values_out_and_double_q_reads_the_online_rows_for_the_choice_alone():
    shape = X.HEAD_SHAPES[2]
    B, nA, embed = shape
    form = (True, X.DELTA, True)
    inp, *_ = X.head_case(shape, form)
    fin = inp["done"] != 0
    over = fin.all(1)
    assert 20 < int(over.sum()) < B - 20 and bool((fin.any(1) & ~over).any())
    base, _ = X.guarded_head(inp, embed, form)
    nan4 = torch.full((4,), O.NAN)
    poisoned = dict(inp, y_next_target=torch.where(fin[..., None], nan4, inp["y_next_target"]),
                    y_next_online=torch.where(fin[..., None], nan4, inp["y_next_online"]),
                    hy_next_target=torch.where(over[:, None, None], nan4, inp["hy_next_target"]))
    out, _ = X.guarded_head(poisoned, embed, form)
    assert O.same_bits(base[:4], out[:4]) and torch.equal(base.stats, out.stats) and bool(torch.isfinite(out.stats).all())
    # scaling the online rows by a positive number moves no choice and so no bit; without double Q they are not read at all
    scaled, _ = X.guarded_head(dict(inp, y_next_online=inp["y_next_online"] * 0.5), embed, form)
    assert O.same_bits(base[:4], scaled[:4])
    single = (False, X.DELTA, True)
    a, _ = X.guarded_head(inp, embed, single)
    b, _ = X.guarded_head(dict(inp, y_next_online=torch.full_like(inp["y_next_online"], O.NAN)), embed, single)
    assert O.same_bits(a[:4], b[:4]) and not O.same_bits((a.td,), (base.td,))
    # the weight is column 0's: the other columns are not read
    c, _ = X.guarded_head(dict(inp, weight=torch.cat([inp["weight"][:, :1], torch.full((B, nA - 1), O.NAN)], 1)), embed, form)
    assert O.same_bits(base[:4], c[:4])


@pytest.mark.parametrize("case", ((1, 1, 5, 4), (5, 3, 11, 8), (257, 2, 8, 8), (300, 4, 14, 16), (12000, 4, 16, 16)),
                         ids=lambda c: "B%d-nA%d-Do%d-E%d" % c)
def test_the_mixers_inputs_are_bit_copies_of_the_joint_observation_between_guard_slabs(case):
    """Every member's row is the batch row's joint observation, NaN payloads and -0 included; the last case strides over its grid
    (12 000 x 25 x 64 floats exceed its 2^24 threads)."""
    B, nA, Do, embed = case
    Mh = X.members(nA, embed)
    g = torch.Generator().manual_seed(8400 + B)
    obs, obs_next = (torch.randint(-2 ** 31, 2 ** 31 - 1, (B, nA, Do), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32) for _ in range(2))
    obs[0, 0, 0] = -0.0
    x_cur, x_next, stray = X.guarded_inputs(obs, obs_next, Mh)
    assert not stray, stray
    for x, o in ((x_cur, obs), (x_next, obs_next)):
        want = o.view(torch.int32).reshape(B, 1, nA * Do).expand(-1, Mh, -1)
        assert torch.equal(x.view(torch.int32).cpu(), want)
