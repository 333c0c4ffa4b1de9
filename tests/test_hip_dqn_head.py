"""The DQN head on the MI355X (csrc/bsx_dqn_head.hip: learner.dqn_head): g4, q and td BIT FOR BIT against the header's contract restated
in numpy float32 (tests/dqn_util.py: contract32 -- every operation is specified, so the bar is exact), on clean inputs and on rows built
to hit the contract's corners, for both mixes, double Q on and off, Huber off and delta = 1, weighted and plain; the statistics within
yardstick_util.scalar_bound of float64; between guard slabs; the same bits on every call; td=None accepted.  The same at the shapes where a
VDN row lies across two tiles or workgroups and where a workgroup takes two or three tiles (dqn_util.SPLIT_SHAPES, LARGE_SHAPES), with
every partial row of the workspace written; and a split row's threads read across the tile edge, and their own row only."""
import numpy as np
import pytest
import torch

import dqn_util as Q
import offpolicy_util as O

pytestmark = pytest.mark.gpu

_bits = O.bits
SHAPE_IDS = dict(ids=lambda s: "B%d-nA%d" % s)
OUTS = ("g4", "q", "td")


def _kw(form):
    mix, dbl, delta, w = form
    return dict(delta=delta, double=dbl, mix=mix, weight=w)


@pytest.mark.parametrize("BnA,form", Q.head_cases(), ids=[Q.head_case_id(c) for c in Q.head_cases()])
def test_the_heads_outputs_are_the_contracts_bits_and_its_statistics_float64s_between_guard_slabs(BnA, form):
    """Clean inputs.  Two fills: an output float that keeps both was not written; the two calls leave the same bits.  Every partial row
    of the workspace -- 513 or 683 of them at dqn_util.LARGE_SHAPES -- is written."""
    inp, ref, yard, e_stats = Q.head_case_of(BnA, form)
    fills = []
    for fill in (7.0, -3.0):
        kept = {}
        res, stray = Q.guarded_head(inp, form, guarded=True, fill=fill, keep=kept)
        assert not stray, stray
        fills.append([t.clone() for t in res])
        ws = kept["workspace"]
        assert ws.shape[0] == Q.PLANS.get(BnA, (0, 0, ws.shape[0]))[2] and not bool((ws == -1).any())      # the -1 fill is gone from every row
    assert O.same_bits(*fills)
    want = Q.contract32(inp, **_kw(form))
    for k in OUTS:
        assert np.array_equal(_bits(getattr(res, k)), want[k].view(np.int32)), k
    what = "DQN B%d-nA%d " % BnA + Q.form_id(form)
    bad = Q.stats_out_of_bounds(res.stats.cpu().numpy(), ref["stats"], e_stats, what)
    assert not bad, (what, bad)
    g4 = _bits(res.g4)
    assert ((g4 != 0).sum(-1) <= 1).all()                                         # one column per row; the other three are +0
    if form[0] == "vdn":
        assert all(np.array_equal(_bits(getattr(res, k)), np.repeat(_bits(getattr(res, k))[:, :1], BnA[1], 1)) for k in ("q", "td"))


@pytest.mark.parametrize("BnA,form", Q.head_cases(), ids=[Q.head_case_id(c) for c in Q.head_cases()])
def test_on_the_corner_rows_the_heads_outputs_are_the_contracts_bits(BnA, form):
    """dqn_util.corner_inputs: ties in act, y_next and y_cur (the first maximum wins), a NaN in a score row (it counts as the maximum),
    done rows whose next values are NaN or infinite (they stay out), a NaN d under Huber, |d| exactly delta, VDN rows where one agent is
    done and another is not.  The same bits wherever the contract gives a number, a NaN wherever it gives a NaN; +0 in the three other
    columns of g4; under VDN the same bits in all nA columns of q and td."""
    inp, fitted = Q.corner_inputs(*BnA)
    res, stray = Q.guarded_head(inp, form, guarded=True)
    assert not stray, stray
    want = Q.contract32(inp, **_kw(form))
    for k in OUTS:
        assert Q.same_bits_or_nan(getattr(res, k).cpu().numpy(), want[k]), (k, fitted)
    g4 = res.g4.cpu().numpy()
    a = np.argmax(inp["act"].numpy(), -1)
    others = np.ones(g4.shape, bool)
    np.put_along_axis(others, a[..., None], False, -1)
    assert not g4.view(np.int32)[others].any()                                    # +0, not -0, not NaN, beside a NaN too
    if form[0] == "vdn":
        for k in ("q", "td"):
            x = getattr(res, k).cpu().numpy()
            assert Q.same_bits_or_nan(x, np.repeat(x[:, :1], BnA[1], 1)), k
    again, _ = Q.guarded_head(inp, form)
    assert all(Q.same_bits_or_nan(getattr(again, k).cpu().numpy(), getattr(res, k).cpu().numpy()) for k in OUTS)
    assert np.array_equal(again.stats.cpu().numpy().view(np.int64), res.stats.cpu().numpy().view(np.int64))
    if BnA[0] >= len(Q.CORNERS):
        st = res.stats.cpu().numpy()
        assert st[0] == BnA[0] * BnA[1] and np.isnan(st[1]) and np.isfinite(st[5:]).all()        # the NaN d reaches the loss, not the counts


@pytest.mark.parametrize("BnA", (Q.SPLIT_SHAPES[0], Q.LARGE_SHAPES[0]), **SHAPE_IDS)
def test_a_thread_of_a_split_vdn_row_reads_across_the_tile_edge_and_its_own_row_only(BnA):
    """VDN, weighted, double Q, Huber, at (171, 3) -- three workgroups of one tile -- and (87382, 3) -- two tiles per workgroup.  Row 85
    is elements 255 .. 257: its first in tile 0, the others in tile 1 (at the larger shape the same workgroup's second tile); row 170 is
    510 .. 512 and lies across two workgroups at both shapes.  With NaN in every input of the rows that lie wholly in tile 0 (y_cur, rew,
    weight) every other row keeps its bits, rows 85 and 86 included: a thread of tile 1 starts at its own row.  With NaN in ONE element
    of a split row, an element of the LATER tile, q and td are NaN in all three columns of that row -- the column the earlier tile owns
    included -- and every other row keeps its bits: a thread reads across the edge, and its own row only."""
    B, nA = BnA
    form = ("vdn", True, Q.DELTA, True)
    inp = Q.head_inputs(B, nA)
    split = Q.split_rows(B, nA)
    assert nA == 3 and split[:2].tolist() == [85, 170] and (85 * nA) // Q.TILE == 0 and (85 * nA + 1) // Q.TILE == 1
    assert (170 * nA + 1) // Q.TILE == 1 and (170 * nA + 2) // Q.TILE == 2
    base, _ = Q.guarded_head(inp, form)
    got = lambda res: {k: getattr(res, k).cpu().numpy() for k in OUTS}            # noqa: E731
    want = got(base)
    assert all(np.isfinite(v).all() for v in want.values())

    def poisoned(rows, cols):
        out = {k: v.clone() for k, v in inp.items()}
        for k in ("y_cur", "rew", "weight"):
            out[k][rows, cols] = O.NAN
        return out

    whole = torch.arange(85)                                                        # the rows that lie wholly in tile 0: elements 0 .. 254
    res, stray = Q.guarded_head(poisoned(whole, slice(None)), form, guarded=True)
    assert not stray, stray
    for k, v in got(res).items():
        assert np.array_equal(v[85:].view(np.int32), want[k][85:].view(np.int32)), k
        assert np.isnan(v[:85]).reshape(85, -1).any(1).all(), k
    for row, col in ((85, 1), (170, 2)):                                            # elements 256 and 512: the first of tiles 1 and 2
        assert (row * nA + col) % Q.TILE == 0
        res, stray = Q.guarded_head(poisoned(row, col), form, guarded=True)
        assert not stray, stray
        out = got(res)
        others = np.arange(B) != row
        for k in OUTS:
            assert np.array_equal(out[k][others].view(np.int32), want[k][others].view(np.int32)), (k, row)
        assert np.isnan(out["q"][row]).all() and np.isnan(out["td"][row]).all(), row
        assert np.isnan(out["g4"][row]).sum() == nA and np.isnan(out["g4"][row]).any(-1).all(), row     # one column per agent, the earlier tile's too


@pytest.mark.parametrize("form", (Q.FORMS[0], Q.FORMS[3], Q.FORMS[10], Q.FORMS[13]), ids=Q.form_id)
def test_td_none_is_accepted_and_changes_nothing_else(form):
    B, nA = Q.HEAD_SHAPES[2]
    inp, *_ = Q.head_case(B, nA, form)
    with_td, _ = Q.guarded_head(inp, form)
    without, stray = Q.guarded_head(inp, form, guarded=True, td=False)
    assert not stray and without.td is None
    assert O.same_bits((with_td.g4, with_td.q), (without.g4, without.q)) and torch.equal(with_td.stats, without.stats)


def test_finished_rows_keep_their_next_values_out_and_double_q_reads_the_online_rows_for_the_choice_alone():
    B, nA = Q.HEAD_SHAPES[2]
    form = ("independent", True, Q.DELTA, True)
    inp, *_ = Q.head_case(B, nA, form)
    over = inp["done"] != 0
    assert 20 < int(over.sum()) < B * nA - 20
    base, _ = Q.guarded_head(inp, form)
    nan4 = torch.full((4,), O.NAN)
    poisoned = dict(inp, y_next_target=torch.where(over[..., None], nan4, inp["y_next_target"]),
                    y_next_online=torch.where(over[..., None], nan4, inp["y_next_online"]))
    out, _ = Q.guarded_head(poisoned, form)
    assert O.same_bits(base[:3], out[:3]) and torch.equal(base.stats, out.stats) and bool(torch.isfinite(out.stats).all())
    # scaling the online rows by a positive number moves no choice and so no bit; without double Q they are not read at all
    scaled, _ = Q.guarded_head(dict(inp, y_next_online=inp["y_next_online"] * 0.5), form)
    assert O.same_bits(base[:3], scaled[:3])
    single = ("independent", False, Q.DELTA, True)
    a, _ = Q.guarded_head(inp, single)
    b, _ = Q.guarded_head(dict(inp, y_next_online=torch.full_like(inp["y_next_online"], O.NAN)), single)
    assert O.same_bits(a[:3], b[:3]) and not O.same_bits((a.td,), (base.td,))
