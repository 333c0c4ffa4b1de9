"""tests/yardstick_util.py, the one statement of the float64 yardstick's bars, pinned on synthetic arrays: where exactly a tensor and
a pooled list of tensors pass and fail, what 0 / 0, x / 0 and NaN do, the scalar floor, the row orders, and the rule from a recorded
spread to a recorded factor.  Errors are small multiples of U = 2^-24 on multiples of 1 / 16: every sum and quotient below is exact."""
import numpy as np
import pytest

import yardstick_util as Y

N, U = 32, 2.0 ** -24
REF = np.arange(N) / 16.0
SIGN = np.where(np.arange(N) % 2, 1.0, -1.0)
E_YARD = U * np.array([4.0] + [1.0] * 31)                          # the yardstick's errors: sum 35 U, max 4 U
E_GOT = U * np.array([16.0] + [2.0] * 23 + [1.0] * 8)              # exactly at the factors: sum 70 U, max 16 U
YARD = REF + SIGN * E_YARD
UP = lambda x: x + np.spacing(x)                                   # noqa: E731
FORMS = {"tensor": lambda x: x.reshape(4, 8), "pooled": lambda x: [x[:5].reshape(5, 1), x[5:]]}


@pytest.mark.parametrize("form", FORMS.values(), ids=list(FORMS))
def test_at_the_factors_passes_and_one_spacing_beyond_either_fails(form):
    fm, fx = Y.FACTORS
    ratios = lambda e: Y.error_ratios(form(REF + SIGN * e), form(REF), form(YARD))                 # noqa: E731
    assert (fm, fx) == (2.0, 4.0) and Y.errors(form(YARD), form(REF)) == (35 * U / N, 4 * U)
    assert ratios(E_GOT) == (fm, fx) and Y.within(ratios(E_GOT))
    assert not Y.within((UP(fm), fx)) and not Y.within((fm, UP(fx)))
    e = E_GOT.copy()
    e[0], e[1] = UP(E_GOT[0]), U                                   # the max one float64 spacing beyond, the mean below its bar
    assert ratios(e)[0] < fm and ratios(e)[1] == UP(fx) and not Y.within(ratios(e))
    e = E_GOT.copy()
    e[-1] = 2 * U                                                  # the mean beyond (71 / 35 of the yardstick's), the max at its bar
    assert ratios(e) == (71.0 / 35.0, fx) and not Y.within(ratios(e))
    assert Y.within((1.5, 7.0), (2.0, 8.0)) and not Y.within((1.5, 7.0))         # a recorded exception widens what it names only


@pytest.mark.parametrize("form", FORMS.values(), ids=list(FORMS))
def test_nothing_over_nothing_passes_something_over_nothing_fails_and_so_does_a_nan_anywhere(form):
    ref = form(REF)
    assert Y.error_ratios(ref, ref, ref) == (0.0, 0.0) and Y.within((0.0, 0.0))
    assert Y.error_ratios(form(REF + U), ref, ref) == (np.inf, np.inf) and not Y.within((np.inf, np.inf))
    for where in (0, N - 1):
        got = YARD.copy()
        got[where] = np.nan
        for yard in (YARD, REF):                                   # NaN / x and NaN / 0 both stay NaN
            r = Y.error_ratios(form(got), ref, form(yard))
            assert np.isnan(r).all() and not Y.within(r)
        assert Y.check_tensors([("exact", REF, REF, REF, Y.FACTORS), ("nan", got, REF, YARD, Y.FACTORS)])[1] == ["nan"]
    assert not Y.within((float("nan"), 1.0)) and not Y.within((1.0, float("nan")))


def test_the_scalar_bound_has_a_floor_of_half_a_float32_spacing():
    assert Y.scalar_bound(1.0, 0.0) == 4 * 2.0 ** -24 == Y.scalar_bound(-1.0, 0.0)
    assert Y.scalar_bound(1.0, 2.0 ** -20) == 4 * 2.0 ** -20
    assert Y.scalar_bound(np.array([[0.25, -3.0], [1.0, 0.0]]), 0.0) == 4 * 2.0 ** -23           # an array: the spacing at max|ref| = 3
    got, ref, e = np.zeros(8), np.zeros(8), np.zeros(8)
    ref[1], e[2] = 1.0, 2.0 ** -20
    got[1:3] = 1.0 + 4 * 2.0 ** -24, UP(4 * 2.0 ** -20)
    assert Y.stats_out_of_bounds(got, ref, e, ("at_the_floor", "beyond")) == ["beyond"]
    got[1] = np.nan
    assert Y.stats_out_of_bounds(got, ref, e, ("nan", "beyond")) == ["nan", "beyond"]


def test_the_row_orders_are_the_given_one_and_eight_seeded_permutations():
    assert list(Y.row_orders(1)) == [None]
    orders = list(Y.row_orders(5))
    assert orders[0] is None and len(list(Y.row_orders(5, perms=2))) == 3
    assert [o.tolist() for o in orders[1:]] == [[2, 0, 4, 3, 1], [1, 4, 3, 2, 0], [0, 1, 3, 2, 4], [2, 4, 0, 1, 3], [1, 0, 3, 4, 2],
                                                [0, 3, 1, 2, 4], [4, 1, 2, 0, 3], [1, 3, 4, 0, 2]]          # what every recorded e_stats was drawn with
    # own_error: per key, element by element the largest error over the orders
    run = lambda order: dict(stats=np.array([1.0, 2.0]) + (0.0 if order is None else float(order[0])), g=np.array([5.0]))     # noqa: E731
    ref = dict(stats=np.array([1.0, 1.0]), g=np.array([4.5]))
    assert [e.tolist() for e in Y.own_error(run, ref, 5, perms=3, keys=("stats", "g"))] == [[2.0, 3.0], [0.5]]
    assert [e.tolist() for e in Y.own_error(run, ref, 1)] == [[0.0, 1.0]]


def test_a_recorded_spread_becomes_a_factor_only_where_it_reaches_the_factors():
    assert Y.factor_rule(3.99, 1.99) == (2.0, 4.0) and Y.factor_rule(4.0, 1.0) == (2.0, 8.0) and Y.factor_rule(1.0, 3.0) == (6.0, 4.0)
    calm, b3 = [3.99, 1.99], [5.0, 1.0]
    flat = {"one": {"w1": calm, "x": [4.0, 1.0], "b3": [1.1, 1.0]}, "two": {"w1": [1.0, 3.0], "b3": b3}, "three": {"w1": calm, "b3": [1.0, 1.0]}}
    assert Y.exceptions_from(flat) == {"one": {"x": [2.0, 8.0]}, "two": {"w1": [6.0, 4.0]}, "*": {"b3": [2.0, 10.0]}}         # b3 filed once, under "*"
    nested = {"s": {"gc": {"w2": [4.5, 1.0], "b3": [1.1, 1.0]}, "ga": {"w2": calm}}, "t": {"gc": {"w2": calm}, "ga": {"b3": b3, "w3": calm}}}
    assert Y.exceptions_from(nested) == {"s": {"gc": {"w2": [2.0, 9.0]}}, "*": {"b3": [2.0, 10.0]}}
    assert Y.exceptions_from({"s": {"w1": calm, "b3": calm}}) == {} == Y.exceptions_from({}) == Y.exceptions_from({"s": {}})
    own, star = {"x": [2.0, 8.0]}, {"b3": [2.0, 10.0], "x": [2.0, 5.0]}           # a case's exception, the one under "*", else FACTORS
    assert [Y.factor_of(own, star)(k) for k in ("x", "b3", "w1")] == [(2.0, 8.0), (2.0, 10.0), Y.FACTORS] and Y.factor_of({})("x") == Y.FACTORS
