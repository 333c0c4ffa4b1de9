"""The float64 yardstick's bars, stated once for every learner-kernel test.  A kernel's `got` is held to a float64 reference `ref` by
what `yard`, a float32 torch evaluation of the same thing, loses on the same inputs:
  errors, error_ratios, within   a tensor, or a list of tensors pooled as one vector: mean|got - ref| <= fm mean|yard - ref| and
                     max|got - ref| <= fx max|yard - ref|, (fm, fx) = FACTORS
  scalar_bound, row_orders, own_error   a scalar statistic: within 4 x the yardstick's own error over nine orders of the rows (the given
                     one and 8 seeded permutations), at least half a float32 spacing
  factor_rule, exceptions_from   the one way a factor widens: where a recorded spread of the yardstick itself reaches (fm, fx)
  recorded, factor_of   what a profile records: a case's exception, the one under "*", else FACTORS
  check_tensors, stats_out_of_bounds   print every figure, return what is out of bounds
numpy only but for torch.randperm; nothing here imports the native library."""
import json
import os

import numpy as np
import torch

# Where 2 and 4 come from: across summation orders of the same float32 network on the CPU the mean error moved by at most 1.13x and the
# max by at most 1.3x; rsqrtf and packed FMAs cost a few ulp more; the next-worse arithmetic (two bf16 terms instead of float32) loses
# 16 to 24 times more.  The factors are conditions, not fits.
FACTORS = (2.0, 4.0)          # mean(e_k) <= 2 mean(e_t), max(e_k) <= 4 max(e_t)


def errors(x, ref):
    """(mean, max) of |x - ref| in float64: of one array, or of a list of arrays pooled as ONE vector (an optimiser step is element-wise:
    a per-tensor maximum over the eight floats of a b3 is noise)."""
    if isinstance(x, (list, tuple)):
        e = np.concatenate([np.abs(np.asarray(a, np.float64) - np.asarray(r, np.float64)).ravel() for a, r in zip(x, ref)])
    else:
        e = np.abs(np.asarray(x, np.float64) - np.asarray(ref, np.float64))
    return float(e.mean()), float(e.max())


def error_ratios(got, ref, yard):
    """(mean|got - ref| / mean|yard - ref|, max|got - ref| / max|yard - ref|); 0 / 0 counts as 0, x / 0 as inf, and NaN stays NaN."""
    return tuple(k / t if t > 0 else (0.0 if k == 0 else k * float("inf")) for k, t in zip(errors(got, ref), errors(yard, ref)))


def within(ratios, factors=FACTORS):
    """Both ratios at or below their factors, written so that a NaN fails."""
    return bool(ratios[0] <= factors[0] and ratios[1] <= factors[1])


def scalar_bound(ref, own_error):
    """4 x the yardstick's own error on a statistic -- but a float32 value cannot be expected closer to float64 than half a float32
    spacing at its size, whatever the nine orders happened to hit.  ref: the float64 scalar, or an array (the spacing at max|ref|)."""
    return FACTORS[1] * max(float(own_error), 0.5 * float(np.spacing(np.float32(np.abs(ref).max()))))


def row_orders(rows, perms=8):
    """The orders a sum over `rows` rows is taken in: None (the given one), then `perms` permutations; one row has the given order only."""
    yield None
    for p in range(perms if rows > 1 else 0):
        yield torch.randperm(rows, generator=torch.Generator().manual_seed(4000 + p))


def own_error(run, ref, rows, perms=8, keys=("stats",)):
    """The yardstick's own error: per key, element by element the largest |run(order)[key] - ref[key]| over row_orders."""
    runs = [run(order) for order in row_orders(rows, perms)]
    return [np.maximum.reduce([np.abs(r[k] - ref[k]) for r in runs]) for k in keys]


def factor_rule(max_spread, mean_spread):
    """(fm, fx) from a tensor's recorded yardstick spread: FACTORS while the spread stays below them; where the yardstick's own mean
    moves by 2x or its max by 4x under an equivalent float32 evaluation, twice the recorded spread (what profiles/
    actor_grad_float64.json does for b3), never less than FACTORS."""
    if mean_spread < FACTORS[0] and max_spread < FACTORS[1]:
        return FACTORS
    return (max(FACTORS[0], round(2 * mean_spread, 2)), max(FACTORS[1], round(2 * max_spread, 2)))


def exceptions_from(spreads):
    """The factors a profile may record, from spreads nested to any depth over leaves {tensor: (max ratio, mean ratio)} -- {case: leaf},
    {shape: {"gc" / "ga": leaf}} --: the same nesting over {tensor: [fm, fx]}, factor_rule wherever it is not FACTORS.  b3, the tensor
    with one value per agent and output, gets ONE pair for all, under "*": the rule on its largest spread."""
    b3 = [1.0, 1.0]

    def walk(node):
        if all(isinstance(v, dict) for v in node.values()):
            return {k: w for k, w in ((k, walk(v)) for k, v in node.items()) if w}
        b3[:] = [max(a, b) for a, b in zip(b3, node.get("b3", b3))]
        return {k: list(factor_rule(*v)) for k, v in node.items() if k != "b3" and factor_rule(*v) != FACTORS}
    out = walk(spreads)
    if factor_rule(*b3) != FACTORS:
        out["*"] = {"b3": list(factor_rule(*b3))}
    return out


def recorded(profile, *path):
    """What the JSON file `profile` holds under the keys of `path`; {} where the file or a key is missing."""
    node = json.load(open(profile)) if os.path.exists(profile) else {}
    for key in path:
        node = node.get(key, {})
    return node


def factor_of(own, star={}):
    """name -> (fm, fx): the exception recorded for the case itself (`own`), the one recorded under "*" (`star`), or FACTORS."""
    return lambda name: tuple(own.get(name, star.get(name, FACTORS)))


LINES = {"ratios": "{what} {k}: mean ratio {rm:.3f} (<= {fm}), max ratio {rx:.3f} (<= {fx}), max error / max|g| {rel:.2e}",
         "errors": "{what} {k}: kernel mean / max error {em:.3e} / {ex:.3e}, yardstick {tm:.3e} / {tx:.3e} (factors {fm}, {fx}); "
                   "max|{unit}| {size:.3e}",
         "pooled": "{what} {k}: mean ratio {rm:.3f} (<= {fm:g}), max ratio {rx:.3f} (<= {fx:g})"}


def check_tensors(items, what="", line="errors", unit="g"):
    """items: (name, got, ref, yard, (fm, fx)) per tensor, or per list of tensors pooled.  Prints every figure in the form LINES[line] ->
    ({name: (mean ratio, max ratio, max error / max|ref|)}, the names out of bounds)."""
    out, bad = {}, []
    for k, got, ref, yard, (fm, fx) in items:
        (em, ex), (tm, tx), (rm, rx) = errors(got, ref), errors(yard, ref), error_ratios(got, ref, yard)
        size = max(float(np.abs(r).max()) for r in (ref if isinstance(ref, (list, tuple)) else [ref]))
        out[k] = (rm, rx, ex / max(size, 1e-300))
        print(LINES[line].format(what=what, k=k, unit=unit, em=em, ex=ex, tm=tm, tx=tx, rm=rm, rx=rx, fm=fm, fx=fx, size=size, rel=out[k][2]))
        if not within((rm, rx), (fm, fx)):
            bad.append(k)
    return out, bad


def stats_out_of_bounds(got, ref, e_stats, names, what=""):
    """got, ref, e_stats: float64 statistics rows; names: of entries 1 .. len(names), each held to scalar_bound of the yardstick's own
    error.  Prints every figure -> the names out of bounds."""
    bad = []
    for i, name in enumerate(names, start=1):
        tol, err = scalar_bound(ref[i], e_stats[i]), abs(got[i] - ref[i])
        print(f"{what} stats.{name}: float64 {ref[i]:.9g}, kernel error {err:.3e}, yardstick's own (9 row orders) {e_stats[i]:.3e}, bound {tol:.3e}")
        if not err <= tol:
            bad.append(name)
    return bad
