#!/usr/bin/env python3
"""Measure the configurations of tests/test_hip_ppo_learner.py on the card and write profiles/ppo_learner_float64.json.

    python tools/measure_ppo_learner.py [--out profiles/ppo_learner_float64.json]

Per configuration of CONFIGS / OPPONENT_CONFIGS (T = 8): the env seeds (41, 42, 43, 44) tried in order until the float64 reference
alone meets the row conditions of the float64 minibatch test (kept >= 0.9 masked, kept >= 500, 5 % .. 60 % of the kept rows clipped,
at most KINK_CAP of the masked rows near a ReLU kink) with the figures of every seed tried; at the chosen seed the test's own
machinery (`_minibatch_against_float64`: the largest mean and max ratios per network, the loss and log_std errors over torch's own) and
the on-policy test (its ratios for the recorded and the recomputed logp / value, and what bf16x3 scores would cost the ratio), both read
from the tests' FIGURES.  A bound that is missed is recorded (`*_ok: false` with the assertion), never widened.  A seed other than the
one a configuration names in the test file is a finding: put it there, with the reason."""
import argparse
import json
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEEDS = (41, 42, 43, 44)


def _round(x):
    if isinstance(x, float):
        return float(f"{x:.4g}")
    if isinstance(x, dict):
        return {k: _round(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_round(v) for v in x]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_learner_float64.json"))
    args = ap.parse_args()
    import ppo_learner_util as L
    import test_hip_ppo_learner as M
    out = {
        "what": "tests/test_hip_ppo_learner.py on an MI355X: one PPOLearner minibatch over a PolicyRollout's own records against the float64 "
                "torch loss (`_ppo` of tests/actor_grad_util.py), and the records on the policy that played, per configuration; T = 8",
        "bounds": "unchanged: per gradient tensor (2 x mean, 4 x max) of torch float32's own error (actor_grad_util.check), the loss and "
                  "log_std's gradient within 4 x torch's own error over 9 row orders; rows: kept >= 0.9 masked, kept >= 500, 5 % .. 60 % of "
                  "the kept rows clipped, at most KINK_CAP = 5 % of the masked rows near a ReLU kink -- on the float64 reference alone",
        "seed_rule": "env seed 41 (the fixture's) where the float64 reference meets the row conditions with it, else the first of "
                     "(41, 42, 43, 44) that does",
        "keys": "float64.*_ratio: the largest over the ten tensors of a network of mean(e_learner) / mean(e_torch32) and max / max; "
                "on_policy.<record>: (mean ratio, max ratio) over the masked rows of every tick, bounds (2, 4); ratio_error_f32 / _bf16x3: "
                "(mean, max) of |exp(logp - float64 logp) - 1| for the float32 record and for scores evaluated in bf16x3 (not bounded)",
        "configurations": {}}
    for name, (kind, kw, ticks) in {**M.CONFIGS, **M.OPPONENT_CONFIGS}.items():
        c = out["configurations"][name] = {"seed_in_test": kw.get("seed", 41), "seeds_tried": {}}
        cols = L.scripted_columns(kw.get("n", 1), kw["opponent"])[1] if kw.get("opponent") else None
        chosen, t0 = None, time.time()
        for seed in SEEDS:
            ro = L.small_rollout(kind, **dict(kw, seed=seed))
            a, b = ticks or (0, ro.T)
            fig = M._ppo_ladder(ro.actor, ro.value_actor, ro.log_std, L.record(ro, a, b), kind, cols)[4]
            fig["meets"] = bool(M._conditions(fig))
            c["seeds_tried"][str(seed)] = fig
            if fig["meets"]:
                chosen = seed
                break
        c["chosen_seed"] = chosen
        if chosen is not None:
            table = M.CONFIGS if name in M.CONFIGS else M.OPPONENT_CONFIGS
            table[name] = (kind, dict(kw, seed=chosen), ticks)
            try:
                ro = L.small_rollout(kind, **dict(kw, seed=chosen))
                c["float64"] = M._minibatch_against_float64(ro, kind, ticks, cols=cols, what=name)[0]
                c["float64_ok"] = True
            except AssertionError:
                c["float64_ok"], c["float64_assertion"] = False, traceback.format_exc()[-1200:]
            try:
                M.test_on_the_policy_that_played_nothing_is_clipped_and_the_records_meet_float64(name)
                c["on_policy_ok"] = True
            except AssertionError:
                c["on_policy_ok"], c["on_policy_assertion"] = False, traceback.format_exc()[-1200:]
            c["on_policy"] = M.FIGURES.get(name, {}).get("on_policy")
            c["masked_rows_all_ticks"] = M.FIGURES.get(name, {}).get("masked_all_ticks")
        c["seconds"] = time.time() - t0
        print(name, "seed", chosen, {k: v for k, v in c.items() if k.endswith("_ok")}, f"{c['seconds']:.1f} s", flush=True)
        json.dump(_round(out), open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
