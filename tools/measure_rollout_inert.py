#!/usr/bin/env python3
"""Measure the cases of tests/test_hip_rollout_inert.py on the card and write profiles/rollout_inert.json.

    python tools/measure_rollout_inert.py [--out profiles/rollout_inert.json]

Per case and form of ORACLE_RUNS: the env seeds (41, 42, 43, 44) tried in order until the ORACLE's flags meet the coverage conditions
(`_coverage`: a game ended strictly inside a run, a run was inert throughout, a block of 32 games held a running, an inert and a
freshly re-spawned game at once, and -- where the tie falls on a run's last tick -- a game ended at tick T - 1 and was re-spawned
before the next run), with what every seed tried gave.  A parity assertion that fails is recorded (`ok: false` with the assertion),
never skipped.  Then the form pairs and the GAE / replay tests as pytest runs them, with the figures they leave in FIGURES.  A seed
other than the one the test file names for a case is a finding: put it into SEEDS there, with the reason."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_inert.json"))
    args = ap.parse_args()
    import test_hip_rollout_inert as M
    out = {
        "what": "tests/test_hip_rollout_inert.py on an MI355X: PolicyRollout on an env without auto-reset beside the C oracle, one schedule "
                "per case (until the time-limit tie has ended every game, one all-inert run, two partial re-spawns by hand)",
        "seed_rule": "env seed 41 where the oracle's flags meet the coverage conditions with it, else the first of (41, 42, 43, 44) that does",
        "keys": "counts over the whole schedule, from the oracle's flags: games that ended at a tick 0 < t < T - 1 / at tick T - 1, runs and rows "
                "(game x tick) that were inert, host re-spawns and the games they re-spawned, aligned blocks of 32 games that held a running, "
                "an inert and a freshly re-spawned game at a re-spawn, games re-spawned right after ending on a run's last tick, re-spawned "
                "games whose OU rows still held the finished game's state when start() was called",
        "cases": {}, "forms_agree": {}, "gae_and_replay": {}}
    for case, form in M.ORACLE_RUNS:
        c = out["cases"][f"{case}/{form}"] = {"seed_in_test": M.SEEDS.get((case, form), 41), "seeds_tried": {}}
        t0, chosen = time.time(), None
        for seed in SEEDS:
            try:
                fig = M.play_against_the_oracle(case, form, seed)
                c["seeds_tried"][str(seed)] = fig
                chosen, c["ok"] = seed, True
                break
            except M.CoverageMiss as exc:
                c["seeds_tried"][str(seed)] = {"coverage_miss": str(exc)[:600]}
            except AssertionError:
                chosen, c["ok"], c["assertion"] = seed, False, traceback.format_exc()[-1500:]
                break
        c["chosen_seed"], c["seconds"] = chosen, round(time.time() - t0, 2)
        print(case, form, "seed", chosen, "ok" if c.get("ok") else "NOT OK", f"{c['seconds']:.1f} s", flush=True)
        json.dump(out, open(args.out, "w"), indent=1)
    for case, a, b in M.FORM_PAIRS:
        t0, r = time.time(), {}
        try:
            M.test_forms_agree_bit_for_bit_without_auto_reset(case, a, b)
            r["ok"] = True
        except AssertionError:
            r["ok"], r["assertion"] = False, traceback.format_exc()[-1500:]
        r["seconds"] = round(time.time() - t0, 2)
        out["forms_agree"][f"{case}/{a}-vs-{b}"] = r
        print(case, a, b, "ok" if r["ok"] else "NOT OK", f"{r['seconds']:.1f} s", flush=True)
        json.dump(out, open(args.out, "w"), indent=1)
    for n, form in ((1, "one_launch"), (2, "graph")):
        t0, r = time.time(), {}
        try:
            M.test_gae_and_replay_ring_over_records_without_auto_reset(n, form)
            r["ok"] = True
        except AssertionError:
            r["ok"], r["assertion"] = False, traceback.format_exc()[-1500:]
        r.update(M.FIGURES.get(f"gae+replay/{n}v{n}/{form}", {}), seconds=round(time.time() - t0, 2))
        out["gae_and_replay"][f"{n}v{n}/{form}"] = r
        print("gae + replay", n, form, "ok" if r["ok"] else "NOT OK", f"{r['seconds']:.1f} s", flush=True)
        json.dump(out, open(args.out, "w"), indent=1)
    bad = [k for part in ("cases", "forms_agree", "gae_and_replay") for k, v in out[part].items() if not v.get("ok")]
    print("not ok:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
