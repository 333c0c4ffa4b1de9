#!/usr/bin/env python3
"""What each precision mode of the actor kernel loses against a float64 reference, for every input class, team size and mode of
tests/test_hip_actor_float64.py (the same inputs, through tests/actor_ref_util.py):

    python tools/micro/actor_precision.py [--out profiles/actor_float64.json]

Per (class, n, mode): max / mean |error| of the kernel's head sums before tanh (e_k), of torch float32 on the CPU (e_t) and of the
float64 model of the mode's bf16 split (e_m), the bounds the test holds e_k to, and the max |error| of the tanh scores overall and on the
outputs with |y64| < 1.  Needs the MI355X."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import actor_ref_util as au                                   # noqa: E402
import test_hip_actor_float64 as t64                          # noqa: E402  (the test's own inputs: the shipped class with its played rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_float64.json"))
    args = ap.parse_args()
    rows = []
    for cls, n in au.COMBOS:
        actor, obs, y, e_t, e_m2, e_m3 = t64._dense(cls, n)
        for mode in au.MODES:
            scores, sums = au.kernel_outputs(actor, obs, n, mode)
            e_k = np.abs(sums - y)
            e_m = t64._model_err(mode, e_t, e_m2, e_m3)
            bmax, bmean = au.bounds(mode, e_t, e_m2, e_m3)
            e_s = np.abs(scores - np.tanh(y))
            body = np.abs(y) < 1
            r = dict(cls=cls, n=n, mode=mode, games=int(obs.shape[0]), outputs=int(y.size), max_abs_head_sum=float(np.abs(y).max()),
                     outputs_below_1=int(body.sum()),
                     e_k_max=float(e_k.max()), e_k_mean=float(e_k.mean()), e_t_max=float(e_t.max()), e_t_mean=float(e_t.mean()),
                     e_m_max=float(e_m.max()), e_m_mean=float(e_m.mean()), bound_max=float(bmax), bound_mean=float(bmean),
                     score_err_max=float(e_s.max()), score_err_max_below_1=float(e_s[body].max()),
                     within_bounds=bool(e_k.max() <= bmax and e_k.mean() <= bmean))
            rows.append(r)
            print(f"{cls:13s} n={n} {mode:6s} e_k {r['e_k_max']:.2e} / {r['e_k_mean']:.2e}  e_t {r['e_t_max']:.2e} / {r['e_t_mean']:.2e}  "
                  f"e_m {r['e_m_max']:.2e} / {r['e_m_mean']:.2e}  score {r['score_err_max']:.2e}", flush=True)
    doc = dict(what="actor kernel (bsx_actor_forward) against a float64 reference: |error| of the head sums before tanh, max / mean; "
                    "e_k kernel, e_t torch float32 (CPU), e_m float64 model of the mode's bf16 split; bounds as tests/test_hip_actor_float64.py",
               command="python tools/micro/actor_precision.py", device="MI355X (gfx950)", rows=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
