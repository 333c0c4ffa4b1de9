#!/usr/bin/env python3
"""Writes profiles/sac_float64.json: what the SAC tests read beside their code (tests/sac_util.py).

    python tools/measure_sac.py [--ratios FILE]     # the CPU part; with a GPU also the learner's side of the bandit

  head_spread, factors   per case of the soft twin head's test the float32 yardstick's own spread over equivalent float32 evaluations
            (sac_util.head_spread: the contract's association and 8 row orders; no kernel output enters) and the (mean, max) factors
            wider than the project's (2, 4) that yardstick_util.exceptions_from makes of it
  stepped   the whole-update case of tests/test_hip_sac_learner.py (sac_util.stepped_case), all on the CPU: per shape every seed tried
            from 0 with the share of elements the kink filter left out and its zeroing rounds (closed: whether it reached a fixed
            point within ddpg_util.MAX_ROUNDS), the first seed that closes under actor_grad_util.KINK_CAP, and how far each misreading
            of the update lies from the float64 reference, in yardstick mean errors (the smallest over the tensors compared).
            --ratios: a file of JSON lines the GPU test appended under BSX_SAC_RATIOS_OUT, kept as "kernel"
            spread, factors: the float32 yardstick's own spread on log_std's and log_alpha's gradients over 8 row orders and the factors
            yardstick_util.exceptions_from makes of it (the other rows and steps hold the project's (2, 4))
  bandit    the learning check at k = 3 with a fixed temperature: the update count N, chosen HERE with the torch composition of SAC
            alone -- the smallest candidate from which on it closes at least 60 % of the gap from its initial held-out reward to 0 (the
            test asks half) --, and, with a GPU, what N captured SACLearner updates reach from the same weights
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ddpg_util as D  # noqa: E402
import sac_util as S  # noqa: E402
import yardstick_util as Y  # noqa: E402

CANDIDATES = (50, 100, 200, 400, 800)
MAX_SEEDS = 1500


def bandit_learner(N):
    from deep_rl_battlespace_amd.learner import SACLearner
    b = S.BANDIT
    rows, held = S.bandit_rows()
    nets = [D.gpu_copy(n) for n in S.bandit_nets()]
    learner = SACLearner(D.ring(rows, b["B"]), *nets, critic_input="own", alpha=b["alpha"], lr_alpha=None, tau=b["tau"], lr_actor=b["lr"],
                         lr_critic=b["lr"], updates=10).capture()
    for _ in range(N // 10):
        learner.update()
    with torch.no_grad():
        return float(D.bandit_reward(held, learner.actor(held.cuda()).cpu()).mean())


def main():
    path = os.path.join(ROOT, "profiles", "sac_float64.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    runs = {N: S.bandit_torch_run(N) for N in CANDIDATES}
    closed = {N: (r1 - r0) / (0.0 - r0) for N, (r0, r1) in runs.items()}
    N = next(n for n in CANDIDATES if all(closed[m] >= 0.6 for m in CANDIDATES if m >= n))
    r0, r1 = runs[N]
    bandit = dict(S.BANDIT, N=N, initial_reward=r0, torch_reward=r1, torch_closed=closed[N],
                  torch_closed_by_candidate={str(n): closed[n] for n in CANDIDATES})
    if torch.cuda.is_available():
        r = bandit_learner(N)
        bandit.update(learner_reward=r, learner_closed=(r - r0) / (0.0 - r0))
    elif old.get("bandit", {}).get("N") == N:                            # keep the learner's figures of an earlier GPU run
        bandit.update({k: old["bandit"][k] for k in ("learner_reward", "learner_closed") if k in old["bandit"]})
    head = {S.head_id(B, nA, w): {k: [round(float(x), 4) for x in v] for k, v in S.head_spread(B, nA, w).items()}
            for B, nA in S.HEAD_SHAPES for w in (True, False)}
    cases, sharp, spread = {}, {}, {}
    for shape in S.MAIN_SHAPES:
        sid, tried = D.shape_id(shape), []
        for seed in range(MAX_SEEDS):
            c, share, rounds = S.try_seed(shape, seed)
            tried.append([seed, c is not None, round(100 * share, 2), rounds])
            if c is not None and share < D.U.KINK_CAP:
                break
        cases[sid] = dict(shape=list(shape), seed=seed, left_out_percent=round(100 * share, 2), zeroing_rounds=rounds,
                          tried="[seed, closed, percent left out, zeroing rounds]", seeds_tried=tried)
        S.STEP_SEEDS[tuple(shape)] = seed
        spread[sid] = {k: [round(float(x), 4) for x in v] for k, v in S.stepped_spread(shape).items()}
        sharp[sid] = {name: round(min(dist[p] / yard[p] for p in dist)) for name, (dist, yard) in S.wrong_variants(S.stepped_case(shape), shape[4]).items()}
    stepped = dict(what="tests/sac_util.py stepped_case: one whole SAC update from target critics that are not the critics, injected normals "
                        "for both draws, eps = 1e-3, float64 on the CPU; the float32 yardstick is the same in float32",
                   seeds="per shape the first seed from 0 at which, on the float64 reference alone, the kink filter closes within 4 zeroing "
                         "rounds and leaves out less than 5 %.  Zeroing a row moves both stepped critics by far more than the kink "
                         "margin (Adam's first step), so at 2v2 every round finds about five fresh rows among 322 and a fixed point is "
                         "reached only where a round finds none",
                   cases=cases, sharpness=sharp, spread=spread, factors=Y.exceptions_from(spread),
                   factors_note="yardstick_util.factor_rule on spread (sac_util.stepped_spread: the yardstick's own error on log_std's and "
                                "log_alpha's gradients over 8 row orders): with one agent these are three numbers and one",
                   kernel=old.get("stepped", {}).get("kernel", {}))
    if "--ratios" in sys.argv:
        for line in open(sys.argv[sys.argv.index("--ratios") + 1]):
            rec = json.loads(line)
            stepped["kernel"][rec["shape"]] = rec["ratios"]
    out = dict(command="python tools/measure_sac.py [--ratios FILE]", head_spread=head, factors=Y.exceptions_from(head),
               factors_note="yardstick_util.factor_rule on head_spread: with ONE element (B = nA = 1) a tensor's error is one draw of a float32 "
                            "rounding, and the yardstick's own moves by more than (2, 4) between torch's association of the head and the "
                            "contract's; every other shape holds the project's (2, 4)",
               bandit=bandit, stepped=stepped)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "stepped"}, indent=1))
    print(json.dumps({k: {a: b for a, b in v.items() if a != "seeds_tried"} for k, v in cases.items()}, indent=1), json.dumps(sharp, indent=1))


if __name__ == "__main__":
    main()
