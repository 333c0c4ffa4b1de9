#!/usr/bin/env python3
"""Writes profiles/td3_float64.json: what the TD3 tests read beside their code (tests/td3_util.py).

    python tools/measure_td3.py [--ratios FILE]     # the CPU part; with a GPU also the learner's side of the bandit

  head_spread, factors   per case of the twin TD head's test the float32 yardstick's own spread over equivalent float32 evaluations
            (td3_util.head_spread: the contract's association and 8 row orders; no kernel output enters) and the (mean, max) factors
            wider than the project's (2, 4) that yardstick_util.exceptions_from makes of it
  stepped   the whole-update case of tests/test_hip_td3_learner.py (td3_util.stepped_case), all on the CPU: per shape the seed, the share
            of elements the kink filter leaves out and its zeroing rounds; how far each misreading of the update lies from the float64
            reference, in yardstick mean errors (the smallest over w1, w2, w3, b3).  --ratios: a file of JSON lines the GPU test
            appended under BSX_TD3_RATIOS_OUT, kept as "kernel"
  bandit    the learning check: the update count N, chosen HERE with the torch composition of TD3 alone -- the smallest candidate from
            which on it closes at least 60 % of the gap from its initial held-out reward to 0 (the test asks half) --, what the
            composition reaches at every candidate, and, with a GPU, what N captured TD3Learner updates reach from the same weights
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ddpg_util as D  # noqa: E402
import td3_util as T  # noqa: E402
import yardstick_util as Y  # noqa: E402

CANDIDATES = (50, 100, 200, 400, 800)
DELAY = 2


def bandit_learner(N):
    from deep_rl_battlespace_amd.learner import TD3Learner
    b = D.BANDIT
    rows, held = D.bandit_rows()
    actor, critic = D.bandit_nets()
    learner = TD3Learner(D.ring(rows, b["B"]), D.gpu_copy(actor), D.gpu_copy(critic), D.gpu_copy(T.bandit_critic2()), critic_input="own",
                         tau=b["tau"], lr_actor=b["lr"], lr_critic=b["lr"], updates=10, policy_delay=DELAY).capture()
    for _ in range(N // 10):
        learner.update()
    with torch.no_grad():
        return float(D.bandit_reward(held, learner.actor(held.cuda()).cpu()).mean())


def main():
    path = os.path.join(ROOT, "profiles", "td3_float64.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    runs = {N: T.bandit_torch_run(N, policy_delay=DELAY) for N in CANDIDATES}
    closed = {N: (r1 - r0) / (0.0 - r0) for N, (r0, r1) in runs.items()}
    N = next(n for n in CANDIDATES if all(closed[m] >= 0.6 for m in CANDIDATES if m >= n))
    r0, r1 = runs[N]
    bandit = dict(D.BANDIT, policy_delay=DELAY, N=N, initial_reward=r0, torch_reward=r1, torch_closed=closed[N],
                  torch_closed_by_candidate={str(n): closed[n] for n in CANDIDATES})
    if torch.cuda.is_available():
        r = bandit_learner(N)
        bandit.update(learner_reward=r, learner_closed=(r - r0) / (0.0 - r0))
    elif old.get("bandit", {}).get("N") == N:                            # keep the learner's figures of an earlier GPU run
        bandit.update({k: old["bandit"][k] for k in ("learner_reward", "learner_closed") if k in old["bandit"]})
    head = {T.head_id(B, nA, w): {k: [round(float(x), 4) for x in v] for k, v in T.head_spread(B, nA, w).items()}
            for B, nA in T.HEAD_SHAPES for w in (True, False)}
    cases, sharp = {}, {}
    for shape in T.MAIN_SHAPES:
        c, sid = T.stepped_case(shape), D.shape_id(shape)
        cases[sid] = dict(seed=c.seed, left_out_percent=round(100 * c.share, 2), zeroing_rounds=c.rounds)
        sharp[sid] = {name: round(min(dist[p] / yard[p] for p in D.SHARP)) for name, (dist, yard) in T.wrong_variants(c, shape[4]).items()}
    stepped = dict(what="tests/td3_util.py stepped_case: one whole TD3 update (policy_delay = 1) from target networks that are not the "
                        "networks, injected smoothing noise, eps = 1e-3, float64 on the CPU; the float32 yardstick is the same in float32",
                   seeds="per shape the first seed from 0 at which, on the float64 reference alone, the kink filter closes within 4 zeroing "
                         "rounds and leaves out less than 5 % (td3_util.STEP_SEEDS says what each seed gave)",
                   cases=cases, sharpness=sharp, kernel=old.get("stepped", {}).get("kernel", {}))
    if "--ratios" in sys.argv:
        for line in open(sys.argv[sys.argv.index("--ratios") + 1]):
            rec = json.loads(line)
            stepped["kernel"][rec["shape"]] = rec["ratios"]
    out = dict(command="python tools/measure_td3.py [--ratios FILE]", head_spread=head, factors=Y.exceptions_from(head),
               factors_note="yardstick_util.factor_rule on head_spread: with ONE element (B = nA = 1) a tensor's error is one draw of a float32 "
                            "rounding, and the yardstick's own moves by more than (2, 4) between torch's association of the head and the "
                            "contract's (td: one fmaf against a multiply and an add); every other shape holds the project's (2, 4)",
               bandit=bandit, stepped=stepped)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
