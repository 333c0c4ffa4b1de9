#!/usr/bin/env python3
"""Writes profiles/td3_float64.json: what the TD3 tests read beside their code (tests/td3_util.py).

    python tools/measure_td3.py [--ratios FILE]     # the CPU part; with a GPU also the learner's side of the bandit

  head_spread, factors   per case of the twin TD head's test the float32 yardstick's own spread over equivalent float32 evaluations
            (td3_util.HEAD.spread: the contract's association and 8 row orders; no kernel output enters) and the (mean, max) factors
            wider than the project's (2, 4) that yardstick_util.exceptions_from makes of it
  stepped   the whole-update case of tests/test_hip_td3_learner.py (td3_util.stepped_case), all on the CPU: per shape the seed, the share
            of elements the kink filter leaves out and its zeroing rounds; how far each misreading of the update lies from the float64
            reference, in yardstick mean errors (the smallest over w1, w2, w3, b3; with more than one agent also the agent-index
            misreading, the smoothing normals of agent j - 1).  --ratios: a file of JSON lines the GPU test
            appended under BSX_TD3_RATIOS_OUT, kept as "kernel"
  bandit    the learning check: the update count N, chosen HERE with the torch composition of TD3 alone -- the smallest candidate from
            which on it closes at least 60 % of the gap from its initial held-out reward to 0 (the test asks half) --, what the
            composition reaches at every candidate, and, with a GPU, what N captured TD3Learner updates reach from the same weights
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ddpg_util as D  # noqa: E402
import offpolicy_util as O  # noqa: E402
import td3_util as T  # noqa: E402

DELAY = 2


def bandit_learner(N):
    from deep_rl_battlespace_amd.learner import TD3Learner
    b = O.BANDIT
    make = lambda ring, *nets: TD3Learner(ring, *nets, critic_input="own", tau=b["tau"], lr_actor=b["lr"], lr_critic=b["lr"], updates=10,     # noqa: E731
                                          policy_delay=DELAY)
    return O.bandit_learner_reward(make, O.bandit_nets(critic2="reseeded"), N)[1]


def main():
    old = json.load(open(T.PROFILE)) if os.path.exists(T.PROFILE) else {}
    bandit = O.bandit_section(old, lambda N: T.bandit_torch_run(N, policy_delay=DELAY), bandit_learner, dict(O.BANDIT, policy_delay=DELAY))
    head, factors = O.head_sections(T.HEAD, T.HEAD_SHAPES)
    cases, sharp = {}, {}
    for shape in T.STEP_SHAPES:
        c, sid = T.stepped_case(shape), D.shape_id(shape)
        cases[sid] = dict(seed=c.seed, left_out_percent=round(100 * c.share, 2), zeroing_rounds=c.rounds)
        sharp[sid] = O.sharpness(T.wrong_variants(c, shape[4]))
    stepped = dict(what="tests/td3_util.py stepped_case: one whole TD3 update (policy_delay = 1) from target networks that are not the "
                        "networks, injected smoothing noise, eps = 1e-3, float64 on the CPU; the float32 yardstick is the same in float32",
                   seeds="per shape the first seed from 0 at which, on the float64 reference alone, the kink filter closes within 4 zeroing "
                         "rounds and leaves out less than 5 % (td3_util.STEP_SEEDS says what each seed gave)",
                   cases=cases, sharpness=sharp, kernel=O.kept_kernel(old))
    out = dict(command="python tools/measure_td3.py [--ratios FILE]", head_spread=head, factors=factors,
               factors_note="yardstick_util.factor_rule on head_spread: with ONE element (B = nA = 1) a tensor's error is one draw of a float32 "
                            "rounding, and the yardstick's own moves by more than (2, 4) between torch's association of the head and the "
                            "contract's (td: one fmaf against a multiply and an add); every other shape holds the project's (2, 4)",
               bandit=bandit, stepped=stepped)
    json.dump(out, open(T.PROFILE, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
