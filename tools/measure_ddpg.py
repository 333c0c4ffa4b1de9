#!/usr/bin/env python3
"""Writes profiles/ddpg_float64.json: what the DDPG tests read beside their code (tests/ddpg_util.py).

    python tools/measure_ddpg.py [--ratios FILE]     # the CPU part; with a GPU also the learner's side of the bandit

  factors   per tensor of the TD head a (mean, max) factor wider than the project's (2, 4), with its reason: none is needed
  bandit    the learning check of tests/test_hip_ddpg_learner.py: the update count N, chosen HERE with the torch composition alone -- the
            smallest candidate from which on it closes at least 60 % of the gap from its initial held-out reward to 0 (the test asks half) --,
            what the torch composition reaches at every candidate, and, with a GPU, what N captured DDPGLearner updates reach from the
            same initial weights
  stepped   the whole-update case of tests/test_hip_ddpg_learner.py (ddpg_util.stepped_case), all on the CPU: per shape the seed, the share
            of elements the kink filter leaves out and its zeroing rounds; how far each misreading of the update lies from the float64
            reference; the float32 yardstick's own spread on both gradients over 8 row orders (ddpg_util.stepped_spread) and the factors
            yardstick_util.exceptions_from makes of it.  --ratios: a file of JSON lines the GPU test appended under BSX_DDPG_RATIOS_OUT,
            kept as "kernel"
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ddpg_util as D  # noqa: E402
import offpolicy_util as O  # noqa: E402


def bandit_learner(N):
    from deep_rl_battlespace_amd.learner import DDPGLearner
    b = O.BANDIT
    make = lambda ring, actor, critic: DDPGLearner(ring, actor, critic, critic_input="own", tau=b["tau"], lr_actor=b["lr"], lr_critic=b["lr"],     # noqa: E731
                                                   updates=10)
    return O.bandit_learner_reward(make, O.bandit_nets(), N)[1]


def main():
    old = json.load(open(D.PROFILE)) if os.path.exists(D.PROFILE) else {}
    bandit = O.bandit_section(old, D.bandit_torch_run, bandit_learner, O.BANDIT)
    cases, sharp, spread = {}, {}, {}
    for shape in D.LEARNER_SHAPES:
        c, sid = D.stepped_case(shape), D.shape_id(shape)
        cases[sid] = dict(seed=c.seed, left_out_percent=round(100 * c.share, 2), zeroing_rounds=c.rounds)
        sharp[sid] = O.sharpness(D.wrong_variants(c, shape[4]))
        spread[sid] = {which: O.rounded(s, 3) for which, s in D.stepped_spread(shape).items()}     # (three digits: as first recorded)
    stepped = dict(
        what="tests/ddpg_util.py stepped_case: one whole update from target networks that are not the networks (each parameter + 0.05 randn), "
             "eps = 1e-3, float64 on the CPU; the float32 yardstick is the same computation in float32 on the CPU",
        seeds="per shape the first seed from 0 at which, on the float64 reference alone, the kink filter closes within 4 zeroing rounds and "
              "leaves out less than 5 % (ddpg_util.STEP_SEEDS says what each seed gave; one base for all shapes was looked for over 80 bases "
              "and not found)",
        cases=cases,
        sharpness_note="smallest ratio over w1, w2, w3, b3 of mean |wrong gradient - right gradient| to the yardstick's mean error, float64 on "
                       "the CPU (tests/test_ddpg_cpu.py asserts >= 1000)",
        sharpness=sharp,
        spread_note="how far the yardstick's own max / mean error on the critic's (gc) and the actor's (ga) gradient moves over 8 other orders "
                    "of the batch's rows (seeds 4000 + p; no kernel output enters): [max ratio, mean ratio].  b3 has one value per agent and "
                    "output and moves by up to 5.3 x / 5.0 x: factors holds mlp_grad_util.factor_rule of its largest spread under '*' for "
                    "every shape and both gradients; every other tensor stays below (2, 4) and keeps them",
        spread=spread, factors=D.stepped_exceptions(spread),
        kernel_note="measured on the MI355X by tests/test_hip_ddpg_learner.py (BSX_DDPG_RATIOS_OUT): [mean ratio, max ratio] of the kernel's "
                    "error to the float32 yardstick's against float64 -- gc / ga: the critic's and the actor's gradient row per tensor (bars 2 "
                    "and 4, b3 the factors above); critic / actor .p .m .v .target: parameters, moments and Polyak target after the step, "
                    "pooled over the ten tensors (bars 2 and 4)",
        kernel=O.kept_kernel(old))
    out = dict(factors={}, factors_note="g_q, g_pi and td hold the project's (2, 4) at every shape of tests/ddpg_util.py: no exception is recorded",
               bandit=bandit, stepped=stepped)
    json.dump(out, open(D.PROFILE, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "stepped"}, indent=1))
    print(json.dumps(cases, indent=1), json.dumps(sharp, indent=1), json.dumps(stepped["factors"], indent=1))


if __name__ == "__main__":
    main()
