#!/usr/bin/env python3
"""Writes profiles/ddpg_float64.json: what the DDPG tests read beside their code (tests/ddpg_util.py).

    python tools/measure_ddpg.py           # the CPU part; with a GPU also the learner's side of the bandit

  factors   per tensor of the TD head a (mean, max) factor wider than the project's (2, 4), with its reason: none is needed
  bandit    the learning check of tests/test_hip_ddpg_learner.py: the update count N, chosen HERE with the torch composition alone -- the
            smallest candidate from which on it closes at least 60 % of the gap from its initial held-out reward to 0 (the test asks half) --,
            what the torch composition reaches at every candidate, and, with a GPU, what N captured DDPGLearner updates reach from the
            same initial weights
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ddpg_util as D  # noqa: E402

CANDIDATES = (50, 100, 200, 400, 800)


def main():
    runs = {N: D.bandit_torch_run(N) for N in CANDIDATES}
    closed = {N: (r1 - r0) / (0.0 - r0) for N, (r0, r1) in runs.items()}
    N = next(n for n in CANDIDATES if all(closed[m] >= 0.6 for m in CANDIDATES if m >= n))
    r0, r1 = runs[N]
    bandit = dict(D.BANDIT, N=N, initial_reward=r0, torch_reward=r1, torch_closed=closed[N],
                  torch_closed_by_candidate={str(n): closed[n] for n in CANDIDATES})
    if torch.cuda.is_available():
        from deep_rl_battlespace_amd.learner import DDPGLearner
        b = D.BANDIT
        rows, held = D.bandit_rows()
        actor, critic = D.bandit_nets()
        learner = DDPGLearner(D.ring(rows, b["B"]), D.gpu_copy(actor), D.gpu_copy(critic), critic_input="own", tau=b["tau"], lr_actor=b["lr"],
                              lr_critic=b["lr"], updates=10).capture()
        for _ in range(N // 10):
            learner.update()
        with torch.no_grad():
            r = float(D.bandit_reward(held, learner.actor(held.cuda()).cpu()).mean())
        bandit.update(learner_reward=r, learner_closed=(r - r0) / (0.0 - r0))
    out = dict(factors={}, factors_note="g_q, g_pi and td hold the project's (2, 4) at every shape of tests/ddpg_util.py: no exception is recorded",
               bandit=bandit)
    path = os.path.join(ROOT, "profiles", "ddpg_float64.json")
    if not torch.cuda.is_available() and os.path.exists(path):          # keep the learner's figures of an earlier GPU run
        old = json.load(open(path)).get("bandit", {})
        if old.get("N") == N:
            bandit.update({k: old[k] for k in ("learner_reward", "learner_closed") if k in old})
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
