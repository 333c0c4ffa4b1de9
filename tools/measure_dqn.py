#!/usr/bin/env python3
"""Writes the two profiles of the DQN learner (learner.DQNLearner; csrc/bsx_dqn_head.hip; tests/dqn_util.py).

    python tools/measure_dqn.py [--blocks 7]                  # on the GPU: profiles/dqn_update.json
    python tools/measure_dqn.py --float64 [--ratios FILE]     # the CPU part of profiles/dqn_float64.json; with a GPU also the bandit's learner

profiles/dqn_update.json: one update at the two shapes of profiles/ddpg_update.json (B = 512, 2v2 and B = 65 536, 1v1), per update:
  independent, vdn           DQNLearner.update() of a captured learner (double Q, Huber delta = 1) on a uniform ring: one graph replay
  independent_prioritised, vdn_prioritised   the same on a PrioritizedReplayBuffer: the weighted draw and the priority update are in the graph
  torch     the same update as a torch composition with autograd: StackedActor, gather, smooth_l1, clip_grad_norm_, torch Adam, foreach
            Polyak, pack() of both networks: eager, on the uniform ring -- the reference of the ratio
  ddpg      DDPGLearner.update() of a captured learner on the same ring (central critic at 2v2, own at 1v1)
Device events around blocks of updates, the ways as ALTERNATING blocks in one process after a warm-up of all (tools/bench_ddpg_update.py's
ring, blocks and statistics); medians, ranges and spreads per way.  The launches per update are counted on one eager call
(tools/bench_td3_update.py's count: every native entry point called, weighed by the launches the header states for it).  No bound is set
here: the figures are what the profile records.

profiles/dqn_float64.json: what tests/test_dqn_cpu.py and test_hip_dqn_learner.py read beside their code:
  stepped   the whole-update cases (dqn_util.STEP_CASES, stepped_case), all on the CPU: per (team, mix, batch) the seed -- the first from 0 at which the
            float64 reference alone qualifies --, every seed tried, the share of rows the kink filter leaves out, its zeroing rounds and
            the smallest arg-max margin.  --ratios: a file of JSON lines the GPU test appended under BSX_DQN_RATIOS_OUT, kept as "kernel"
  bandit    the learning check's configuration and what its torch composition reaches at the candidates 100 .. 400 on the CPU: the
            update count is the smallest after which its greedy action is the paying arm on every probe observation, for both mixes
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

SIZES = ((512, 2, 8, True, 16), (65536, 1, 5, False, 4))            # (B, nA, Do, DDPG's critic central, updates per block)
Q_SCALE, DELTA = 20.0, 1.0


def float64_profile(argv):
    import torch
    import dqn_util as Q
    import offpolicy_util as O
    old = json.load(open(Q.PROFILE)) if os.path.exists(Q.PROFILE) else {}
    cases = {}
    for team, mix, batch in Q.STEP_CASES:
        tried, seed = [], 0
        while True:
            c, share, rounds, low = Q.try_seed(team, mix, seed, batch)
            tried.append([seed, c is not None, round(100 * share, 2), rounds, float("%.3e" % low)])
            if c is not None:
                break
            seed += 1
        assert seed == Q.step_seed(team, mix, batch), (team, mix, batch, seed)
        cases[Q.team_id(team, mix, batch)] = dict(seed=seed, left_out_percent=round(100 * c.share, 2), zeroing_rounds=c.rounds,
                                                  smallest_argmax_margin=float("%.3e" % c.margin), seeds_tried=tried)
    stepped = dict(what="tests/dqn_util.py stepped_case: one whole DQN update (double Q, Huber delta = 1, q_scale = 4) from a target network "
                        "that is not the network, eps = 1e-3, float64 on the CPU; the float32 yardstick is the same in float32",
                   seeds="per (team, mix) the first seed from 0 at which, on the float64 reference alone, the kink filter closes within 4 "
                         "zeroing rounds, leaves out at most a quarter of the rows and no arg-max margin lies below 1e-4",
                   cases=cases, kernel=O.kept_kernel(old, argv))
    b = Q.BANDIT
    rows, probe = Q.bandit_rows()
    runs = {}
    for mix in Q.MIXES:
        for N in (100, 200, 300, 400):
            net, losses = Q.bandit_twin(mix, Q.bandit_draws(N), torch.float32)
            runs[f"{mix}-{N}"] = dict(greedy_is_best_on_every_probe=Q.greedy_is_best(net, probe), first_loss=losses[0], last_loss=losses[-1])
    N = next(n for n in (100, 200, 300, 400) if all(runs[f"{m}-{k}"]["greedy_is_best_on_every_probe"] for m in Q.MIXES for k in (100, 200, 300, 400)
                                                     if k >= n))
    assert N == b["N"], (N, b["N"])
    out = dict(command="python tools/measure_dqn.py --float64 [--ratios FILE]", factors={},
               factors_note="every whole-update comparison pools a row or a step over its ten tensors and holds the project's (2, 4); nothing "
                            "is held to a wider factor",
               stepped=stepped, bandit=dict(b, torch_composition=runs))
    json.dump(out, open(Q.PROFILE, "w"), indent=1)
    print(json.dumps(out, indent=1))


def torch_dqn(torch, buf, qnet, mix):
    """The update as a torch user writes it (eager, autograd) -> (a callable, what it must keep alive)."""
    import bench_ddpg_update as BD
    target = copy.deepcopy(qnet)
    blobs = [qnet.pack(), target.pack()]
    opt = torch.optim.Adam(qnet.parameters(), lr=BD.LR)

    def update():
        buf.sample()
        obs, obs_next, act, rew, done = buf._b_obs, buf._b_obs_, buf._b_act, buf._b_rew, buf._b_done
        with torch.no_grad():
            nxt = target(obs_next).gather(-1, qnet(obs_next).argmax(-1, keepdim=True))[..., 0]
            N, R = (1.0 - done.to(torch.float32)) * Q_SCALE * nxt, rew
            if mix == "vdn":
                N, R = N.sum(1, keepdim=True), R.sum(1, keepdim=True)
            y = R + BD.GAMMA * N
        Q = Q_SCALE * qnet(obs).gather(-1, act.argmax(-1, keepdim=True))[..., 0]
        if mix == "vdn":
            Q = Q.sum(1, keepdim=True)
        opt.zero_grad(set_to_none=True)
        (2.0 * DELTA * torch.nn.functional.smooth_l1_loss(Q, y, reduction="none", beta=DELTA)).mean(0).sum().backward()
        torch.nn.utils.clip_grad_norm_(qnet.parameters(), BD.MGN)
        opt.step()
        with torch.no_grad():
            ts, ns = list(target.parameters()), list(qnet.parameters())
            torch._foreach_mul_(ts, 1.0 - BD.TAU)
            torch._foreach_add_(ts, ns, alpha=BD.TAU)
        qnet.pack(out=blobs[0])
        target.pack(out=blobs[1])
    return update, (blobs, target, opt)


def update_profile(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_dqn.py measures on the GPU: none found (the CPU part is --float64)")
    import bench_ddpg_update as BD
    import bench_td3_update as BT
    from deep_rl_battlespace_amd.learner import DDPGLearner, DQNLearner
    from deep_rl_battlespace_amd.replay import PrioritizedReplayBuffer
    from deep_rl_battlespace_amd.rollout import StackedActor
    BT.LAUNCHES.setdefault("bsx_dqn_head", 2)                         # the head pass and its merge (include/battlespace_hip.h)

    def prio_ring(B, nA, Do, seed):
        src = BD.filled_ring(torch, B, nA, Do, 4, seed)
        buf = PrioritizedReplayBuffer(BD.RING_ROWS, B, list(range(nA)), Do, Do * nA, 4, device="cuda", seed=seed)
        buf._put(src.actor_states.clone(), src.action_mem.clone(), src.rew_mem.clone(), src.actor_new_states.clone(), src.done_mem.clone())
        return buf

    result = dict(command="python tools/measure_dqn.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  ring_rows=BD.RING_ROWS, gamma=BD.GAMMA, tau=BD.TAU, lr=BD.LR, max_grad_norm=BD.MGN, q_scale=Q_SCALE, huber_delta=DELTA, double=True,
                  sizes=[])
    kept = []

    def write():
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    for B, nA, Do, central, reps in SIZES:
        torch.manual_seed(B + nA)
        q0 = StackedActor(nA, Do, 4, device="cuda")
        Dc = nA * (Do + 4) if central else Do + 4
        critic0 = StackedActor(nA, Dc, 1, device="cuda")
        kw = dict(q_scale=Q_SCALE, huber_delta=DELTA, gamma=BD.GAMMA, tau=BD.TAU, lr=BD.LR, max_grad_norm=BD.MGN)
        learners = {}
        for mix in ("independent", "vdn"):
            learners[mix] = DQNLearner(BD.filled_ring(torch, B, nA, Do, 4, 1), copy.deepcopy(q0), mix=mix, **kw).capture()
            learners[mix + "_prioritised"] = DQNLearner(prio_ring(B, nA, Do, 1), copy.deepcopy(q0), mix=mix, **kw).capture()
        learners["ddpg"] = DDPGLearner(BD.filled_ring(torch, B, nA, Do, 4, 1), copy.deepcopy(q0), copy.deepcopy(critic0),
                                       critic_input="central" if central else "own", gamma=BD.GAMMA, tau=BD.TAU, lr_actor=BD.LR, lr_critic=BD.LR,
                                       max_grad_norm=BD.MGN).capture()
        ways = {name: x.update for name, x in learners.items()}
        ways["torch"], keep = torch_dqn(torch, BD.filled_ring(torch, B, nA, Do, 4, 1), copy.deepcopy(q0), "independent")
        x = BD.alternate(torch, ways, reps, args.blocks)
        per = {name: BD.stats(v) for name, v in x.items()}
        ratio = lambda a, b: round(per[a]["median_ms"] / per[b]["median_ms"], 3)          # noqa: E731
        result["sizes"].append(dict(batch=B, agents=nA, obs_len=Do, ddpg_critic_input="central" if central else "own", updates_per_block=reps, **per,
                                    launches_per_update={name: None for name in learners},
                                    torch_over_independent=ratio("torch", "independent"), vdn_over_independent=ratio("vdn", "independent"),
                                    prioritised_over_uniform=ratio("independent_prioritised", "independent"),
                                    ddpg_over_independent=ratio("ddpg", "independent"),
                                    differences_beyond_the_spreads=dict(torch=bool(per["torch"]["min_ms"] > per["independent"]["max_ms"]),
                                                                        ddpg=bool(per["ddpg"]["min_ms"] > per["independent"]["max_ms"]))))
        kept.append((learners, keep))
        write()                                                       # the times first: the launch counts run the updates once more, eagerly
    for entry, (learners, _) in zip(result["sizes"], kept):
        for name, learner in learners.items():
            entry["launches_per_update"][name] = BT.launches(learner._run)
    print(json.dumps(result))
    write()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--float64", action="store_true")
    ap.add_argument("--ratios")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_update.json"))
    args = ap.parse_args()
    float64_profile(sys.argv) if args.float64 else update_profile(args)


if __name__ == "__main__":
    main()
