#!/usr/bin/env python3
"""One SAC update on the device against one TD3 update and against the torch composition of the same SAC, on the same ring rows and
initial weights (learner.SACLearner; csrc/bsx_sac_head.hip).

    python tools/bench_sac_update.py [--blocks 7] [--out profiles/sac_update.json]

  sac     SACLearner.update() of a captured learner (updates = 2: one graph replay is two updates), per update
  td3     TD3Learner.update() of a captured learner on the same ring and shape (updates = 2, policy_delay = 2), per update
  torch   the torch composition of the same SAC with autograd: StackedActor, clip_grad_norm_ and one Adam over both critics with the
          foreach Polyak lines of both targets, clip and one Adam over the actor and log_std, one Adam over log_alpha, pack() of the five
          networks: eager, per update

at the two shapes of profiles/ddpg_update.json (tools/bench_ddpg_update.py, whose ring, blocks and statistics these are) with k = 3.
Device events around blocks of calls, the three ways as ALTERNATING blocks in one process after a warm-up of all; medians, ranges and
spreads per way.  The launches per update of the two learners are counted on one eager call (tools/bench_td3_update.py: launches).  No
bound is set here: the figures are what the profile records."""
import argparse
import copy
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import bench_ddpg_update as BD  # noqa: E402
import bench_td3_update as B3  # noqa: E402

UPDATES, K, ALPHA, LR_ALPHA, TARGET_ENTROPY = 2, 3, 0.2, 3e-4, -3.0
# launches per native call where it is not one (include/battlespace_hip.h states them)
B3.LAUNCHES.update({"bsx_sac_head": 2, "bsx_sac_policy_grad": 2})


def torch_sac(torch, buf, actor, critic, critic2, central):
    B, nA, k = buf.batch_size, buf.n_agents, buf.n_actions
    nets = (actor, critic, critic2)
    targets = tuple(copy.deepcopy(n) for n in nets[1:])
    blobs = [n.pack() for n in nets + targets]
    log_std = torch.full((nA, 3), math.log(0.2), device="cuda", requires_grad=True)
    log_alpha = torch.full((nA,), math.log(ALPHA), device="cuda", requires_grad=True)
    pi_params = list(actor.parameters()) + [log_std]
    both = list(critic.parameters()) + list(critic2.parameters())
    oa, oc, ot = torch.optim.Adam(pi_params, lr=BD.LR), torch.optim.Adam(both, lr=BD.LR), torch.optim.Adam([log_alpha], lr=LR_ALPHA)
    own = torch.eye(nA, device="cuda").view(1, nA, nA, 1)
    const = 1.5 * math.log(2.0 * math.pi)

    def joined(o, a):
        if not central:
            return torch.cat([o, a], -1)
        return torch.cat([o.reshape(B, 1, -1), a.reshape(B, 1, -1)], -1).expand(B, nA, -1)

    def draw(mu):
        z = torch.randn_like(mu)
        return mu + torch.exp(log_std) * z, (-0.5 * z * z - log_std).sum(-1) - const

    def update():
        buf.sample()
        obs, obs_next, act, rew, done = buf._b_obs, buf._b_obs_, buf._b_act, buf._b_rew, buf._b_done
        with torch.no_grad():
            alpha = torch.exp(log_alpha)
            a, lp = draw(actor(obs_next))
            x_next = joined(obs_next, a)
            v = torch.minimum(targets[0](x_next, squash=False)[..., 0], targets[1](x_next, squash=False)[..., 0]) - alpha * lp
            y = rew + BD.GAMMA * (1.0 - done.to(torch.float32)) * v
        x_cur = joined(obs, act)
        oc.zero_grad(set_to_none=True)
        (((critic(x_cur, squash=False)[..., 0] - y) ** 2).mean(0).sum() + ((critic2(x_cur, squash=False)[..., 0] - y) ** 2).mean(0).sum()).backward()
        torch.nn.utils.clip_grad_norm_(both, BD.MGN)
        oc.step()
        with torch.no_grad():
            for t, n in zip(targets, nets[1:]):
                ts, ns = list(t.parameters()), list(n.parameters())
                torch._foreach_mul_(ts, 1.0 - BD.TAU)
                torch._foreach_add_(ts, ns, alpha=BD.TAU)
        pi, logp = draw(actor(obs))
        if central:
            actions = own * pi.unsqueeze(1) + (1.0 - own) * act.unsqueeze(1)
            x_pi = torch.cat([obs.reshape(B, 1, -1).expand(B, nA, -1), actions.reshape(B, nA, nA * k)], -1)
        else:
            x_pi = torch.cat([obs, pi], -1)
        oa.zero_grad(set_to_none=True)
        (alpha * logp - torch.minimum(critic(x_pi, squash=False)[..., 0], critic2(x_pi, squash=False)[..., 0])).mean(0).sum().backward()
        torch.nn.utils.clip_grad_norm_(pi_params, BD.MGN)
        oa.step()
        ot.zero_grad(set_to_none=True)
        (-(log_alpha * (logp.detach() + TARGET_ENTROPY).mean(0)).sum()).backward()
        ot.step()
        for n, b in zip(nets + targets, blobs):
            n.pack(out=b)

    def two():
        for _ in range(UPDATES):
            update()
    return two, (blobs, targets, oa, oc, ot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_update.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sac_update.py measures on the GPU: none found")
    from deep_rl_battlespace_amd.learner import SACLearner, TD3Learner
    from deep_rl_battlespace_amd.rollout import StackedActor
    result = dict(command="python tools/bench_sac_update.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  ring_rows=BD.RING_ROWS, gamma=BD.GAMMA, tau=BD.TAU, lr=BD.LR, lr_alpha=LR_ALPHA, alpha=ALPHA, target_entropy=TARGET_ENTROPY,
                  max_grad_norm=BD.MGN, updates_per_call=UPDATES, unit="ms per update: a call is two updates", sizes=[])
    learners = []
    for B, nA, Do, _, central, reps in BD.SIZES:
        k = K
        Dc = nA * (Do + k) if central else Do + k
        torch.manual_seed(B + nA)
        actor0, critic0, critic20 = StackedActor(nA, Do, k, device="cuda"), StackedActor(nA, Dc, 1, device="cuda"), StackedActor(nA, Dc, 1, device="cuda")
        kw = dict(critic_input="central" if central else "own", gamma=BD.GAMMA, tau=BD.TAU, lr_actor=BD.LR, lr_critic=BD.LR, max_grad_norm=BD.MGN,
                  updates=UPDATES)
        ring = lambda: BD.filled_ring(torch, B, nA, Do, k, 1)             # noqa: E731
        nets = lambda: (copy.deepcopy(actor0), copy.deepcopy(critic0), copy.deepcopy(critic20))     # noqa: E731
        sac = SACLearner(ring(), *nets(), alpha=ALPHA, lr_alpha=LR_ALPHA, target_entropy=TARGET_ENTROPY, **kw).capture()
        td3 = TD3Learner(ring(), *nets(), policy_delay=2, **kw).capture()
        eager, keep = torch_sac(torch, ring(), *nets(), central)
        ways = dict(sac=sac.update, td3=td3.update, torch=eager)
        calls = max(1, reps // UPDATES)
        x = BD.alternate(torch, ways, calls, args.blocks)
        per = {name: BD.stats([ms / UPDATES for ms in v]) for name, v in x.items()}
        entry = dict(batch=B, agents=nA, obs_len=Do, actions=k, critic_input=kw["critic_input"], critic_inputs=Dc, calls_per_block=calls, **per,
                     launches_per_update=dict(sac=None, td3=None, torch=None),
                     sac_over_td3=round(per["sac"]["median_ms"] / per["td3"]["median_ms"], 3),
                     torch_over_sac=round(per["torch"]["median_ms"] / per["sac"]["median_ms"], 3),
                     differences_beyond_the_spreads=dict(td3=bool(per["sac"]["min_ms"] > per["td3"]["max_ms"]),
                                                         torch=bool(per["torch"]["min_ms"] > per["sac"]["max_ms"])))
        result["sizes"].append(entry)
        learners.append((sac, td3))
        del ways, keep, eager
        torch.cuda.empty_cache()

    def write():
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    write()                                                           # the times first: the launch counts below run the updates once more, eagerly
    for entry, (sac, td3) in zip(result["sizes"], learners):
        for name, learner in (("sac", sac), ("td3", td3)):
            n = B3.launches(learner._run)
            entry["launches_per_update"][name] = None if n is None else n / UPDATES
    print(json.dumps(result))
    write()


if __name__ == "__main__":
    main()
