#!/usr/bin/env python3
"""One TD3 update on the device against one DDPG update and against the torch composition of TD3, on the same ring rows and initial
weights (learner.TD3Learner; csrc/bsx_td3_head.hip).

    python tools/bench_td3_update.py [--blocks 7] [--out profiles/td3_update.json]

  td3     TD3Learner.update() of a captured learner (updates = 2, policy_delay = 2: one graph replay is two updates, one of them with
          the actor's half), per update
  ddpg    DDPGLearner.update() of a captured learner on the same ring and shape (updates = 2), per update
  torch   the torch composition of TD3 with autograd: StackedActor, clip_grad_norm_ over both critics, one Adam over both, the actor's
          step and the foreach Polyak lines every second update, pack() of the six networks: eager, per update

at the two shapes of profiles/ddpg_update.json (tools/bench_ddpg_update.py, whose ring, blocks and statistics these are).  Device events
around blocks of calls, the three ways as ALTERNATING blocks in one process after a warm-up of all; medians, ranges and spreads per
way.  The launches per update of the two learners are counted on one eager call: every native entry point called, weighed by the launches
the header states for it (the two counter increments of an update are torch's and not in it).  No bound is set here: the figures are what the profile records."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import bench_ddpg_update as BD  # noqa: E402

UPDATES, DELAY, SIGMA, CLIP = 2, 2, 0.2, 0.5


# launches per native call where it is not one (include/battlespace_hip.h states them): the head pass and its merge, the norm and the step
LAUNCHES = {"bsx_td_head": 2, "bsx_td3_head": 2, "bsx_adam_step_mlp": 2}


def launches(run):
    """Kernel launches of one eager run(): every call of a native entry point counted at the library object and weighed by LAUNCHES
    (torch's own launches -- the two counter increments of an update -- are not in it); None if the count could not be taken."""
    from deep_rl_battlespace_amd import _lib
    lib, seen, real = _lib.load(), {}, {}
    try:
        for name in _lib.SIGNATURES:
            real[name] = getattr(lib, name)

            def counted(*a, _f=real[name], _n=name):
                seen[_n] = seen.get(_n, 0) + 1
                return _f(*a)
            setattr(lib, name, counted)
        run()
        return sum(n * LAUNCHES.get(k, 1) for k, n in seen.items() if not k.endswith("_bytes"))
    except Exception:                                                 # noqa: BLE001  (the count stays open; the times are written already)
        return None
    finally:
        for name, f in real.items():
            setattr(lib, name, f)


def torch_td3(torch, buf, actor, critic, critic2, central):
    B, nA, k = buf.batch_size, buf.n_agents, buf.n_actions
    nets = (actor, critic, critic2)
    targets = tuple(copy.deepcopy(n) for n in nets)
    blobs = [n.pack() for n in nets + targets]
    oa = torch.optim.Adam(actor.parameters(), lr=BD.LR)
    both = list(critic.parameters()) + list(critic2.parameters())
    oc = torch.optim.Adam(both, lr=BD.LR)
    own = torch.eye(nA, device="cuda").view(1, nA, nA, 1)
    count = [0]

    def joined(o, a):
        if not central:
            return torch.cat([o, a], -1)
        return torch.cat([o.reshape(B, 1, -1), a.reshape(B, 1, -1)], -1).expand(B, nA, -1)

    def update():
        buf.sample()
        obs, obs_next, act, rew, done = buf._b_obs, buf._b_obs_, buf._b_act, buf._b_rew, buf._b_done
        with torch.no_grad():
            a = targets[0](obs_next)
            a = torch.clamp(a + torch.clamp(SIGMA * torch.randn_like(a), -CLIP, CLIP), -1.0, 1.0)
            x_next = joined(obs_next, a)
            y = rew + BD.GAMMA * (1.0 - done.to(torch.float32)) * torch.minimum(targets[1](x_next, squash=False)[..., 0],
                                                                               targets[2](x_next, squash=False)[..., 0])
        x_cur = joined(obs, act)
        oc.zero_grad(set_to_none=True)
        (((critic(x_cur, squash=False)[..., 0] - y) ** 2).mean(0).sum() + ((critic2(x_cur, squash=False)[..., 0] - y) ** 2).mean(0).sum()).backward()
        torch.nn.utils.clip_grad_norm_(both, BD.MGN)
        oc.step()
        count[0] += 1
        if count[0] % DELAY == 0:
            pi = actor(obs)
            if central:
                actions = own * pi.unsqueeze(1) + (1.0 - own) * act.unsqueeze(1)
                x_pi = torch.cat([obs.reshape(B, 1, -1).expand(B, nA, -1), actions.reshape(B, nA, nA * k)], -1)
            else:
                x_pi = torch.cat([obs, pi], -1)
            oa.zero_grad(set_to_none=True)
            (-critic(x_pi, squash=False)[..., 0].mean(0).sum()).backward()
            torch.nn.utils.clip_grad_norm_(actor.parameters(), BD.MGN)
            oa.step()
            with torch.no_grad():
                for t, n in zip(targets, nets):
                    ts, ns = list(t.parameters()), list(n.parameters())
                    torch._foreach_mul_(ts, 1.0 - BD.TAU)
                    torch._foreach_add_(ts, ns, alpha=BD.TAU)
        for n, b in zip(nets + targets, blobs):
            n.pack(out=b)

    def two():
        for _ in range(UPDATES):
            update()
    return two, (blobs, targets, oa, oc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td3_update.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_td3_update.py measures on the GPU: none found")
    from deep_rl_battlespace_amd.learner import DDPGLearner, TD3Learner
    from deep_rl_battlespace_amd.rollout import StackedActor
    result = dict(command="python tools/bench_td3_update.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  ring_rows=BD.RING_ROWS, gamma=BD.GAMMA, tau=BD.TAU, lr=BD.LR, max_grad_norm=BD.MGN, updates_per_call=UPDATES, policy_delay=DELAY,
                  target_noise=SIGMA, noise_clip=CLIP, unit="ms per update: a call is two updates, one of them with the actor's half", sizes=[])
    learners = []
    for B, nA, Do, k, central, reps in BD.SIZES:
        Dc = nA * (Do + k) if central else Do + k
        torch.manual_seed(B + nA)
        actor0, critic0, critic20 = StackedActor(nA, Do, k, device="cuda"), StackedActor(nA, Dc, 1, device="cuda"), StackedActor(nA, Dc, 1, device="cuda")
        kw = dict(critic_input="central" if central else "own", gamma=BD.GAMMA, tau=BD.TAU, lr_actor=BD.LR, lr_critic=BD.LR, max_grad_norm=BD.MGN,
                  updates=UPDATES)
        ring = lambda: BD.filled_ring(torch, B, nA, Do, k, 1)             # noqa: E731
        td3 = TD3Learner(ring(), copy.deepcopy(actor0), copy.deepcopy(critic0), copy.deepcopy(critic20), policy_delay=DELAY, target_noise=SIGMA,
                         noise_clip=CLIP, **kw).capture()
        ddpg = DDPGLearner(ring(), copy.deepcopy(actor0), copy.deepcopy(critic0), **kw).capture()
        eager, keep = torch_td3(torch, ring(), copy.deepcopy(actor0), copy.deepcopy(critic0), copy.deepcopy(critic20), central)
        ways = dict(td3=td3.update, ddpg=ddpg.update, torch=eager)
        calls = max(1, reps // UPDATES)
        x = BD.alternate(torch, ways, calls, args.blocks)
        per = {name: BD.stats([ms / UPDATES for ms in v]) for name, v in x.items()}
        entry = dict(batch=B, agents=nA, obs_len=Do, actions=k, critic_input=kw["critic_input"], critic_inputs=Dc, calls_per_block=calls, **per,
                     launches_per_update=dict(td3=None, ddpg=None, torch=None),
                     td3_over_ddpg=round(per["td3"]["median_ms"] / per["ddpg"]["median_ms"], 3),
                     torch_over_td3=round(per["torch"]["median_ms"] / per["td3"]["median_ms"], 3),
                     differences_beyond_the_spreads=dict(ddpg=bool(per["td3"]["min_ms"] > per["ddpg"]["max_ms"]),
                                                         torch=bool(per["torch"]["min_ms"] > per["td3"]["max_ms"])))
        result["sizes"].append(entry)
        learners.append((td3, ddpg))
        del ways, keep, eager
        torch.cuda.empty_cache()

    def write():
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    write()                                                           # the times first: the launch counts below run the updates once more, eagerly
    for entry, (td3, ddpg) in zip(result["sizes"], learners):
        for name, learner in (("td3", td3), ("ddpg", ddpg)):
            n = launches(learner._run)
            entry["launches_per_update"][name] = None if n is None else n / UPDATES
    print(json.dumps(result))
    write()


if __name__ == "__main__":
    main()
