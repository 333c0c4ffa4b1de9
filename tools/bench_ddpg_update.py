#!/usr/bin/env python3
"""One MADDPG update on the device, three ways on the same ring rows and initial weights (learner.DDPGLearner; csrc/bsx_ddpg_head.hip).

    python tools/bench_ddpg_update.py [--blocks 7] [--out profiles/ddpg_update.json]

  learner   DDPGLearner.update() of a captured learner: one graph replay, the ring's draw included
  hand      the composition the fused MLP calls allowed before: bsx_mlp_forward / mlp_grad / mlp_adam_step with torch glue on preallocated
            tensors (cat-style slice copies, the TD target with `done`, both grad_out tensors from element-wise ops, mlp_grad's padded
            copy), as tests/test_hip_adam_mlp.py writes it, extended to a central critic; captured as one graph too
  torch     StackedActor under autograd, clip_grad_norm_, torch Adam, foreach Polyak, pack() of all four networks: eager (its autograd
            graph is rebuilt per update, as a torch user runs it)

at the reference's size (B = 512, 2v2, central critic 24 -> 64 -> 64 -> 1) and at a large batch (B = 65 536, 1v1, own critics).  Device
events around blocks of updates, the three ways as ALTERNATING blocks in one process after a warm-up of all; medians, ranges and
spreads per way, and the two ratios to the learner.  No bound is set here: the ratios are what the profile records."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((512, 2, 8, 4, True, 16), (65536, 1, 5, 4, False, 4))      # (B, nA, Do, k, central, updates per block)
RING_ROWS = 1 << 17
GAMMA, TAU, LR, MGN = 0.95, 0.01, 1e-3, 0.5


def stats(x):
    m = statistics.median(x)
    return dict(median_ms=round(m, 5), min_ms=round(min(x), 5), max_ms=round(max(x), 5), spread=round((max(x) - min(x)) / m, 4))


def block(torch, step, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(torch, steps, reps, blocks):
    for _ in range(2):
        for step in steps.values():
            step()
    torch.cuda.synchronize()
    out = {k: [] for k in steps}
    for _ in range(blocks):
        for k, step in steps.items():
            out[k].append(block(torch, step, reps))
    return out


def filled_ring(torch, B, nA, Do, k, seed):
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    g = torch.Generator(device="cuda").manual_seed(seed)
    uni = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1       # noqa: E731
    buf = DeviceReplayBuffer(RING_ROWS, B, list(range(nA)), Do, Do * nA, k, device="cuda", seed=seed)
    buf._put(uni(RING_ROWS, nA, Do), uni(RING_ROWS, nA, k), torch.randn((RING_ROWS, nA), generator=g, device="cuda"), uni(RING_ROWS, nA, Do),
             torch.rand((RING_ROWS, nA), generator=g, device="cuda") < 0.05)
    return buf


def hand_update(torch, buf, actor, critic, central):
    """The composition of the existing calls with torch glue -> a callable (captured as one graph)."""
    from deep_rl_battlespace_amd import _lib, learner as L
    lib = _lib.load()
    B, nA, Do, k = buf.batch_size, buf.n_agents, buf.actor_states.shape[2], buf.n_actions
    W, Dc = (nA * Do, nA * (Do + k)) if central else (Do, Do + k)
    t_actor, t_critic = copy.deepcopy(actor), copy.deepcopy(critic)
    for t in (t_actor, t_critic):
        t.__dict__.pop("_bsx_mlp_buffers", None)
    blobs = [n.pack() for n in (actor, critic, t_actor, t_critic)]
    st_a, st_c = L.AdamState(actor), L.AdamState(critic)
    hp = L.adam_hyper(LR, max_grad_norm=MGN, tau=TAU)
    step_a, step_c = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    sa, sc = (torch.zeros(4, dtype=torch.float64, device="cuda") for _ in range(2))
    ws = torch.empty(L.mlp_adam_step_workspace_bytes(nA, 1) // 8 + 1, dtype=torch.int64, device="cuda")
    f = lambda *s: torch.zeros(s, device="cuda")                                 # noqa: E731
    x_cur, x_next, x_pi, y4, yq = f(B, nA, Dc), f(B, nA, Dc), f(B, nA, Dc), f(B, nA, 4), f(B, nA, 4)
    q, q_next, td, notdone = f(B, nA), f(B, nA), f(B, nA), f(B, nA)
    go_q, minus, dqda = f(B, nA, 1), torch.full((B, nA, 1), -1.0 / B, device="cuda"), f(B, nA, k)
    stream = lambda: torch.cuda.current_stream().cuda_stream                     # noqa: E731

    def forward(blob, x, y, raw=None):
        _lib.check(lib.bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y.data_ptr(), raw.data_ptr() if raw is not None else None, B, nA, x.shape[2],
                                       stream()), "bsx_mlp_forward")

    def join_obs(x, o):
        x[..., :W].copy_(o.reshape(B, 1, W) if central else o)

    def join_act(x, a):                                                          # every slot (central) or the own columns
        x[..., W:].copy_(a[..., :k].reshape(B, 1, nA * k) if central else a[..., :k])

    def update():
        buf.sample()
        obs, obs_next, act, rew, done = buf._b_obs, buf._b_obs_, buf._b_act, buf._b_rew, buf._b_done
        join_obs(x_cur, obs); join_act(x_cur, act)
        join_obs(x_next, obs_next); join_obs(x_pi, obs); join_act(x_pi, act)
        forward(blobs[2], obs_next, y4)
        join_act(x_next, y4)
        forward(blobs[3], x_next, yq, q_next)
        notdone.copy_(done)
        notdone.neg_().add_(1.0)
        q_next.mul_(notdone)
        torch.add(rew, q_next, alpha=GAMMA, out=td)
        forward(blobs[1], x_cur, yq, q)
        torch.sub(q, td, out=go_q[..., 0])
        go_q.mul_(2.0 / B)
        row_c, _ = L.mlp_grad(critic, blobs[1], x_cur, go_q, squash=False, input_grad=False)
        L.mlp_adam_step([critic], [row_c], [st_c], [blobs[1]], hp, step_c, targets=[t_critic], target_blobs=[blobs[3]], stats=sc, workspace=ws)
        forward(blobs[0], obs, y4)
        if central:
            for i in range(nA):
                x_pi[:, i, W + i * k:W + (i + 1) * k].copy_(y4[:, i, :k])
        else:
            join_act(x_pi, y4)
        _, gx = L.mlp_grad(critic, blobs[1], x_pi, minus, squash=False, input_grad=True)
        if central:
            for i in range(nA):
                dqda[:, i].copy_(gx[:, i, W + i * k:W + (i + 1) * k])
        else:
            dqda.copy_(gx[..., W:])
        row_a, _ = L.mlp_grad(actor, blobs[0], obs, dqda, squash=True, input_grad=False)
        L.mlp_adam_step([actor], [row_a], [st_a], [blobs[0]], hp, step_a, targets=[t_actor], target_blobs=[blobs[2]], stats=sa, workspace=ws)
    update()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update()
    keep = (graph, blobs, t_actor, t_critic, st_a, st_c)
    return graph.replay, keep


def torch_update(torch, buf, actor, critic, central):
    B, nA, k = buf.batch_size, buf.n_agents, buf.n_actions
    t_actor, t_critic = copy.deepcopy(actor), copy.deepcopy(critic)
    nets = (actor, critic, t_actor, t_critic)
    blobs = [n.pack() for n in nets]
    oa, oc = torch.optim.Adam(actor.parameters(), lr=LR), torch.optim.Adam(critic.parameters(), lr=LR)
    own = torch.eye(nA, device="cuda").view(1, nA, nA, 1)

    def joined(o, a):
        if not central:
            return torch.cat([o, a], -1)
        return torch.cat([o.reshape(B, 1, -1), a.reshape(B, 1, -1)], -1).expand(B, nA, -1)

    def update():
        buf.sample()
        obs, obs_next, act, rew, done = buf._b_obs, buf._b_obs_, buf._b_act, buf._b_rew, buf._b_done
        with torch.no_grad():
            y = rew + GAMMA * (1.0 - done.to(torch.float32)) * t_critic(joined(obs_next, t_actor(obs_next)), squash=False)[..., 0]
        oc.zero_grad(set_to_none=True)
        ((critic(joined(obs, act), squash=False)[..., 0] - y) ** 2).mean(0).sum().backward()
        torch.nn.utils.clip_grad_norm_(critic.parameters(), MGN)
        oc.step()
        pi = actor(obs)
        if central:
            actions = own * pi.unsqueeze(1) + (1.0 - own) * act.unsqueeze(1)
            x_pi = torch.cat([obs.reshape(B, 1, -1).expand(B, nA, -1), actions.reshape(B, nA, nA * k)], -1)
        else:
            x_pi = torch.cat([obs, pi], -1)
        oa.zero_grad(set_to_none=True)
        (-critic(x_pi, squash=False)[..., 0].mean(0).sum()).backward()
        torch.nn.utils.clip_grad_norm_(actor.parameters(), MGN)
        oa.step()
        with torch.no_grad():
            for t, n in ((t_actor, actor), (t_critic, critic)):
                ts, ns = list(t.parameters()), list(n.parameters())
                torch._foreach_mul_(ts, 1.0 - TAU)
                torch._foreach_add_(ts, ns, alpha=TAU)
        for n, b in zip(nets, blobs):
            n.pack(out=b)
    return update, (blobs, t_actor, t_critic, oa, oc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg_update.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddpg_update.py measures on the GPU: none found")
    from deep_rl_battlespace_amd.learner import DDPGLearner
    from deep_rl_battlespace_amd.rollout import StackedActor
    result = dict(command="python tools/bench_ddpg_update.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  ring_rows=RING_ROWS, gamma=GAMMA, tau=TAU, lr=LR, max_grad_norm=MGN, sizes=[])
    for B, nA, Do, k, central, reps in SIZES:
        Dc = nA * (Do + k) if central else Do + k
        torch.manual_seed(B + nA)
        actor0, critic0 = StackedActor(nA, Do, k, device="cuda"), StackedActor(nA, Dc, 1, device="cuda")
        ways, keep = {}, []
        learner = DDPGLearner(filled_ring(torch, B, nA, Do, k, 1), copy.deepcopy(actor0), copy.deepcopy(critic0),
                              critic_input="central" if central else "own", gamma=GAMMA, tau=TAU, lr_actor=LR, lr_critic=LR, max_grad_norm=MGN).capture()
        ways["learner"] = learner.update
        ways["hand"], k1 = hand_update(torch, filled_ring(torch, B, nA, Do, k, 1), copy.deepcopy(actor0), copy.deepcopy(critic0), central)
        ways["torch"], k2 = torch_update(torch, filled_ring(torch, B, nA, Do, k, 1), copy.deepcopy(actor0), copy.deepcopy(critic0), central)
        keep += [learner, k1, k2]
        x = alternate(torch, ways, reps, args.blocks)
        per = {name: stats(v) for name, v in x.items()}
        entry = dict(batch=B, agents=nA, obs_len=Do, actions=k, critic_input="central" if central else "own", critic_inputs=Dc,
                     updates_per_block=reps, **per,
                     torch_over_learner=round(per["torch"]["median_ms"] / per["learner"]["median_ms"], 3),
                     hand_over_learner=round(per["hand"]["median_ms"] / per["learner"]["median_ms"], 3),
                     differences_beyond_the_spreads=dict(torch=bool(per["torch"]["min_ms"] > per["learner"]["max_ms"]),
                                                         hand=bool(per["hand"]["min_ms"] > per["learner"]["max_ms"])))
        result["sizes"].append(entry)
        del ways, keep, learner, k1, k2
        torch.cuda.empty_cache()
    print(json.dumps(result))
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
