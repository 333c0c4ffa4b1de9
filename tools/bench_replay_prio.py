#!/usr/bin/env python3
"""What prioritised replay costs on the device (replay.PrioritizedReplayBuffer; csrc/bsx_replay_prio.hip), at the two shapes of
profiles/ddpg_update.json on a FILLED ring of 2^20 rows.

    python tools/bench_replay_prio.py [--blocks 7] [--out profiles/replay_prio.json]

  a  update     a captured DDPGLearner.update() on the prioritised ring against the same learner on a plain DeviceReplayBuffer -- with
                a plain ring every launch of an update is what it was before the prioritised ring existed, so that is the earlier update
  b  sample     PrioritizedReplayBuffer.sample() against DeviceReplayBuffer.sample() (bsx_replay_sample)
  c  priorities update_priorities alone
  d  append     bsx_replay_prio_append alone after an append of 32 x 4096 rows (and the ring's own three launches, for scale)
  e  torch      the torch composition of the same draw and update: cumsum over the whole ring (the rebuild), searchsorted, the five
                gathers, pow for the weights, abs / max / clamp / pow for the new priorities, index_put_

Every way is captured as a graph of `calls` calls (device time, not the host's launch cost) and timed with device events around blocks of
replays, the ways of a group as ALTERNATING blocks in one process after a warm-up of all; medians, ranges, spreads.  The one bar:
b + c below e at both shapes -- otherwise the tree has no reason to exist.  a is reported as it comes out."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_ddpg_update as BD  # noqa: E402

M = 1 << 20
APPEND_ROWS = 32 * 4096
SIZES = ((512, 2, 8, 4, True, 16), (65536, 1, 5, 4, False, 4))      # (B, nA, Do, k, central, calls per graph): bench_ddpg_update's


def ring(torch, cls, B, nA, Do, k, seed, **kw):
    """A ring of M rows, filled; a prioritised one with priorities spread over six octaves (what TD errors of 0.01 .. 30 leave)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    uni = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1       # noqa: E731
    buf = cls(M, B, list(range(nA)), Do, Do * nA, k, device="cuda", seed=seed, **kw)
    buf._put(uni(M, nA, Do), uni(M, nA, k), torch.randn((M, nA), generator=g, device="cuda"), uni(M, nA, Do),
             torch.rand((M, nA), generator=g, device="cuda") < 0.05)
    if hasattr(buf, "priorities"):
        buf.priorities.copy_((65536.0 * torch.exp2(torch.rand(M, generator=g, device="cuda") * 6.0 - 3.0)).to(torch.int32))
        buf.rebuild_tree()
    return buf


def graphed(torch, step, calls):
    """step() x calls as one graph -> its replay (one warm-up call first)."""
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            step()
    return graph


def torch_composition(torch, buf, q, y, alpha=0.6, beta=0.4, eps=1e-6, dmax=32.0):
    """Proportional prioritised replay the obvious way in torch, on the same ring: float32 priorities [M]."""
    B, nA = buf.batch_size, buf.n_agents
    p = 2.0 ** (torch.rand(M, device="cuda") * 6.0 - 3.0)
    w = torch.zeros((B, nA), device="cuda")

    def step():
        c = torch.cumsum(p, 0)                                              # the full rebuild: M words per draw
        idx = torch.searchsorted(c, torch.rand(B, device="cuda") * c[-1]).clamp_(max=M - 1)
        batch = [getattr(buf, f)[idx] for f in ("actor_states", "actor_new_states", "action_mem", "rew_mem", "done_mem")]
        pb = p[idx]
        w.copy_(((pb.min() / pb) ** beta).unsqueeze(1).expand(B, nA))
        new = ((q - y).abs().max(1).values.clamp(max=dmax) + eps) ** alpha
        p.index_put_((idx,), new)
        return batch
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_prio.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay_prio.py measures on the GPU: none found")
    from deep_rl_battlespace_amd.learner import DDPGLearner
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, PrioritizedReplayBuffer, prio_levels
    from deep_rl_battlespace_amd.rollout import StackedActor
    result = dict(command=f"python tools/bench_replay_prio.py --blocks {args.blocks}", device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  ring_rows=M, levels=prio_levels(M), append_rows=APPEND_ROWS,
                  launches=dict(sample=2, uniform_sample=1, update_priorities=5, append_extra=4, added_per_update=6), sizes=[])
    for B, nA, Do, k, central, calls in SIZES:
        Dc = nA * (Do + k) if central else Do + k
        torch.manual_seed(B + nA)
        actor0, critic0 = StackedActor(nA, Do, k, device="cuda"), StackedActor(nA, Dc, 1, device="cuda")
        kw = dict(critic_input="central" if central else "own", gamma=BD.GAMMA, tau=BD.TAU, lr_actor=BD.LR, lr_critic=BD.LR, max_grad_norm=BD.MGN)
        prio, plain = ring(torch, PrioritizedReplayBuffer, B, nA, Do, k, 1), ring(torch, DeviceReplayBuffer, B, nA, Do, k, 1)
        learners = [DDPGLearner(b, copy.deepcopy(actor0), copy.deepcopy(critic0), updates=calls, **kw).capture() for b in (prio, plain)]
        a = BD.alternate(torch, dict(prioritised=learners[0].update, uniform=learners[1].update), 4, args.blocks)
        # b .. e on rings of their own: the learners' graphs hold theirs
        prio2, plain2, ring_e = (ring(torch, c, B, nA, Do, k, 2) for c in (PrioritizedReplayBuffer, DeviceReplayBuffer, DeviceReplayBuffer))
        q, y = torch.randn((B, nA), device="cuda"), torch.randn((B, nA), device="cuda")
        prio2.sample()
        graphs = dict(sample=graphed(torch, prio2.sample, calls), uniform_sample=graphed(torch, plain2.sample, calls),
                      update_priorities=graphed(torch, lambda: prio2.update_priorities(q, y), calls),
                      torch=graphed(torch, torch_composition(torch, ring_e, q, y), calls))
        bcde = BD.alternate(torch, {name: g.replay for name, g in graphs.items()}, 4, args.blocks)
        rnd = lambda *s: torch.randn(s, device="cuda")                                 # noqa: E731
        src = [rnd(APPEND_ROWS, nA, Do), rnd(APPEND_ROWS, nA, k), rnd(APPEND_ROWS, nA), rnd(APPEND_ROWS, nA, Do), rnd(APPEND_ROWS, nA) > 1.5]
        prio2._put(*src)
        extra = lambda: prio2._prio("bsx_replay_prio_append", prio2._counter.data_ptr(), prio2._stored.data_ptr(), APPEND_ROWS)      # noqa: E731
        d = BD.alternate(torch, dict(append_extra=graphed(torch, extra, calls).replay,
                                     ring_append=graphed(torch, lambda: plain2._put(*src), calls).replay), 4, args.blocks)
        torch.cuda.synchronize()
        per = {name: BD.stats([v / calls for v in x]) for name, x in {**a, **bcde, **d}.items()}
        b_c = per["sample"]["median_ms"] + per["update_priorities"]["median_ms"]
        entry = dict(batch=B, agents=nA, obs_len=Do, actions=k, critic_input=kw["critic_input"], calls_per_graph=calls, per_call=per,
                     update_prioritised_over_uniform=round(per["prioritised"]["median_ms"] / per["uniform"]["median_ms"], 3),
                     sample_plus_priorities_ms=round(b_c, 5), torch_ms=per["torch"]["median_ms"],
                     torch_over_sample_plus_priorities=round(per["torch"]["median_ms"] / b_c, 2),
                     tree_beats_torch=bool(per["sample"]["max_ms"] + per["update_priorities"]["max_ms"] < per["torch"]["min_ms"]))
        result["sizes"].append(entry)
        del learners, graphs, prio, plain, prio2, plain2, ring_e
        torch.cuda.empty_cache()
    print(json.dumps(result))
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    if not all(s["tree_beats_torch"] for s in result["sizes"]):
        raise SystemExit("sample + update_priorities is not below the torch composition at every shape")


if __name__ == "__main__":
    main()
