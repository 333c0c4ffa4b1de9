#!/usr/bin/env python3
"""What n-step returns cost in front of the device ring (replay.NStepAppender; csrc/bsx_replay_nstep.hip): one append_rollout at n = 3
against the plain DeviceReplayBuffer.append_rollout (three launches that nothing here changes) on the SAME rollout record, at
65 536 x 1v1 x T = 32 and 4 096 x 2v2 x T = 32.

    python tools/bench_nstep.py [--blocks 9] [--out profiles/nstep_append.json]

The record is a real PolicyRollout's (scripted blue, games ending and re-spawning inside it), run a few times and then left alone.  Each
way stores into a ring of its own with as many rows as one call offers (every kept row is written, none is merely counted; the ring
wraps as the replays go on, which costs nothing).  Each is
captured as a graph of `calls` calls (device time, not the host's launch cost) and timed with device events around blocks of replays, the
ways as ALTERNATING blocks in one process after a warm-up of all; medians, ranges, spreads.  `fold_carry` is the appender's two launches
alone (the fold into the staging buffers, the carry), `nstep` the whole call.  The staging roughly doubles the bytes moved, so about twice
the plain append is what the design predicts; the ratio is recorded, not held to a bar."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_ddpg_update as BD  # noqa: E402

N_STEP, GAMMA, T = 3, 0.95, 32
SIZES = ((65536, 1, 4), (4096, 2, 16))                       # (games, planes per team, calls per graph)
REPS = 4


def graphed(torch, step, calls):
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            step()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_append.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_nstep.py measures on the GPU: none found")
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import _lib, instinct
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, NStepAppender
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    result = dict(command=f"python tools/bench_nstep.py --blocks {args.blocks}", device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  reps_per_block=REPS, n_step=N_STEP, gamma=GAMMA, T=T, launches=dict(plain=3, nstep=5, fold_carry=2), sizes=[])
    for E, n, calls in SIZES:
        env = bsx.parallel_env(n_agents=n, n_envs=E, seed=5, auto_reset=True, device="cuda")
        env.reset()
        torch.manual_seed(5)
        actor = StackedActor(2 * n, 3 * n + 2, 4, device="cuda")
        with torch.no_grad():
            actor.w3.mul_(100.0)                                                # decisive play: games end inside the rollouts
        ro = PolicyRollout(env, actor, T, noise_std=0.2, one_launch=True, opponent=instinct.Team(env.possible_blue, env.possible_red, env))
        ro.start()
        for _ in range(6):
            ro.run()
        torch.cuda.synchronize()
        D, rows = env.obs_size, T * E
        rings = [DeviceReplayBuffer(rows, 512, env.possible_red, D, D * n, 4, device="cuda", seed=0) for _ in range(2)]
        app = NStepAppender(rings[1], N_STEP, GAMMA, T, E)
        lone = NStepAppender(DeviceReplayBuffer(8, 4, env.possible_red, D, D * n, 4, device="cuda"), N_STEP, GAMMA, T, E)

        def fold_carry():                                                        # the two launches of `lone`, on the same record
            src = _lib.BsxReplaySource(ro.obs.data_ptr(), 2 * n * D, D, None, 0, 0, ro.scores.data_ptr(), 2 * n * 4, 4, ro.rew.data_ptr(), 2 * n, 1,
                                       ro._done.data_ptr(), 2 * n, 1, ro.env_done.data_ptr(), 1)
            lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
            _lib.check(lib.bsx_replay_nstep_fold(ctypes.byref(src), ctypes.byref(lone._carry), T, E, n, D, 4, N_STEP, GAMMA,
                                                 lone._staging.data_ptr(), ctypes.byref(lone._folded), s), "bsx_replay_nstep_fold")
            _lib.check(lib.bsx_replay_nstep_carry(ctypes.byref(src), ctypes.byref(lone._carry), T, E, n, D, 4, N_STEP, s), "bsx_replay_nstep_carry")

        graphs = dict(plain=graphed(torch, lambda: rings[0].append_rollout(ro, range(n)), calls),
                      nstep=graphed(torch, lambda: app.append_rollout(ro, range(n)), calls),
                      fold_carry=graphed(torch, fold_carry, calls))
        times = BD.alternate(torch, {name: g.replay for name, g in graphs.items()}, REPS, args.blocks)
        torch.cuda.synchronize()
        per = {name: BD.stats([v / calls for v in x]) for name, x in times.items()}
        kept = int(rings[0]._stored)
        word = 4 * n * (2 * D + 4 + 1) + n                                       # bytes of one ring row
        ratio = per["nstep"]["median_ms"] / per["plain"]["median_ms"]
        entry = dict(games=E, team=f"{n}v{n}", rows=rows, rows_kept_plain=kept, rows_kept_nstep=int(rings[1]._stored), calls_per_graph=calls,
                     per_call=per, nstep_over_plain=round(ratio, 3),
                     bytes=dict(plain=2 * kept * word, nstep=2 * rows * word + 2 * int(rings[1]._stored) * word,
                                note="read + written, from shapes: the plain append moves its kept rows once; the fold reads and stages every "
                                     "row of the call (its carry copy apart), the append then moves the kept ones"))
        if ratio > 3.0:
            f = per["fold_carry"]["median_ms"]
            entry["where_the_time_goes"] = (f"above 3x: the fold and carry launches alone take {f:.4f} ms of the call's "
                                            f"{per['nstep']['median_ms']:.4f} ms, the ring's own three launches on the staged source the rest")
        result["sizes"].append(entry)
        del graphs, rings, app, lone, ro, env
        torch.cuda.empty_cache()
    print(json.dumps(result))
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
