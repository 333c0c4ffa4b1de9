#!/usr/bin/env python3
"""What epsilon-greedy exploration costs a rollout, and that the greedy path costs what it did (profiles/epsilon_greedy.json):
microseconds per tick of a captured PolicyRollout at 65 536 x 1v1, T = 32, as the per-tick graph and as one launch -- greedy, and with
epsilon = 0.1 with and without the `explored` record -- and bsx_epsilon_advance's time per launch.  Runs on the GPU box.

    python tools/measure_epsilon.py                                   # this checkout, one JSON line
    python tools/measure_epsilon.py --root DIR                        # another checkout of the project (one without epsilon=: greedy only)
    python tools/measure_epsilon.py --against DIR --rounds 4 --json profiles/epsilon_greedy.json
                                                                      # DIR (the parent commit, built) and this checkout in ALTERNATING
                                                                      # processes: per figure the median over the rounds and every round's value,
                                                                      # the parent's own spread next to the difference

Each figure is the median of `--windows` timed windows of `--reps` synchronised-at-the-end replays after three warm-up replays."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(root, E, n, T, reps, windows):
    sys.path.insert(0, root)
    import torch
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import rollout as R

    def window(fn):
        for _ in range(3):
            fn()
        out = []
        for _ in range(windows):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / reps)
        return statistics.median(out)

    def rollout_us(one_launch, epsilon=None, record=True):
        env = bsx.parallel_env(n_agents=n, n_envs=E, auto_reset=True, seed=1234)
        env.reset()
        torch.manual_seed(0)
        actor = R.StackedActor(2 * n, 3 * n + 2, 4, device="cuda")
        with torch.no_grad():
            actor.w3.mul_(100.0)
        kw = {} if epsilon is None else dict(epsilon=epsilon)
        ro = R.PolicyRollout(env, actor, T, one_launch=one_launch, chains=1, **kw)
        if not record:                               # the same launches without the `explored` pointer
            plain = ro.fused.noise_struct

            def bare(E, noise_std=0.0, ou=None, z=None, sample=None, value=None, epsilon=None):
                return plain(E, noise_std, ou, z, sample, value, {f: v for f, v in epsilon.items() if f != "explored"})
            ro.fused.noise_struct = bare
        ro.start(); ro.capture()
        return round(window(ro.run) / T * 1e6, 3)

    res = {"root": os.path.abspath(root), "games": E, "n": n, "T": T, "reps": reps, "windows": windows}
    has_eps = hasattr(R, "EpsilonSchedule")
    for form, one in (("per_tick_graph", False), ("one_launch", True)):
        res[f"{form}_greedy_us_per_tick"] = rollout_us(one)
        if has_eps:
            res[f"{form}_epsilon_0.1_us_per_tick"] = rollout_us(one, 0.1)
            res[f"{form}_epsilon_0.1_no_record_us_per_tick"] = rollout_us(one, 0.1, record=False)
    if has_eps:
        sched = R.EpsilonSchedule(1.0, 0.1, 1000000).bind(2 * n, "cuda")
        g = torch.cuda.CUDAGraph()
        sched.advance(1); torch.cuda.synchronize()
        with torch.cuda.graph(g):
            for _ in range(100):
                sched.advance(1)
        res["epsilon_advance_us_per_launch_in_a_graph_of_100"] = round(window(g.replay) / 100 * 1e6, 3)
        res["epsilon_advance_us_per_launch_eager"] = round(window(lambda: sched.advance(1)) * 1e6, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE); ap.add_argument("--against"); ap.add_argument("--rounds", type=int, default=4); ap.add_argument("--json")
    ap.add_argument("--envs", type=int, default=65536); ap.add_argument("--n-agents", type=int, default=1); ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not a.against:
        print(json.dumps(measure(a.root, a.envs, a.n_agents, a.T, a.reps, a.windows)))
        return 0
    sizes = ["--envs", str(a.envs), "--n-agents", str(a.n_agents), "--T", str(a.T), "--reps", str(a.reps), "--windows", str(a.windows)]
    runs = {"parent": [], "this": []}
    for r in range(a.rounds):                        # alternating, a fresh process each: other work shares the host
        for who, root in (("parent", a.against), ("this", HERE)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, *sizes], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                return p.returncode or 1
            runs[who].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(who, r, p.stdout.strip().splitlines()[-1], flush=True)
    out = {"method": "tools/measure_epsilon.py --against PARENT: parent commit and this tree in alternating processes, per process the median of "
                     f"{a.windows} windows of {a.reps} replays; per figure the median over {a.rounds} rounds, every round's value kept",
           "workload": f"{a.envs} games x {a.n_agents}v{a.n_agents}, T = {a.T}, captured PolicyRollout, f32, no opponent"}
    for who, rs in runs.items():
        keys = [k for k in rs[0] if k.endswith("_tick") or "advance" in k]
        out[who] = {k: {"median": statistics.median(x[k] for x in rs), "rounds": [x[k] for x in rs]} for k in keys}
    for form in ("per_tick_graph", "one_launch"):
        k = f"{form}_greedy_us_per_tick"
        p, t = out["parent"][k], out["this"][k]
        out[f"{form}_greedy"] = {"parent_us_per_tick": p["median"], "this_us_per_tick": t["median"], "difference": round(t["median"] - p["median"], 3),
                                 "parent_spread_max_minus_min": round(max(p["rounds"]) - min(p["rounds"]), 3)}
    print(json.dumps(out, indent=1))
    if a.json:
        prev = json.load(open(a.json)) if os.path.exists(a.json) else {}
        prev["rollout_timings"] = out
        json.dump(prev, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
