#!/usr/bin/env python3
"""What a centralised critic (PolicyRollout(central_critic=), PPOLearner on it: MAPPO) costs and saves, on one GPU.

    python tools/bench_mappo.py --parent <tree of the parent commit, built> [--blocks 7] [--trace-dir DIR] [--out profiles/mappo_update.json]

Shapes: 65 536 x 1v1, 4 096 x 2v2 and 4 096 x 4v4 at T = 32, categorical head, epochs = 4, minibatches = 4, max_grad_norm 0.5,
device_step=True, every update captured.  Timed with device events in ALTERNATING blocks after a warm-up of every path; per path the
median, minimum and maximum block and the spread (max - min) / median.
  rollout  (a) us per tick of a captured run(): central_critic in the per-tick graph and in the one-launch form, against the same
           rollout with value_actor (per-tick graph; one launch at 1v1, the only size that form takes a value head at).  The central
           figures include the critic's pass over the T + 1 ticks' records (join + forward), the value_actor figures its value pass.
  update   (b) ms per captured update(): central against the own-critic PPOLearner of THIS tree (alternating blocks in one process)
           and of the PARENT commit (--parent: processes of the two trees, alternating, each measuring the own-critic update and the
           value_actor rollout: the guard that the default path did not move).  The join's share of the central update: kernel time by
           name from `rocprofv3 --kernel-trace` of one process that replays the captured update (a run of its own; --no-trace skips it).
  join     (c) bsx_ppo_joint_obs alone on the T + 1 ticks' observation rows, sixteen launches captured as one graph: us per launch and
           the algorithmic bytes R A Do (1 + n) 4 over it.
One JSON line on stdout, also written to --out with the commands."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((65536, 1), (4096, 2), (4096, 4))          # (E, n)
T, TAU = 32, 0.7
TRACE_UPDATES = 24
KW = dict(clip=0.2, c_v=0.5, c_e=0.01, vclip=0.2, epochs=4, minibatches=4, max_grad_norm=0.5, device_step=True)


def stats(x, unit="ms", scale=1.0):
    x = [v * scale for v in x]
    m = statistics.median(x)
    return {f"median_{unit}": round(m, 4), f"min_{unit}": round(min(x), 4), f"max_{unit}": round(max(x), 4), "spread": round((max(x) - min(x)) / m, 4)}


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
    """steps: {name: callable}.  Warm-up of all, then `blocks` rounds of one block each, in turn -> {name: [ms per call]}."""
    for _ in range(2):
        for s in steps.values():
            s()
    torch.cuda.synchronize()
    out = {k: [] for k in steps}
    for _ in range(blocks):
        for k, s in steps.items():
            out[k].append(block(torch, s, reps))
    return out


def make_rollout(E, n, critic, one_launch=False):
    """A captured PolicyRollout after two runs: critic "central", "own" or None."""
    import torch
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    A, D = 2 * n, 3 * n + 2
    torch.manual_seed(0)
    actor = StackedActor(A, D, 4, device="cuda")
    net = StackedActor(A, n * D if critic == "central" else D, 1, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(50.0); net.w3.mul_(50.0)
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=1, auto_reset=True, device="cuda")
    env.reset()
    kw = dict(gae=dict(gamma=0.99, lam=0.95)) if critic else {}
    if critic:
        kw["central_critic" if critic == "central" else "value_actor"] = net
    ro = PolicyRollout(env, actor, T, seed=3, sample="categorical", temperature=TAU, one_launch=one_launch, chains=1, **kw)
    ro.start(); ro.capture()
    ro.run(); ro.run()
    torch.cuda.synchronize()
    return ro


def default_path(args):
    """--role default: the own-critic update and the value_actor rollout of whatever tree this file's package is imported from."""
    import torch
    from deep_rl_battlespace_amd.learner import PPOLearner
    out = []
    for E, n in SHAPES:
        ro = make_rollout(E, n, "own")
        learner = PPOLearner(ro, **KW).capture()
        t = alternate(torch, dict(run=ro.run, update=learner.update), 8, args.blocks)
        out.append(dict(games=E, n=n, rollout_us_per_tick=stats(t["run"], "us", 1e3 / T), update_ms=stats(t["update"])))
        del learner, ro
        torch.cuda.empty_cache()
    return out


def trace_role(args):
    """--role trace: replay the captured central update of one shape a few times (run under rocprofv3 --kernel-trace)."""
    import torch
    from deep_rl_battlespace_amd.learner import PPOLearner
    E, n = SHAPES[args.shape]
    learner = PPOLearner(make_rollout(E, n, "central"), **KW).capture()
    for _ in range(TRACE_UPDATES):
        learner.update()
    torch.cuda.synchronize()


def child(tree, role, blocks, extra=(), wrap=()):
    """This file run as a fresh process on the package of `tree` -> its last stdout line as JSON (None for the trace role).  The
    orchestrating process never opens the GPU itself: every measurement is a process of its own."""
    env = dict(os.environ, BSX_BENCH_TREE=tree)
    cmd = [*wrap, sys.executable, os.path.abspath(__file__), "--role", role, "--blocks", str(blocks), *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-1500:]}")
    return json.loads(r.stdout.strip().splitlines()[-1]) if role != "trace" else None


def join_share(d):
    """Kernel time by name in the kernel trace under `d`, of one process replaying the captured central update -> dict(share of
    bsx_ppo_joint_obs, ...)."""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"no kernel trace under {d}")
    by_name = {}
    for r in csv.DictReader(open(files[0])):
        by_name[r["Kernel_Name"]] = by_name.get(r["Kernel_Name"], 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    # the process also plays two warm-up rollouts: their step kernels are left out by name; what is left is TRACE_UPDATES + 1 updates
    # (the capture's eager one) and the two rollouts' critic passes, 2 x (T + 1) ticks of join and forward against TRACE_UPDATES x 4 x T
    rest = {k: v for k, v in by_name.items() if "bsx_step" not in k and "bsx_rollout" not in k}
    total = sum(rest.values())
    join = sum(v for k, v in rest.items() if "joint_obs" in k)
    top = sorted(rest.items(), key=lambda kv: -kv[1])[:8]
    return dict(updates_traced=TRACE_UPDATES, join_ns=join, kernels_ns=total, join_share_of_kernel_time=round(join / total, 4) if total else None,
                top_kernels_ns={k[:70]: v for k, v in top})


def central_path(args):
    """--role central: (a), (b) against this tree's own critic and (c), all shapes in one process -> (device name, the entries)."""
    import torch
    from deep_rl_battlespace_amd.learner import PPOLearner, joint_obs
    entries = []
    for E, n in SHAPES:
        A, D = 2 * n, 3 * n + 2
        entry = dict(games=E, n=n, agents=A, obs_len=D, critic_inputs=n * D)
        # (a) the rollouts
        ros = dict(central_graph=make_rollout(E, n, "central"), central_one_launch=make_rollout(E, n, "central", one_launch=True),
                   own_graph=make_rollout(E, n, "own"))
        if n == 1:
            ros["own_one_launch"] = make_rollout(E, n, "own", one_launch=True)
        t = alternate(torch, {k: ro.run for k, ro in ros.items()}, 16, args.blocks)
        entry["rollout_us_per_tick"] = {k: stats(v, "us", 1e3 / T) for k, v in t.items()}
        entry["central_chunk_ticks"] = ros["central_graph"].central_chunk
        # (b) the updates, this tree: central against own, alternating
        central, own = PPOLearner(ros["central_graph"], **KW).capture(), PPOLearner(ros["own_graph"], **KW).capture()
        t = alternate(torch, dict(central=central.update, own=own.update), 4, args.blocks)
        entry["update_ms"] = dict(central=stats(t["central"]), own_this_tree=stats(t["own"]),
                                  central_over_own=round(statistics.median(t["central"]) / statistics.median(t["own"]), 4))
        # (c) the join alone, on the T + 1 ticks' rows
        obs = ros["central_graph"].obs.view(-1, A, D)
        x = torch.empty((obs.shape[0], A, n * D), device="cuda")
        joint_obs(obs, out=x)
        torch.cuda.synchronize()
        sixteen = torch.cuda.CUDAGraph()
        with torch.cuda.graph(sixteen):
            for _ in range(16):
                joint_obs(obs, out=x)
        sixteen.replay()
        j = [block(torch, sixteen.replay, 8) / 16 for _ in range(args.blocks)]
        nbytes = obs.shape[0] * A * D * (1 + n) * 4
        entry["join"] = dict(stats(j, "us", 1e3), rows=obs.shape[0], algorithmic_bytes=nbytes,
                             gb_per_s=round(nbytes / (statistics.median(j) * 1e-3) / 1e9, 1))
        # the join's time inside one update by device events: sixteen minibatches of T / 4 ticks' rows each
        mb_rows = T // KW["minibatches"] * E
        sixteen_mb = torch.cuda.CUDAGraph()
        with torch.cuda.graph(sixteen_mb):
            for _ in range(16):
                joint_obs(obs[:mb_rows], out=x[:mb_rows])
        sixteen_mb.replay()
        jm = [block(torch, sixteen_mb.replay, 8) for _ in range(args.blocks)]
        entry["join"]["sixteen_minibatch_joins_ms"] = stats(jm)
        entry["join"]["share_of_central_update_by_events"] = round(statistics.median(jm) / statistics.median(t["central"]), 4)
        del sixteen, sixteen_mb, central, own, ros, obs, x
        torch.cuda.empty_cache()
        entries.append(entry)
    return dict(device=torch.cuda.get_device_name(0), shapes=entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the default-path guard")
    ap.add_argument("--role", default="main", choices=("main", "central", "default", "trace"))
    ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build", "mappo_trace"), help="where the rocprofv3 runs write (build/ is not tracked)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappo_update.json"))
    args = ap.parse_args()
    if args.role != "main":
        sys.path.insert(0, os.environ.get("BSX_BENCH_TREE") or ROOT)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_mappo.py measures on the GPU: none found")
        if args.role == "trace":
            trace_role(args)
        else:
            print(json.dumps(default_path(args) if args.role == "default" else central_path(args)))
        return
    measured = child(ROOT, "central", args.blocks)
    result = dict(command=f"python tools/bench_mappo.py --parent <parent tree> --blocks {args.blocks}", device=measured["device"],
                  blocks=args.blocks, ticks=T, learner=KW, shapes=measured["shapes"])
    for i, entry in enumerate(result["shapes"]):
        if args.no_trace:
            entry["join"]["kernel_trace"] = dict(not_measured="--no-trace")
            continue
        d = os.path.join(args.trace_dir, f"mappo_trace_{i}")
        # (a traced process that fails ends the whole tool, like any other child: nothing more is started on the GPU after it)
        child(ROOT, "trace", args.blocks, ["--shape", str(i)], ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"])
        try:
            entry["join"]["kernel_trace"] = join_share(d)
        except (OSError, KeyError, ValueError, RuntimeError) as exc:  # a trace that cannot be read: the figure is missing, and the file says why
            entry["join"]["kernel_trace"] = dict(not_measured=str(exc)[-600:])
    # the guard on the default path: this tree and the parent commit, processes in turn
    if args.parent:
        runs = []
        for rep in range(2):
            for name, tree in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
                runs.append(dict(tree=name, rep=rep, shapes=child(tree, "default", args.blocks)))
        guard = []
        for i, (E, n) in enumerate(SHAPES):
            g = dict(games=E, n=n)
            for key, unit in (("update_ms", "ms"), ("rollout_us_per_tick", "us")):
                med = {name: [r["shapes"][i][key][f"median_{unit}"] for r in runs if r["tree"] == name] for name in ("parent", "this")}
                lo = {name: min(r["shapes"][i][key][f"min_{unit}"] for r in runs if r["tree"] == name) for name in med}
                hi = {name: max(r["shapes"][i][key][f"max_{unit}"] for r in runs if r["tree"] == name) for name in med}
                g[key] = dict(parent_medians=med["parent"], this_medians=med["this"], parent_range=[lo["parent"], hi["parent"]],
                              this_range=[lo["this"], hi["this"]],
                              this_median_inside_parents_range=bool(lo["parent"] <= statistics.median(med["this"]) <= hi["parent"]))
            guard.append(g)
        result["default_path_guard"] = dict(what="own-critic PPOLearner.update() (captured) and a value_actor rollout: four processes in turn, "
                                                 "parent, this, parent, this; range = the smallest and largest block over both processes of a tree",
                                            shapes=guard, runs=runs)
    else:
        result["default_path_guard"] = dict(not_measured="no --parent tree given")
    print(json.dumps(result))
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
