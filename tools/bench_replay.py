#!/usr/bin/env python3
"""The device replay ring against the torch ring (replay.DeviceReplayBuffer vs ReplayBuffer) at the reference's sizes: 65 536 games,
T = 32 ticks per rollout, the red team, a ring of 1 000 000 rows (maddpg/buffer.py; SURVEY.md component table row 7).

    python tools/bench_replay.py --out plain.json                                     # measurements, profiler off
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python tools/bench_replay.py --reps 10 --out profiled.json
    python tools/bench_replay.py --merge --result plain.json --profiled profiled.json --kernel-trace prof/<host>/<pid>_kernel_trace.csv \
        --out profiles/replay_device.json                                            # no GPU needed

Per team size it measures, after warm-up, medians over `reps`:
  append_us           DeviceReplayBuffer.append_rollout of one rollout into the 1 000 000-row ring, device events around it.  A rollout
                      keeps ~2.07 M rows > M: the newest M are written, the rest only counted (as ReplayBuffer._put keeps them)
  append_M_ge_R_us    the same append into a ring of 2^22 rows, where every kept row is written
  store_rollout_us    ReplayBuffer.store_rollout of the same rollout, host clock from a synchronised start to its return (it syncs)
  sample[B]           DeviceReplayBuffer.sample() and ReplayBuffer.sample() at B = 512 (the reference's batch) and 65 536, device events
  loop_us             rollout + store + sample (B = 512): ONE graph (PolicyRollout.capture(then=...)) replayed and synchronised, against
                      ro.run(); ReplayBuffer.store_rollout(); ReplayBuffer.sample(); synchronise -- host clock per iteration
Bytes are counted from shapes, for what each path has to move.  Row body = 4*nA*(2D + n_act + 1) bytes (both observations, the actions,
the rewards) + nA done bytes.  A device append reads one skip byte per source row and, for the min(R, M) rows it stores, reads and writes
a row body each.  The torch path index-selects every kept row before its ring slices them: R rows read and written.  A draw reads a row
and writes it, plus 8 bytes of index.  Kernel times come from the profiled run: the tool logs every append and sample it issues, in
order, and --merge pairs that log with the replay kernels' dispatches in the trace."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, T, M = 65536, 32, 1_000_000
M_BIG = 1 << 22                                      # >= T * E: every kept row of a rollout is written
CALLS = []                                           # (kind, label) of every append / sample issued, in issue order (--merge)


def row_body(nA, D, n_act):
    """Bytes of one ring row: observation, next observation, actions, reward (float32) + the done bytes."""
    return 4 * nA * (2 * D + n_act + 1) + nA


def device_append_bytes(rows_total, kept, mem, body):
    """What a device append has to move: a skip byte per source row, and the min(R, M) rows it stores read and written."""
    return rows_total + 2 * min(kept, mem) * body


def events_us(fn, reps, torch):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def wall_us(fn, reps, torch):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def one_team(n, reps, torch):
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, ReplayBuffer
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor

    def rollout(seed):
        env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, device="cuda"); env.reset()
        torch.manual_seed(seed)
        actor = StackedActor(2 * n, 3 * n + 2, 4, device="cuda")
        ro = PolicyRollout(env, actor, T, noise_std=0.1, one_launch=True, opponent=instinct.Team(env.possible_blue, env.possible_red, env))
        ro.start()
        return env, ro

    def append(buf, ro, label):                      # every device append and sample goes through these two: the call log
        CALLS.append(("append", f"n{n}/{label}"))
        return buf.append_rollout(ro, cols)

    def sample(buf, label):
        CALLS.append(("sample", f"n{n}/{label}"))
        return buf.sample()
    env, ro = rollout(1)
    D, cols = env.obs_size, range(n)
    args = (env.possible_red, D, D * n, 4)
    ro.capture()
    for _ in range(3):                               # past the first games' ends: a steady share of kept rows
        ro.run()
    torch.cuda.synchronize()
    kept, total, body = int((ro.env_done[:T] == 0).sum()), T * E, row_body(n, D, 4)
    res = dict(n=n, E=E, T=T, M=M, team="red", D=D, n_act=4, rows_kept=kept, rows_total=total, row_body_bytes=body,
               append_bytes=device_append_bytes(total, kept, M, body), append_M_ge_R_bytes=device_append_bytes(total, kept, M_BIG, body),
               store_rollout_bytes=2 * kept * body)

    dev = DeviceReplayBuffer(M, 512, *args, device="cuda", seed=0)
    ref = ReplayBuffer(M, 512, *args, device="cuda")
    for _ in range(3):
        append(dev, ro, "warm"); ref.store_rollout(ro, cols)
    res["append_us"] = events_us(lambda: append(dev, ro, "append"), reps, torch)
    res["append_GBps"] = res["append_bytes"] / res["append_us"] / 1e3

    def dev_store():
        CALLS.append(("append", f"n{n}/store_rollout"))
        return dev.store_rollout(ro, cols)
    res["device_store_rollout_us"] = wall_us(dev_store, reps, torch)
    res["store_rollout_us"] = wall_us(lambda: ref.store_rollout(ro, cols), reps, torch)
    res["store_rollout_GBps"] = res["store_rollout_bytes"] / res["store_rollout_us"] / 1e3

    big = DeviceReplayBuffer(M_BIG, 512, *args, device="cuda", seed=0)
    for _ in range(2):
        append(big, ro, "warm")
    res["M_big"] = M_BIG
    res["append_M_ge_R_us"] = events_us(lambda: append(big, ro, "append_M_ge_R"), reps, torch)
    res["append_M_ge_R_GBps"] = res["append_M_ge_R_bytes"] / res["append_M_ge_R_us"] / 1e3
    del big
    torch.cuda.empty_cache()

    res["sample"] = {}
    draw = body + (body + 8)                         # read a row; write it and its index
    for B in (512, 65536):
        d = DeviceReplayBuffer(M, B, *args, device="cuda", seed=0) if B != 512 else dev
        r = ReplayBuffer(M, B, *args, device="cuda") if B != 512 else ref
        if B != 512:
            for _ in range(2):
                append(d, ro, "warm"); r.store_rollout(ro, cols)
        for _ in range(3):
            sample(d, "warm"); r.sample()
        dus = events_us(lambda: sample(d, f"sample_B{B}"), reps, torch)
        rus = events_us(r.sample, reps, torch)
        res["sample"][str(B)] = dict(device_us=dus, torch_us=rus, bytes=B * draw, device_GBps=B * draw / dus / 1e3)
        if B != 512:
            del d, r
            torch.cuda.empty_cache()

    # rollout + store + sample: one graph against the torch loop, each iteration synchronised (a learner consumes the batch)
    env2, ro2 = rollout(2)
    g_dev = DeviceReplayBuffer(M, 512, *args, device="cuda", seed=0)
    ro2.capture(then=lambda: (g_dev.append_rollout(ro2, cols), g_dev.sample()))     # recorded, not run: logged per replay below
    _, ro3 = rollout(2)
    ro3.capture()
    t_ref = ReplayBuffer(M, 512, *args, device="cuda")

    def graph_loop():
        CALLS.append(("append", f"n{n}/loop")); CALLS.append(("sample", f"n{n}/loop"))
        ro2.run()

    def torch_loop():
        ro3.run(); t_ref.store_rollout(ro3, cols); t_ref.sample()
    for _ in range(3):
        graph_loop(); torch_loop()
    torch.cuda.synchronize()
    res["loop_us"] = dict(one_graph=wall_us(graph_loop, reps, torch), torch_path=wall_us(torch_loop, reps, torch),
                          rollout_only=wall_us(ro3.run, reps, torch))
    return res


DOC = dict(
    what="Device replay ring (DeviceReplayBuffer, csrc/bsx_replay.hip) vs the torch ring (ReplayBuffer): 65536 games, T = 32, red team, "
         "M = 1 000 000 (and 2^22 for the M >= R point), one MI355X",
    commands=["python tools/bench_replay.py --out plain.json",
              "rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python tools/bench_replay.py --reps 10 --out profiled.json",
              "python tools/bench_replay.py --merge --result plain.json --profiled profiled.json --kernel-trace prof/<host>/<pid>_kernel_trace.csv "
              "--out profiles/replay_device.json"],
    units=dict(times="microseconds; medians over --reps (30 plain, 10 under the profiler)", rates="GB/s = bytes from shapes / time, 1e9 bytes"),
    method=dict(
        append_us="device events around DeviceReplayBuffer.append_rollout into the M = 1 000 000 ring (three kernels + launch gaps); "
                  "rows_kept > M, so min(R, M) = M rows are written",
        append_M_ge_R_us="the same into a ring of M_big = 2^22 rows >= T*E: every kept row is written",
        store_rollout_us="host clock around ReplayBuffer.store_rollout from a synchronised start (it ends in a sync)",
        device_store_rollout_us="host clock around DeviceReplayBuffer.store_rollout (append + reading the count back)",
        sample="device events around sample(), device and torch ring",
        loop_us="host clock per synchronised iteration: one_graph = PolicyRollout.capture(then=append + sample) replayed; torch_path = graph "
                "rollout, ReplayBuffer.store_rollout, ReplayBuffer.sample(); rollout_only = the rollout graph alone",
        bytes="row_body = 4*nA*(2D+n_act+1) + nA.  append_bytes = rows_total skip bytes + 2*min(rows_kept, M)*row_body (what the device append "
              "moves; with R > M the older ranks are counted, never copied).  store_rollout_bytes = 2*rows_kept*row_body (the torch path "
              "index-selects every kept row).  A draw: 2*row_body + 8",
        kernels_rocprofv3="per-dispatch durations of the replay kernels in the profiled run, paired in issue order with the tool's call log; "
                          "medians per labelled phase"))


def merge(result, profiled, trace):
    """The committed file: the plain run's measurements + kernel times from the profiled run's trace, paired with its call log."""
    import csv
    plain, prof = json.load(open(result)), json.load(open(profiled))
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3     # noqa: E731
    disp = {k: [us(r) for r in rows if f"bsx_replay_{k}_kernel" in r["Kernel_Name"]] for k in ("count", "scan", "scatter", "sample")}
    apps = [lab for kind, lab in prof["calls"] if kind == "append"]
    smps = [lab for kind, lab in prof["calls"] if kind == "sample"]
    assert len(disp["count"]) == len(disp["scan"]) == len(disp["scatter"]) == len(apps), (len(disp["scatter"]), len(apps))
    assert len(disp["sample"]) == len(smps), (len(disp["sample"]), len(smps))
    per = {}
    for i, lab in enumerate(apps):
        for k in ("count", "scan", "scatter"):
            per.setdefault(lab, {}).setdefault(k, []).append(disp[k][i])
    for i, lab in enumerate(smps):
        per.setdefault(lab, {}).setdefault("sample", []).append(disp["sample"][i])
    med = lambda v: round(statistics.median(v), 2)                                # noqa: E731
    out = dict(DOC, device=plain["device"], torch=plain["torch"], results=[])
    for r in plain["results"]:
        n, k = r["n"], {}
        for phase, mbytes in (("append", r["append_bytes"]), ("append_M_ge_R", r["append_M_ge_R_bytes"])):
            p = per[f"n{n}/{phase}"]
            t = {name: med(v) for name, v in p.items()}
            t_sum = sum(t.values())
            k[phase] = dict(t, calls=len(p["scatter"]), sum_us=round(t_sum, 2), GBps=round(mbytes / t_sum / 1e3, 1))
        for B in ("512", "65536"):
            v = per[f"n{n}/sample_B{B}"]["sample"]
            k[f"sample_B{B}"] = dict(sample=med(v), calls=len(v), GBps=round(r["sample"][B]["bytes"] / med(v) / 1e3, 1))
        rnd = lambda x: round(x, 2) if isinstance(x, float) else ({a: rnd(b) for a, b in x.items()} if isinstance(x, dict) else x)   # noqa: E731
        out["results"].append(dict(rnd(r), kernels_rocprofv3=k))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--teams", default="1,4")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--merge", action="store_true", help="combine --result, --profiled and --kernel-trace into --out (no GPU)")
    ap.add_argument("--result"); ap.add_argument("--profiled"); ap.add_argument("--kernel-trace")
    a = ap.parse_args(argv)
    if a.merge:
        out = merge(a.result, a.profiled, a.kernel_trace)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_replay.py measures on the MI355X: no GPU visible")
        results = [one_team(int(n), a.reps, torch) for n in a.teams.split(",")]
        out = dict(tool="tools/bench_replay.py", argv=sys.argv[1:], device=torch.cuda.get_device_name(0), torch=torch.__version__,
                   results=results, calls=CALLS)
    text = json.dumps(out, indent=1)
    print(text if a.merge else json.dumps({k: v for k, v in out.items() if k != "calls"}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
