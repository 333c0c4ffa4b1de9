#!/usr/bin/env python3
"""GAE on device (advantage.gae, csrc/bsx_advantage.hip) at the C5 sizes: 65 536 games x 1v1 and x 4v4, T = 32, on the records of a real
categorical-policy rollout with a value head (PolicyRollout(sample="categorical", value_actor=...)).

    python tools/bench_advantage.py --out plain.json                                     # measurements, profiler off
    rocprofv3 --kernel-trace --stats --output-format csv -d prof1 -- python tools/bench_advantage.py --teams 1 --reps 20 --out prof1.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof4 -- python tools/bench_advantage.py --teams 4 --reps 20 --out prof4.json
    python tools/bench_advantage.py --merge --reps 20 --result plain.json --kernel-trace 1=prof1/<host>/<pid>_kernel_trace.csv,4=prof4/... \\
        --out profiles/advantage.json                                                   # no GPU needed

Per team size, after warm-up, medians over `reps` of device events around:
  gae_us         advantage.gae, plain (one launch)                                          } per call: 20 calls back to back in one
  gae_norm_us    advantage.gae(normalize=True) (GAE + tile moments, one-workgroup merge, scale)  } graph, events around its replay / 20
  torch_us       the textbook reverse loop with the same float32 maths (mask, where, mul, add per tick) captured in ONE torch graph and
                 replayed -- what a learner writes without the kernel
  value_us       the value-only bootstrap pass V(obs[T]) (FusedActor.forward_into with value=, no noise: the actor half runs too), as gae_us
  rollout_us     one replay of the rollout itself (T ticks, no gae=), for scale
Bytes are what the contract moves, from shapes: per column and tick rew, value (4 + 4), done (1) in, adv, ret (4 + 4), mask (1) out;
env_done one byte per game and tick; last_value (4) and done_prev (1 in, 1 out) per column.  normalize adds a pass that reads every mask
byte and reads and writes the masked advantages.  The value pass: the observation row in, 4 scores and the value out.
Kernel times: the profiled runs (one team each) log nothing; --merge takes the medians of every bsx_gae_* dispatch, and of the LAST
20 * (reps + 2) actor-kernel dispatches (the value phase runs last in the process), from each trace."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, T = 65536, 32
GAMMA, LAM = 0.99, 0.95


def gae_bytes(T, E, A):
    N = E * A
    return 18 * T * N + T * E + 6 * N


def norm_extra_bytes(T, E, A, masked):
    return T * E * A + 8 * masked


def value_bytes(E, A, D):
    return E * A * (4 * D + 16 + 4)


def events_us(fn, reps, torch):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def graph_us(fn, reps, torch, k=20):
    """Per call: k calls captured back to back into one graph, device events around a replay, / k (a Python call's host time would
    otherwise sit between the events: the kernels are shorter than their host-side validation)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(k):
            fn()
    for _ in range(2):
        g.replay()
    return events_us(g.replay, reps, torch) / k


def torch_gae(rew, value, last_value, done, env_done, done_prev, adv, ret, mask, g, gl):
    """The same contract as bsx_gae in torch ops (float32, each op rounded on its own), for the graph comparison.  g, gl: float32
    device scalars gamma and gamma * lam (made before a capture: a host-to-device copy cannot be captured)."""
    import torch
    T = rew.shape[0]
    zero = torch.zeros_like(last_value)
    an = zero
    for t in range(T - 1, -1, -1):
        before = done_prev if t == 0 else done[t - 1]
        m = (env_done[t] == 0)[:, None] & (before == 0)
        term = done[t] != 0
        nv = torch.where(term, zero, last_value if t == T - 1 else value[t + 1])
        a = torch.where(term, zero, an)
        a = ((rew[t] + g * nv) - value[t]) + gl * a
        adv[t] = torch.where(m, a, zero)
        ret[t] = torch.where(m, a + value[t], zero)
        mask[t] = m
        an = adv[t]
    done_prev.copy_(done[T - 1])


def one_team(n, reps, torch):
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import advantage
    from deep_rl_battlespace_amd.rollout import FusedActor, PolicyRollout, StackedActor
    A, D = 2 * n, 3 * n + 2
    torch.manual_seed(5)
    actor, critic = StackedActor(A, D, 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=1, auto_reset=True, device="cuda")
    env.reset()
    ro = PolicyRollout(env, actor, T, seed=3, one_launch=(n == 1), sample="categorical", temperature=1.0, value_actor=critic)
    ro.start(); ro.capture()
    for _ in range(6):                                                   # past the first games' ends (tie at 121 ticks in 1v1)
        ro.run()
    torch.cuda.synchronize()
    res = dict(n=n, E=E, T=T, A=A, form="one launch" if n == 1 else f"graph, chains={ro.chains}", gamma=GAMMA, lam=LAM)
    res["rollout_us"] = events_us(ro.run, reps, torch)
    torch.cuda.synchronize()
    lv = torch.zeros((E, A), dtype=torch.float32, device="cuda")
    prev0 = ro._done[T - 1].clone()
    prev = prev0.clone()
    adv, ret = torch.empty_like(ro.rew), torch.empty_like(ro.rew)
    mask = torch.empty((T, E, A), dtype=torch.uint8, device="cuda")
    stats = torch.zeros(3, dtype=torch.float64, device="cuda")
    ws = torch.empty(advantage.workspace_bytes(E, A, T), dtype=torch.uint8, device="cuda")
    fused = FusedActor(actor, n, seed=0)
    scores = torch.empty((E, A, 4), dtype=torch.float32, device="cuda")
    vw = critic.pack()

    def value_pass():
        fused.forward_into(ro.obs[T], scores, 0.0, seq=0, value=dict(weights=vw, out=lv))

    def plain():
        advantage.gae(ro.rew, ro.value, lv, ro._done, ro.env_done, prev, GAMMA, LAM, out=(adv, ret, mask))

    def norm():
        advantage.gae(ro.rew, ro.value, lv, ro._done, ro.env_done, prev, GAMMA, LAM, normalize=True, out=(adv, ret, mask), stats=stats,
                      workspace=ws)
    value_pass(); plain()
    torch.cuda.synchronize()
    masked = int(mask.sum())
    res.update(masked_rows=masked, rows=T * E * A, gae_bytes=gae_bytes(T, E, A), gae_norm_bytes=gae_bytes(T, E, A) + norm_extra_bytes(T, E, A, masked),
               value_bytes=value_bytes(E, A, D))
    res["gae_us"] = graph_us(plain, reps, torch)
    res["gae_norm_us"] = graph_us(norm, reps, torch)
    # the torch loop, captured once, checked against the kernel's bits on the same inputs
    t_adv, t_ret, t_mask, t_prev = torch.empty_like(adv), torch.empty_like(ret), torch.empty_like(mask), prev.clone()
    gs = torch.tensor(GAMMA, dtype=torch.float32, device="cuda")
    gls = gs * torch.tensor(LAM, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch_gae(ro.rew, ro.value, lv, ro._done, ro.env_done, t_prev, t_adv, t_ret, t_mask, gs, gls)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        torch_gae(ro.rew, ro.value, lv, ro._done, ro.env_done, t_prev, t_adv, t_ret, t_mask, gs, gls)
    prev.copy_(prev0); t_prev.copy_(prev0)
    plain(); g.replay()
    torch.cuda.synchronize()
    res["torch_equals_kernel"] = bool(torch.equal(adv.view(torch.int32), t_adv.view(torch.int32)) and torch.equal(ret, t_ret)
                                      and torch.equal(mask, t_mask))
    for _ in range(3):
        g.replay()
    res["torch_us"] = events_us(g.replay, reps, torch)
    res["value_us"] = graph_us(value_pass, reps, torch)              # last: the profiled runs take the last actor dispatches
    for k in ("gae", "gae_norm"):
        res[k + "_TBps"] = res[k + "_bytes"] / res[k + "_us"] / 1e6
    res["torch_TBps"] = res["gae_bytes"] / res["torch_us"] / 1e6
    res["value_TBps"] = res["value_bytes"] / res["value_us"] / 1e6
    res["gae_share_of_rollout"] = res["gae_us"] / res["rollout_us"]
    return res


DOC = dict(
    what="GAE advantages on device (advantage.gae, csrc/bsx_advantage.hip) against a torch reverse loop in one graph, with the value-only "
         "bootstrap pass and the rollout for scale: 65536 games, T = 32, categorical policy + value head, one MI355X",
    commands=["python tools/bench_advantage.py --out plain.json",
              "rocprofv3 --kernel-trace --stats --output-format csv -d prof1 -- python tools/bench_advantage.py --teams 1 --reps 20 --out prof1.json",
              "rocprofv3 --kernel-trace --stats --output-format csv -d prof4 -- python tools/bench_advantage.py --teams 4 --reps 20 --out prof4.json",
              "python tools/bench_advantage.py --merge --reps 20 --result plain.json --kernel-trace 1=prof1/.../_kernel_trace.csv,4=prof4/... "
              "--out profiles/advantage.json"],
    units=dict(times="microseconds, medians over --reps", rates="TB/s = contract bytes / time, 1e12 bytes"),
    method=dict(
        bytes="gae_bytes = 18*T*E*A (rew, value, done in; adv, ret, mask out) + T*E (env_done) + 6*E*A (last_value, done_prev in and out); "
              "gae_norm_bytes adds T*E*A mask bytes and 8 bytes per masked row (the scale pass); value_bytes = E*A*(4D + 16 + 4)",
        events="device events around one graph replay: 20 calls back to back (gae, gae_norm, value; the figure is per call) or the graph "
               "itself (torch, rollout)",
        kernels_rocprofv3="per-dispatch durations from the profiled runs (one process per team): medians per kernel; value = the last 20*(reps+2) "
                          "dispatches of the actor kernel"))


def merge(result, traces, reps):
    """The committed file: the plain run's measurements + kernel medians from the profiled runs' traces (traces: {n: csv path})."""
    import csv
    plain = json.load(open(result))
    out = dict(DOC, device=plain["device"], torch=plain["torch"], results=[])
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3     # noqa: E731
    for r in plain["results"]:
        res = dict(r)
        if r["n"] in traces:
            rows = sorted(csv.DictReader(open(traces[r["n"]])), key=lambda x: int(x["Start_Timestamp"]))
            k = {}
            for x in rows:
                if "bsx_gae_" in x["Kernel_Name"]:
                    k.setdefault(x["Kernel_Name"], []).append(us(x))
            res["kernels_rocprofv3"] = {nm: dict(median_us=round(statistics.median(v), 2), calls=len(v)) for nm, v in sorted(k.items())}
            plain_k = [statistics.median(v) for nm, v in k.items() if "bsx_gae_kernel<" in nm]
            if plain_k:
                res["gae_kernel_us"] = plain_k[0]
                res["gae_kernel_TBps"] = r["gae_bytes"] / plain_k[0] / 1e6
            actor = [us(x) for x in rows if "bsx_actor_kernel" in x["Kernel_Name"]]
            res["value_kernel_us"] = statistics.median(actor[-20 * (reps + 2):])
        rnd = lambda x: round(x, 3) if isinstance(x, float) else x      # noqa: E731
        out["results"].append({a: rnd(b) for a, b in res.items()})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--teams", default="1,4")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--merge", action="store_true", help="combine --result and --kernel-trace n=path,... into --out (no GPU); --reps = "
                    "the profiled runs' reps")
    ap.add_argument("--result"); ap.add_argument("--kernel-trace")
    a = ap.parse_args(argv)
    if a.merge:
        out = merge(a.result, {int(t.split("=", 1)[0]): t.split("=", 1)[1] for t in a.kernel_trace.split(",")}, a.reps)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_advantage.py measures on the MI355X: no GPU visible")
        results = [one_team(int(n), a.reps, torch) for n in a.teams.split(",")]
        out = dict(tool="tools/bench_advantage.py", argv=sys.argv[1:], device=torch.cuda.get_device_name(0), torch=torch.__version__,
                   results=results)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
