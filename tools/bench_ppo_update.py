#!/usr/bin/env python3
"""The PPO loss head and one whole minibatch of a PPO update over a rollout's records: the fused path (learner.ppo_head: bsx_ppo_head;
PPOLearner.minibatch_grads) against the torch composition of the same loss with autograd, on the same tensors, in one process on one GPU.

    python tools/bench_ppo_update.py [--blocks 7] [--out profiles/ppo_update.json]

Per size and policy head, timed with device events in ALTERNATING blocks (torch, fused, torch, fused ...) after a warm-up of both; a block
is a few back-to-back steps between two events.  Reported per path: the median, minimum and maximum block (ms per step) and the spread
(max - min) / median.
  head       (a) ppo_head alone, into given buffers, against (b) the torch loss from leaf tensors y, v (and log_std) to y.grad and v.grad --
             log_softmax / gather / exp / clamp / minimum / masking / sums and their autograd mirror, the form of
             tests/actor_grad_util.py::_ppo; the played actions (rec.argmax) are handed to the torch path ready-made.  Peak memory
             allocated by one step of each beyond what is held before it.  The fused head's traffic -- the bytes the algorithm moves
             (86 per element with v_old: 16 y + 16 rec + 5 x 4 + 1 mask, read; the mask once more by the count pass; 32 written) over its
             time -- next to bsx_gae's on the same card (19 bytes per element: rew, value, adv, ret, done, mask, and done once more)
  minibatch  (c) PPOLearner.minibatch_grads over a real PolicyRollout's records (pack, one forward with the value head, the loss head,
             two backward calls) against StackedActor forwards, the torch loss and autograd into both networks' parameters
Sizes: R x A = 2 097 152 x 2 (one T = 32 rollout of 65 536 x 1v1) and 524 288 x 8 (T = 8 of 65 536 x 4v4).  One JSON line on stdout, also
written to --out with the command.

    python tools/bench_ppo_update.py --adam [--blocks 7] [--ratios ratios.jsonl] [--out profiles/adam_step.json]

measures the optimiser step instead (learner.adam_step: bsx_adam_step; PPOLearner(device_step=True)), as two alternating A/B pairs at
65 536 x 1v1 and 4 096 x 1v1, T = 32, categorical head, max_grad_norm 0.5:
  step       (a) one optimiser step on fixed gradient rows: install + clip_grad_norm_ + torch Adam + two pack() against adam_step
             (eager, with the binding's argument checks on the host; and sixteen of them captured: the two launches' device time)
  update     (b) a whole update(), epochs = 4, minibatches = 4: the default path eager against device_step=True captured (one graph replay)
Per path and block: host wall clock to a final synchronise and device time between two events (ms per step / update); and once per path
the GPU activities of one call as torch's profiler sees them (kernels, copies, fills; the captured update's are counted on its eager
form; null where the profiler gives none) and the peak
allocation beyond what is held.  --ratios: the accuracy table tests/test_hip_adam_step.py writes with BSX_ADAM_RATIOS_OUT (error against
the float64 restatement over torch's own, mean / max per network and quantity), copied into the result.

    python tools/bench_ppo_update.py --shuffle [--blocks 7] [--out profiles/ppo_shuffle.json]

measures what shuffled minibatches cost (PPOLearner(shuffle=True): one bsx_minibatch_gather per optimiser step), at the two sizes of --adam:
  update     the captured update(), epochs = 4, minibatches = 4, with shuffle=False and shuffle=True: two learners on one rollout, as
             ALTERNATING blocks in one process (device events; the unshuffled learner of the same tree and run is the reference)
  gather     bsx_minibatch_gather alone: the sixteen gathers of one update captured as one graph, device time per gather, and the bytes it
             moves (every field read once and written once, the index written) over that time"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((32, 65536, 1), (8, 65536, 4))          # (T, E, n)
CLIP, VCLIP, TAU, C_V, C_E = 0.2, 0.2, 0.7, 0.5, 0.01
HEAD_BYTES, GAE_BYTES = 86, 19
LOG_2PI = math.log(2.0 * math.pi)


def torch_loss(torch, kind, y, v, act, logp_old, adv, ret, w, v_old, log_std):
    if kind == "categorical":
        lp = torch.log_softmax(y / TAU, dim=-1)
        logp = lp.gather(-1, act.unsqueeze(-1)).squeeze(-1)
        ent = -(lp.exp() * lp).sum(-1)
    else:
        z = (act[..., :3] - y[..., :3]) * torch.exp(-log_std)
        logp = (-0.5 * z * z - log_std).sum(-1) - 1.5 * LOG_2PI
        ent = (log_std + 0.5 * (1.0 + LOG_2PI)).sum(-1).expand_as(logp)
    ratio = torch.exp(logp - logp_old)
    surr = torch.minimum(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
    vc = v_old + (v - v_old).clamp(-VCLIP, VCLIP)
    lv = 0.5 * torch.maximum((v - ret) ** 2, (vc - ret) ** 2)
    return (-(surr * w).sum() + C_V * (lv * w).sum() - C_E * (ent * w).sum()) / w.sum()


ADAM_SIZES = ((32, 65536, 1), (32, 4096, 1))     # (T, E, n)


def adam_pairs(args):
    """--adam: the two A/B pairs of the optimiser step -> the result dict."""
    import time
    import torch
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd.learner import PPOLearner, adam_step
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor

    def block(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps, e0.elapsed_time(e1) / reps

    def stats(x):
        m = statistics.median(x)
        return dict(median_ms=round(m, 4), min_ms=round(min(x), 4), max_ms=round(max(x), 4), spread=round((max(x) - min(x)) / m, 4))

    def gpu_activities(step):
        """Kernels, copies and fills one call puts on the GPU, counted by torch's profiler; None if it records no device activity."""
        try:
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA")) or None
        except Exception as exc:                                          # a build without device tracing: the count is left out
            print(f"[bench_ppo_update] no launch count: {exc}", file=sys.stderr)
            return None

    def peak_of(step):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    def pair(slow, fast, slow_reps, fast_reps, count_fast=None):
        """count_fast: the eager form of a captured `fast` (the profiler does not always see the kernels of a graph replay)."""
        for step in (slow, fast, slow, fast):
            step()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.blocks):
            a.append(block(slow, slow_reps))
            b.append(block(fast, fast_reps))
        out = {}
        for name, x, step, count in (("torch", a, slow, slow), ("device", b, fast, count_fast or fast)):
            out[name] = dict(host_wall=stats([w for w, _ in x]), device_events=stats([d for _, d in x]), gpu_activities=gpu_activities(count),
                             peak_bytes=peak_of(step))
        for key in ("host_wall", "device_events"):
            t, f = out["torch"][key], out["device"][key]
            out[f"torch_over_device_{key}"] = round(t["median_ms"] / f["median_ms"], 2)
            out[f"device_faster_beyond_spread_{key}"] = bool(f["max_ms"] < t["min_ms"])
        return out

    torch.manual_seed(0)
    mgn, epochs, minibatches = 0.5, 4, 4
    result = dict(command=f"python tools/bench_ppo_update.py --adam --blocks {args.blocks}", device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  max_grad_norm=mgn, epochs=epochs, minibatches=minibatches, sizes=[])
    for T, E, n in ADAM_SIZES:
        A, D = 2 * n, 3 * n + 2
        actor, critic = StackedActor(A, D, 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
        with torch.no_grad():
            actor.w3.mul_(50.0); critic.w3.mul_(50.0)
        env = bsx.parallel_env(n_agents=n, n_envs=E, seed=1, auto_reset=True, device="cuda")
        env.reset()
        ro = PolicyRollout(env, actor, T, seed=3, sample="categorical", temperature=TAU, value_actor=critic, gae=dict(gamma=0.99, lam=0.95), chains=1)
        ro.start(); ro.capture()
        ro.run(); ro.run()
        torch.cuda.synchronize()
        kw = dict(clip=CLIP, c_v=C_V, c_e=C_E, vclip=VCLIP, epochs=epochs, minibatches=minibatches, max_grad_norm=mgn)
        plain, device = PPOLearner(ro, **kw), PPOLearner(ro, device_step=True, **kw)
        row_a, row_v, _, _ = (r.clone() if r is not None else None for r in device.minibatch_grads(0, T // minibatches, pack=False))
        blob_a, blob_v = torch.empty_like(ro.fused.weights), torch.empty_like(ro._value_w)

        def torch_step():
            plain.install(row_a, row_v, None)
            torch.nn.utils.clip_grad_norm_(plain.params, mgn)
            plain.optimizer.step()
            actor.pack(out=blob_a)
            critic.pack(out=blob_v)

        def device_step():
            adam_step([actor, critic], [row_a, row_v], [device.adam_a, device.adam_v], [device._blob_a, device._blob_v], device.hyper,
                      device.step_count, stats=device.step_stats[0], workspace=device._adam_ws)
        entry = dict(n=n, ticks=T, games=E, rows_per_minibatch=T // minibatches * E, step=pair(torch_step, device_step, 8, 64))
        # the step's own device time: the eager call above is bound by the binding's argument checks on the host
        sixteen = torch.cuda.CUDAGraph()
        with torch.cuda.graph(sixteen):
            for _ in range(16):
                device_step()
        sixteen.replay()
        entry["step"]["device_captured_ms_per_step"] = stats([block(sixteen.replay, 8)[1] / 16 for _ in range(args.blocks)])
        del sixteen
        device.sync()
        eager = PPOLearner(ro, device_step=True, **kw)
        eager.update()
        device.sync()
        device.capture()
        entry["update"] = pair(plain.update, device.update, 1, 1, count_fast=eager.update)
        entry["update"]["optimiser_steps"] = epochs * minibatches
        result["sizes"].append(entry)
        del ro, plain, device, env, actor, critic
        torch.cuda.empty_cache()
    if args.ratios:
        result["error_over_torch_float32_mean_max"] = [json.loads(line) for line in open(args.ratios) if line.strip()]
    return result


def shuffle_pairs(args):
    """--shuffle: the captured update with and without shuffled minibatches, and the gather alone -> the result dict."""
    import torch
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd.learner import GATHER_ROWS, PPOLearner
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor

    def block(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def stats(x):
        m = statistics.median(x)
        return dict(median_ms=round(m, 4), min_ms=round(min(x), 4), max_ms=round(max(x), 4), spread=round((max(x) - min(x)) / m, 4))

    torch.manual_seed(0)
    mgn, epochs, minibatches = 0.5, 4, 4
    result = dict(command=f"python tools/bench_ppo_update.py --shuffle --blocks {args.blocks}", device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  max_grad_norm=mgn, epochs=epochs, minibatches=minibatches, rows_per_workgroup=GATHER_ROWS, sizes=[])
    for T, E, n in ADAM_SIZES:
        A, D = 2 * n, 3 * n + 2
        actor, critic = StackedActor(A, D, 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
        with torch.no_grad():
            actor.w3.mul_(50.0); critic.w3.mul_(50.0)
        env = bsx.parallel_env(n_agents=n, n_envs=E, seed=1, auto_reset=True, device="cuda")
        env.reset()
        ro = PolicyRollout(env, actor, T, seed=3, sample="categorical", temperature=TAU, value_actor=critic, gae=dict(gamma=0.99, lam=0.95), chains=1)
        ro.start(); ro.capture()
        ro.run(); ro.run()
        torch.cuda.synchronize()
        kw = dict(clip=CLIP, c_v=C_V, c_e=C_E, vclip=VCLIP, epochs=epochs, minibatches=minibatches, max_grad_norm=mgn, device_step=True)
        plain, mixed = PPOLearner(ro, **kw).capture(), PPOLearner(ro, shuffle=True, **kw).capture()
        for step in (plain.update, mixed.update, plain.update, mixed.update):
            step()
        a, b = [], []
        for _ in range(args.blocks):
            a.append(block(plain.update, 4))
            b.append(block(mixed.update, 4))
        t, f = stats(a), stats(b)
        entry = dict(n=n, ticks=T, games=E, rows=T * E, rows_per_minibatch=T * E // minibatches,
                     update=dict(unshuffled=t, shuffled=f, shuffled_over_unshuffled=round(f["median_ms"] / t["median_ms"], 4),
                                 difference_beyond_the_spreads=bool(f["min_ms"] > t["max_ms"])))
        # the gather alone: the sixteen gathers of one update as one graph (an eager call is bound by the binding's checks on the host)
        sixteen = torch.cuda.CUDAGraph()
        with torch.cuda.graph(sixteen):
            for i in range(epochs * minibatches):
                mixed._gather(i)                                    # (the gather only: not the five calls after it)
        sixteen.replay()
        g = stats([block(sixteen.replay, 8) / (epochs * minibatches) for _ in range(args.blocks)])
        row_bytes = 2 * (A * (D + 4 + 4) * 4 + A) + 8               # seven fields read and written, the index written
        entry["gather"] = dict(g, bytes_per_row=row_bytes, gb_per_s=round(row_bytes * (T * E // minibatches) / (g["median_ms"] * 1e-3) / 1e9, 1),
                               share_of_the_unshuffled_update=round(epochs * minibatches * g["median_ms"] / t["median_ms"], 4))
        result["sizes"].append(entry)
        del sixteen, plain, mixed, ro, env, actor, critic
        torch.cuda.empty_cache()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--adam", action="store_true", help="measure the optimiser step (adam_step) instead: profiles/adam_step.json")
    ap.add_argument("--shuffle", action="store_true", help="measure shuffled minibatches (PPOLearner(shuffle=True)) instead: profiles/ppo_shuffle.json")
    ap.add_argument("--ratios", default=None, help="with --adam: the accuracy table written by tests/test_hip_adam_step.py")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ppo_shuffle.json" if args.shuffle else "adam_step.json" if args.adam else "ppo_update.json")
    if args.adam or args.shuffle:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_ppo_update.py measures on the GPU: none found")
        result = shuffle_pairs(args) if args.shuffle else adam_pairs(args)
        print(json.dumps(result))
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
        return
    import torch
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import advantage
    from deep_rl_battlespace_amd.learner import PARAMS, PPOLearner, ppo_head, ppo_head_workspace_bytes
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppo_update.py measures on the GPU: none found")

    def block(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def stats(x):
        m = statistics.median(x)
        return dict(median_ms=round(m, 4), min_ms=round(min(x), 4), max_ms=round(max(x), 4), spread=round((max(x) - min(x)) / m, 4))

    def alternate(slow, fast, slow_reps, fast_reps):
        for step in (slow, fast, slow, fast):                            # warm-up of both paths at this shape
            step()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.blocks):
            a.append(block(slow, slow_reps))
            b.append(block(fast, fast_reps))
        t, f = stats(a), stats(b)
        return dict(torch_autograd=t, fused=f, torch_over_fused=round(t["median_ms"] / f["median_ms"], 2),
                    fused_not_slower_beyond_the_spreads=bool(f["median_ms"] <= t["median_ms"] + (t["max_ms"] - t["min_ms"]) + (f["max_ms"] - f["min_ms"])),
                    fused_faster_beyond_spread=bool(f["max_ms"] < t["min_ms"]))

    def peak_of(step):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    torch.manual_seed(0)
    result = dict(command=f"python tools/bench_ppo_update.py --blocks {args.blocks}", device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  clip=CLIP, vclip=VCLIP, temperature=TAU, c_v=C_V, c_e=C_E, sizes=[])
    for T, E, n in SIZES:
        A, D, R = 2 * n, 3 * n + 2, T * E
        entry = dict(rows=R, n=n, agents=A, ticks=T, games=E, head={}, minibatch={})
        # ---- the loss head alone, on synthetic records of a policy a step away from the one that played
        for kind in ("categorical", "gaussian"):
            f32 = lambda *s: torch.randn(s, device="cuda")                # noqa: E731
            y_old, adv, ret, v_old = torch.tanh(f32(R, A, 4)), f32(R, A), f32(R, A), f32(R, A)
            y, v = torch.tanh(torch.atanh(y_old * 0.999) + 0.1 * f32(R, A, 4)), v_old + 0.3 * f32(R, A)
            mask = (torch.rand((R, A), device="cuda") < 0.8).to(torch.uint8)
            log_std = (torch.rand((A, 3), device="cuda") - 1.0) if kind == "gaussian" else None
            if kind == "categorical":
                rec = y_old / TAU - torch.log(-torch.log(torch.rand((R, A, 4), device="cuda").clamp_(1e-20, 1.0 - 1e-7)))
                act = rec.argmax(-1)
                logp_old = torch.log_softmax(y_old / TAU, -1).gather(-1, act.unsqueeze(-1)).squeeze(-1)
            else:
                y_old[..., 3], y[..., 3] = 0.0, 0.0
                rec = torch.zeros((R, A, 4), device="cuda")
                rec[..., :3] = y_old[..., :3] + torch.exp(log_std) * f32(R, A, 3)
                act = rec
                z = (rec[..., :3] - y_old[..., :3]) * torch.exp(-log_std)
                logp_old = (-0.5 * z * z - log_std).sum(-1) - 1.5 * LOG_2PI
            w = mask.float()
            out = (torch.empty_like(y), torch.empty_like(y), torch.empty((A, 3), device="cuda") if log_std is not None else None,
                   torch.empty(8, dtype=torch.float64, device="cuda"))
            ws = torch.empty(ppo_head_workspace_bytes(R, A) // 8, dtype=torch.int64, device="cuda")
            kw = dict(temperature=TAU) if kind == "categorical" else dict(log_std=log_std)
            yl, vl = y.clone().requires_grad_(), v.clone().requires_grad_()
            ll = log_std.clone().requires_grad_() if log_std is not None else None

            def fused_head():
                ppo_head(kind, y, v, rec, logp_old, adv, ret, mask, clip=CLIP, c_v=C_V, c_e=C_E, v_old=v_old, vclip=VCLIP, out=out, workspace=ws, **kw)

            def torch_head():
                yl.grad, vl.grad = None, None
                if ll is not None:
                    ll.grad = None
                torch_loss(torch, kind, yl, vl, act, logp_old, adv, ret, w, v_old, ll).backward()
            h = alternate(torch_head, fused_head, 4, 32)
            h["peak_bytes_torch"], h["peak_bytes_fused"] = peak_of(torch_head), peak_of(fused_head)
            # both paths computed the same gradient, each in float32: the elements further apart than 1e-5 of the largest gradient (a row
            # whose ratio sits within rounding of a clip boundary takes another branch in one of them: its whole gradient moves)
            h["elements_apart_beyond_1e-5_of_max_gradient"] = int(((out[0] - yl.grad).abs() > 1e-5 * yl.grad.abs().max()).sum())
            h["fused_bytes_per_element"] = HEAD_BYTES
            h["fused_gb_per_s"] = round(HEAD_BYTES * R * A / (h["fused"]["median_ms"] * 1e-3) / 1e9, 1)
            entry["head"][kind] = h
            del y_old, y, v, adv, ret, v_old, mask, rec, act, logp_old, w, out, ws, yl, vl
            torch.cuda.empty_cache()
        # ---- a whole minibatch over a real rollout's records (categorical head), and bsx_gae's bandwidth on those records
        actor, critic = StackedActor(A, D, 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
        with torch.no_grad():
            actor.w3.mul_(50.0); critic.w3.mul_(50.0)
        env = bsx.parallel_env(n_agents=n, n_envs=E, seed=1, auto_reset=True, device="cuda")
        env.reset()
        ro = PolicyRollout(env, actor, T, seed=3, sample="categorical", temperature=TAU, value_actor=critic, gae=dict(gamma=0.99, lam=0.95), chains=1)
        ro.start(); ro.capture()
        ro.run(); ro.run()
        torch.cuda.synchronize()
        learner = PPOLearner(ro, clip=CLIP, c_v=C_V, c_e=C_E, vclip=VCLIP, epochs=1, minibatches=1)
        obs = ro.obs[:T].view(R, A, D)
        act, flat = ro.scores.argmax(-1).view(R, A), (lambda x: x.view(R, A))
        w = ro.mask.view(R, A).float()

        def fused_minibatch():
            learner.minibatch_grads(0, T)

        def torch_minibatch():
            for net in (actor, critic):
                for k in PARAMS:
                    getattr(net, k).grad = None
            torch_loss(torch, "categorical", actor(obs), critic(obs, squash=False)[..., 0], act, flat(ro.logp), flat(ro.adv), flat(ro.ret), w,
                       flat(ro.value), None).backward()
        m = alternate(torch_minibatch, fused_minibatch, 2, 8)
        m["peak_bytes_torch"], m["peak_bytes_fused"] = peak_of(torch_minibatch), peak_of(fused_minibatch)
        m["masked_share_of_rows"] = round(float(w.mean()), 4)
        entry["minibatch"]["categorical"] = m
        done_prev = torch.zeros((E, A), dtype=torch.uint8, device="cuda")
        gae_out = (torch.empty_like(ro.adv), torch.empty_like(ro.ret), torch.empty_like(ro._mask))

        def gae_step():
            advantage.gae(ro.rew, ro.value, ro.last_value, ro._done, ro.env_done, done_prev, 0.99, 0.95, out=gae_out)
        gae_step()
        g = stats([block(gae_step, 32) for _ in range(args.blocks)])
        entry["bsx_gae"] = dict(g, bytes_per_element=GAE_BYTES, gb_per_s=round(GAE_BYTES * R * A / (g["median_ms"] * 1e-3) / 1e9, 1))
        result["sizes"].append(entry)
        del ro, learner, env, obs, act, w, actor, critic, gae_out
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
