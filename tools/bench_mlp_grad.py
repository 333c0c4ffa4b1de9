#!/usr/bin/env python3
"""The backward of a Q critic with the gradient to its input: bsx_mlp_grad with grad_x, bsx_mlp_grad without it, and torch autograd of
StackedActor.forward with x.requires_grad (what a DDPG learner on this project had before), on the same tensors, in one process on one GPU.

    python tools/bench_mlp_grad.py [--blocks 7] [--out profiles/mlp_input_grad.json]

Per shape the three paths are timed with device events in ALTERNATING blocks (torch, without, with, torch, ...) after a warm-up of all
three; a block is a few back-to-back calls between two events.  The two kernel paths are learner.mlp_grad on a packed blob: the
backward alone (forward recomputed in the kernel), grad_out copied into its 4-column buffer.  The torch path is forward AND backward
of (y * go).sum() into the ten parameters' .grad and x.grad: autograd has no backward without its forward's saved activations, so this is
the step a user ran, not the backward's share of it.  Reported per path: the median, minimum and maximum block (ms per call), the spread
(max - min) / median; the extra time of grad_x over the plain backward; torch over the path with grad_x.  Also, per shape, the ratios
mean(e_k) / mean(e_t), max(e_k) / max(e_t) of grad_x against float64 autograd on the first 4 096 rows, e_t from torch float32 on the
CPU (the bound of tests/test_hip_mlp_grad.py at the size that is timed; the rows are random and ReLU kinks are NOT left out here, so a row
whose hidden unit flips between float32 and float64 shows in max_error_over_max_gradient -- in the kernel and in the yardstick alike).
Shapes (R, A, D): 524 288 x 2 x 9 (the 1v1 Q critic) and 131 072 x 4 x 24 (the reference's 2v2 critic).  One JSON line on stdout, also
written with the command as the `timing` part of --out (the rest of that file is tools/measure_mlp_grad.py's and is kept)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((524288, 2, 9), (131072, 4, 24))
CHECK_ROWS = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_input_grad.json"))
    args = ap.parse_args()
    import torch
    import deep_rl_battlespace_amd  # noqa: F401
    from deep_rl_battlespace_amd.learner import PARAMS, mlp_grad
    from deep_rl_battlespace_amd.rollout import StackedActor
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_grad.py measures on the GPU: none found")
    torch.manual_seed(0)
    result = dict(command="python tools/bench_mlp_grad.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), blocks=args.blocks,
                  what="ms per call; with_grad_x / without_grad_x: learner.mlp_grad (the backward alone); torch_autograd: forward + backward "
                       "of StackedActor.forward with x.requires_grad", shapes=[])
    for R, A, D in SHAPES:
        net = StackedActor(A, D, 1, device="cuda")
        with torch.no_grad():
            net.w3.mul_(100.0)
        x = torch.rand((R, A, D), device="cuda") * 2 - 1
        go = torch.randn((R, A, 1), device="cuda")
        blob = net.pack()

        def step(path):
            if path == "torch_autograd":
                for k in PARAMS:
                    getattr(net, k).grad = None
                xx = x.detach().requires_grad_()
                (net(xx, squash=False) * go).sum().backward()
            else:
                mlp_grad(net, blob, x, go, squash=False, input_grad=path == "with_grad_x")

        def block(path, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                step(path)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps
        paths = (("torch_autograd", 4), ("without_grad_x", 16), ("with_grad_x", 16))
        for _ in range(2):                                           # warm-up of the three paths at this shape
            for path, _reps in paths:
                step(path)
        torch.cuda.synchronize()
        times = {path: [] for path, _ in paths}
        for _ in range(args.blocks):
            for path, reps in paths:
                times[path].append(block(path, reps))

        def stats(t):
            m = statistics.median(t)
            return dict(median_ms=round(m, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), spread=round((max(t) - min(t)) / m, 4))
        s = {path: stats(t) for path, t in times.items()}
        # grad_x at this size against float64, on the first rows (the rows are independent: a prefix is a fair sample)
        _, gx = mlp_grad(net, blob, x, go, squash=False)
        torch.cuda.synchronize()
        got = gx[:CHECK_ROWS].double().cpu()
        ref = {}
        for dt in (torch.float64, torch.float32):
            c = StackedActor(A, D, 1, dtype=dt)
            with torch.no_grad():
                for k in PARAMS:
                    getattr(c, k).copy_(getattr(net, k).detach().cpu().to(dt))
            xx = x[:CHECK_ROWS].detach().cpu().to(dt).requires_grad_()
            (c(xx, squash=False) * go[:CHECK_ROWS].cpu().to(dt)).sum().backward()
            ref[dt] = xx.grad.double()
        ek, et = (got - ref[torch.float64]).abs(), (ref[torch.float32] - ref[torch.float64]).abs()
        result["shapes"].append(dict(rows=R, agents=A, inputs=D, **s,
                                     grad_x_extra_ms=round(s["with_grad_x"]["median_ms"] - s["without_grad_x"]["median_ms"], 4),
                                     with_over_without=round(s["with_grad_x"]["median_ms"] / s["without_grad_x"]["median_ms"], 3),
                                     torch_over_with_grad_x=round(s["torch_autograd"]["median_ms"] / s["with_grad_x"]["median_ms"], 2),
                                     grad_x_against_float64=dict(rows=CHECK_ROWS, mean_ratio=round(float(ek.mean() / et.mean()), 3),
                                                                 max_ratio=round(float(ek.max() / et.max()), 3),
                                                                 max_error_over_max_gradient=float(ek.max() / ref[torch.float64].abs().max()))))
        del x, go, net, gx
        torch.cuda.empty_cache()
    print(json.dumps(result))
    whole = json.load(open(args.out)) if os.path.exists(args.out) else {}     # the accuracy part belongs to tools/measure_mlp_grad.py
    whole["timing"] = result
    with open(args.out, "w") as fh:
        fh.write(json.dumps(whole, indent=1) + "\n")


if __name__ == "__main__":
    main()
