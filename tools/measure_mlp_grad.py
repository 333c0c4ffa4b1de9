#!/usr/bin/env python3
"""Measure the cases of tests/test_hip_mlp_grad.py on the card and write the accuracy part of profiles/mlp_input_grad.json.

    python tools/measure_mlp_grad.py [--out profiles/mlp_input_grad.json]

Per case of tests/mlp_grad_util.py CASES (and for the DDPG step), against float64 autograd on the CPU, with e_t = torch float32 autograd on
the CPU (the yardstick):
  kernel             mean(e_k) / mean(e_t), max(e_k) / max(e_t), max(e_k) / max|gradient| of the ten parameter tensors and of x
  yardstick_spread   how far the yardstick itself moves under an equivalent float32 evaluation, [max ratio, mean ratio], the larger of
                     a / b and b / a:  torch_gpu = torch float32 autograd on the GPU against the same on the CPU;  unit_permutation = the
                     same network with its hidden units in another order, 8 orders, on the CPU (mlp_grad_util.unit_permutation_spread);
                     row_permutation = the rows in another order, 8 orders, on the CPU (mlp_grad_util.row_permutation_spread)
  factors            the project's (2, 4) and the exceptions mlp_grad_util.exceptions_from derives from the LARGEST of the three spreads:
                     per case and tensor, and for b3 one pair for every case from its largest spread over the cases (the project's
                     treatment of b3, profiles/actor_grad_float64.json).  No kernel output enters them.
A bound that is missed is recorded (`within: false`), never widened.  The `timing` part of the file belongs to tools/bench_mlp_grad.py
and is kept."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_input_grad.json"))
    args = ap.parse_args()
    import torch
    import actor_ref_util as R
    import mlp_grad_util as M
    import yardstick_util as Y
    from deep_rl_battlespace_amd.learner import fused_mlp
    if not torch.cuda.is_available():
        raise SystemExit("measure_mlp_grad.py measures on the GPU: none found")

    def to_gpu(net):
        a = R._new(net.n_actors, net.obs_len, net.n_actions, device="cuda")
        with torch.no_grad():
            for k in M.PARAMS:
                getattr(a, k).copy_(getattr(net, k).detach())
        return a

    def gpu_grads(net_cpu, x_cpu, go, squash, fused):
        net, x = to_gpu(net_cpu), x_cpu.to("cuda").requires_grad_()
        y = fused_mlp(net, x, squash=squash) if fused else net(x, squash=squash)
        (y * go.to("cuda")).sum().backward()
        torch.cuda.synchronize()
        out = {k: getattr(net, k).grad.double().cpu().numpy() for k in M.PARAMS}
        out["x"] = x.grad.double().cpu().numpy()
        return out

    def spread(ga, g32, g64, names):
        return {k: [round(v[0], 2), round(v[1], 2)] for k, v in M.spread(g64, g32, [ga], names).items()}

    def ratios(got, g64, g32, names=M.TENSORS):
        """{name: (mean(e_k) / mean(e_t), max(e_k) / max(e_t), max(e_k) / max|g64|)}"""
        return {k: (*Y.error_ratios(got[k], g64[k], g32[k]), Y.errors(got[k], g64[k])[1] / max(float(abs(g64[k]).max()), 1e-300)) for k in names}

    def figures(r, factor_of, names):
        return {k: dict(mean_ratio=round(r[k][0], 3), max_ratio=round(r[k][1], 3), max_error_over_max_gradient=float("%.3g" % r[k][2]),
                        within=Y.within(r[k][:2], factor_of(k))) for k in names}

    kernel, sp_gpu, sp_unit, sp_row, raw = {}, {}, {}, {}, {}
    for case in M.CASES:
        cid = M.case_id(case)
        net, x, go, g64, g32, _ = M.reference(case)
        sp_gpu[cid] = spread(gpu_grads(net, x, go, case[3], False), g32, g64, M.TENSORS)
        sp_unit[cid] = {k: [round(v[0], 2), round(v[1], 2)] for k, v in M.unit_permutation_spread(case, 8).items()}
        sp_row[cid] = {k: [round(v[0], 2), round(v[1], 2)] for k, v in M.row_permutation_spread(case, 8).items()}
        raw[cid] = ratios(gpu_grads(net, x, go, case[3], True), g64, g32)
    exceptions = M.exceptions_from(dict(torch_gpu=sp_gpu, unit_permutation=sp_unit, row_permutation=sp_row))
    for case in M.CASES:
        cid = M.case_id(case)
        kernel[cid] = figures(raw[cid], Y.factor_of(exceptions.get(cid, {}), exceptions.get("*", {})), M.TENSORS)
        print(cid, "largest kernel ratios", max(v["mean_ratio"] for v in kernel[cid].values()), max(v["max_ratio"] for v in kernel[cid].values()),
              "missed:", [k for k, v in kernel[cid].items() if not v["within"]], flush=True)
    # the DDPG step: the actor's and the critic's ten tensors, (2, 4) but for b3's pair
    dd = M.ddpg_case()
    a64, c64 = M.ddpg_grads(*dd[:6], torch.float64)
    a32, c32 = M.ddpg_grads(*dd[:6], torch.float32)
    at, ct = M.ddpg_grads(*dd[:6], torch.float32, "cuda")
    af, cf = M.ddpg_grads(*dd[:6], torch.float32, "cuda", lambda net, x, squash: fused_mlp(net, x, squash=squash))
    for name, got, t, g64, g32 in (("ddpg-actor", af, at, a64, a32), ("ddpg-critic", cf, ct, c64, c32)):
        sp_gpu[name] = spread(t, g32, g64, M.PARAMS)
        kernel[name] = figures(ratios(got, g64, g32, M.PARAMS), Y.factor_of({}, exceptions.get("*", {})), M.PARAMS)
        print(name, "largest kernel ratios", max(v["mean_ratio"] for v in kernel[name].values()), max(v["max_ratio"] for v in kernel[name].values()), flush=True)
    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result = dict(what="Accuracy of bsx_mlp_grad (parameter row and grad_x) on the cases of tests/test_hip_mlp_grad.py, and the timings of "
                       "tools/bench_mlp_grad.py.  Bound: per tensor, mean(e_k) <= fm mean(e_t) and max(e_k) <= fx max(e_t), e_k = |kernel - float64 "
                       "autograd|, e_t = |torch float32 autograd on the CPU - float64 autograd| (tests/mlp_grad_util.py).",
                  accuracy_command="python tools/measure_mlp_grad.py", device=torch.cuda.get_device_name(0),
                  yardstick_spread=dict(what="[max ratio, mean ratio] by which max(e_t) and mean(e_t) move under an equivalent float32 evaluation of "
                                             "the yardstick: torch float32 autograd on the GPU, the hidden units in 8 other orders on the CPU, the rows in 8 other orders "
                                             "on the CPU (seeds 4000 .. 4007, as profiles/actor_grad_float64.json)",
                                        torch_gpu=sp_gpu, unit_permutation=sp_unit, row_permutation=sp_row),
                  factors=dict(what="[fm, fx].  The project's (2, 4) for every case and tensor but the exceptions: where one of the three recorded "
                                    "spreads of the yardstick itself reaches 2 on the mean or 4 on the max, twice the largest recorded spread "
                                    "(mlp_grad_util.exceptions_from).  These are the one-row cases, where a tensor is a single draw of rounding "
                                    "errors and not a sum over rows (per case and tensor), and b3 (under '*': every case, as in "
                                    "profiles/actor_grad_float64.json): it has one value per agent and output, a sum of grad_out over the "
                                    "rows whose float32 error is that sum's order and nothing else, and its yardstick moves by up to the "
                                    "recorded spread when the rows are merely reordered.  From the float32 reference's own behaviour; no kernel output entered them.",
                               default=[M.FM, M.FX], exceptions=exceptions),
                  kernel=kernel)
    if "timing" in old:
        result["timing"] = old["timing"]
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
