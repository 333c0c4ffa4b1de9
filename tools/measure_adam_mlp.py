#!/usr/bin/env python3
"""Time the free-width optimiser step with Polyak targets (learner.mlp_adam_step) on the card and write profiles/adam_step_mlp.json.

    python tools/measure_adam_mlp.py [--out profiles/adam_step_mlp.json] [--ratios FILE] [--parent-lib LIB] [--runs 4]

Per size -- (A, D, n_actions) = (3, 9, 1), (4, 24, 1) and (32, 64, 1) with two networks -- by HIP events, in `--runs` ALTERNATING runs (the order reversed in every second one) of
  with_targets     one mlp_adam_step with a target on every network
  without_targets  the same call without targets
  torch            the composition it replaces: clip_grad_norm_ + Adam.step() + the Polyak update (torch._foreach_mul_ / _foreach_add_)
                   + pack() of every network and of every target
The two device calls are timed twice: as a captured graph of CALLS calls replayed back to back (the device's time per call: what a
captured learner pays) and as eager calls from Python (what an uncaptured one pays: the host's enqueue is part of it).  torch's path is
eager only.  Every run is median / min / max over the runs, in microseconds per call.

--parent-lib: a build of the PARENT commit's library.  bsx_adam_step is then called through the raw C ABI of both libraries on the
same tensors at n = 1 and n = 16 (two networks), graphs of CALLS calls, `--parent-runs` alternating runs in which the two take turns
to go first -- is the older entry as fast behind its new front?
--ratios: the JSON lines tests/test_hip_adam_mlp.py writes with BSX_ADAM_MLP_RATIOS_OUT set; folded in as the accuracy table.
Parts of the output file this run does not measure are kept."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((3, 9, 1, 1), (4, 24, 1, 1), (32, 64, 1, 2))        # A, D, n_actions, networks
CALLS, REPLAYS, EAGER_CALLS = 20, 10, 100


def summary(xs):
    return dict(median_us=round(statistics.median(xs), 2), min_us=round(min(xs), 2), max_us=round(max(xs), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_step_mlp.json"))
    ap.add_argument("--ratios")
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--parent-runs", type=int, default=8)
    args = ap.parse_args()
    import torch
    import adam_case_util as C
    import adam_mlp_util as MU
    import adam_util as U
    from deep_rl_battlespace_amd import _lib, learner
    if not torch.cuda.is_available():
        raise SystemExit("measure_adam_mlp.py measures on the GPU: none found")

    def timed(fn, calls):
        """fn() `calls` times (or replays worth `calls` calls) between two events -> microseconds per call."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / calls

    def graph_of(call):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(CALLS):
                call()
        g.replay()
        torch.cuda.synchronize()
        return lambda: [g.replay() for _ in range(REPLAYS)]

    hp = U.hyper32(lr=3e-4, max_grad_norm=0.5)
    sizes = []
    for A, D, na, nets in SIZES:
        case = C.Case(A, D, (na,) * nets, hp, tau=0.005, seed=300)
        rows, _ = case.draw(torch.Generator().manual_seed(1))
        grads = C.flat_split(case, rows, None)
        yard = C.TorchPath(case, hp, 0.005)
        tnets = [C.clone_net(n) for n in case.nets + case.targets]
        ps, ts = [p for grp in yard.params for p in grp], [t for grp in yard.targets for t in grp]
        for grp, gs in zip(yard.params, grads):
            for p, g in zip(grp, gs):
                p.grad = g.clone()

        def torch_step():
            torch.nn.utils.clip_grad_norm_(ps, hp["max_grad_norm"])
            yard.opt.step()
            with torch.no_grad():
                torch._foreach_mul_(ts, 1.0 - 0.005)
                torch._foreach_add_(ts, [p.detach() for p in ps], alpha=0.005)
            return [n.pack() for n in tnets]

        variants = {"with_targets_graph": (graph_of(lambda: case.run(rows, None)), CALLS * REPLAYS),
                    "without_targets_graph": (graph_of(lambda: case.run(rows, None, with_targets=False)), CALLS * REPLAYS),
                    "with_targets_eager": (lambda: [case.run(rows, None) for _ in range(EAGER_CALLS)], EAGER_CALLS),
                    "without_targets_eager": (lambda: [case.run(rows, None, with_targets=False) for _ in range(EAGER_CALLS)], EAGER_CALLS),
                    "torch_eager": (lambda: [torch_step() for _ in range(EAGER_CALLS)], EAGER_CALLS)}
        for fn, calls in variants.values():                              # every shape of the timed window, warm
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for r in range(args.runs):
            for k, (fn, calls) in (list(variants.items()) if r % 2 == 0 else reversed(list(variants.items()))):
                times[k].append(timed(fn, calls))
        entry = dict(A=A, D=D, n_actions=na, networks=nets, row_floats=learner.grad_floats(D), blob_floats=MU.blob_floats(D),
                     **{k: summary(v) for k, v in times.items()})
        entry["torch_over_with_targets_graph"] = round(entry["torch_eager"]["median_us"] / entry["with_targets_graph"]["median_us"], 1)
        entry["torch_over_with_targets_eager"] = round(entry["torch_eager"]["median_us"] / entry["with_targets_eager"]["median_us"], 1)
        print(json.dumps(entry), flush=True)
        sizes.append(entry)

    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(what="learner.mlp_adam_step (bsx_adam_step_mlp): microseconds per call by HIP events, median / min / max over alternating runs "
                       "-- as a captured graph of calls replayed back to back and as eager calls from Python -- next to the torch "
                       "composition it replaces (clip_grad_norm_ + Adam.step() + foreach Polyak + pack() of networks and targets, eager); and "
                       "the accuracy ratios of tests/test_hip_adam_mlp.py.",
                  command="python tools/measure_adam_mlp.py", device=torch.cuda.get_device_name(0), runs=args.runs,
                  calls_per_graph=CALLS, replays_per_run=REPLAYS, eager_calls_per_run=EAGER_CALLS, sizes=sizes)

    if args.parent_lib:
        libs = {"parent": ctypes.CDLL(args.parent_lib), "tree": ctypes.CDLL(_lib.LIB_PATH)}
        for lib in libs.values():
            lib.bsx_adam_step.restype = ctypes.c_int
            lib.bsx_adam_step.argtypes = _lib.SIGNATURES["bsx_adam_step"][1]
        older = []
        for n in (1, 16):
            A, D = 2 * n, 3 * n + 2
            case = C.Case(A, D, (4, 1), hp, targets=(False, False), seed=300)
            rows, _ = case.draw(torch.Generator().manual_seed(2))
            io = _lib.BsxAdamIo()
            io.nets = 2
            for i, (net, row, st, blob) in enumerate(zip(case.nets, rows, case.states, case.blobs)):
                for q, k in enumerate(U.PARAMS):
                    io.net[i].p[q] = getattr(net, k).data_ptr()
                io.net[i].grad, io.net[i].m, io.net[i].v, io.net[i].blob, io.net[i].n_actions = \
                    row.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), blob.data_ptr(), net.n_actions
            io.hyper, io.step = case.hyper.data_ptr(), case.step.data_ptr()

            def raw(lib):
                rc = lib.bsx_adam_step(ctypes.byref(io), n, case.ws.data_ptr(), case.stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
            # the same bits from both libraries, from one state, before anything is timed
            start = case.bits()
            outs = {}
            for name, lib in libs.items():
                for k, v in case.tensors().items():
                    v.view(start[k].dtype).copy_(start[k])
                raw(lib)
                outs[name] = case.bits()
            same = C.same_bits(outs["parent"], outs["tree"]) == []
            graphs = {name: graph_of(lambda lib=lib: raw(lib)) for name, lib in libs.items()}
            times = {name: [] for name in libs}
            for r in range(args.parent_runs):                            # whichever goes first in a run goes second in the next
                for name, fn in (list(graphs.items()) if r % 2 == 0 else reversed(list(graphs.items()))):
                    times[name].append(timed(fn, CALLS * REPLAYS))
            entry = dict(n=n, A=A, D=D, networks=2, same_bits=same, runs=args.parent_runs, **{k: summary(v) for k, v in times.items()})
            entry["ranges_overlap"] = bool(entry["tree"]["min_us"] <= entry["parent"]["max_us"] and entry["parent"]["min_us"] <= entry["tree"]["max_us"])
            print(json.dumps(entry), flush=True)
            older.append(entry)
        result["bsx_adam_step_parent_against_tree"] = dict(
            what="bsx_adam_step through the raw C ABI of a build of the parent commit and of this tree, on the same tensors: graphs of calls "
                 "replayed back to back, alternating runs, microseconds per call; same_bits: both libraries leave the same output bits from one state",
            sizes=older)

    if args.ratios:
        result["error_over_torch_float32_mean_max"] = [json.loads(line) for line in open(args.ratios) if line.strip()]
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
