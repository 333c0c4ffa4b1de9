"""Regenerates profiles/kernarg_entry_fetch.json from the bench lines and profiler summaries the A/B calls left in <dir>/c1 ... <dir>/c5
(<form>_<workload>_<run>.out = one bench.py line; kt_<form>.json / pmc_<form>.json = tools/pmc_kernel.py's output): per call and workload every
run of every form (us per step() by HIP events) and the medians.  The record of how the table was made, runnable only where those
directories still exist.     python tools/mk_kernarg_entry_fetch.py <dir>"""
import collections
import glob
import json
import os
import re
import statistics
import sys

D = sys.argv[1]


def table(tag, names):
    t = collections.defaultdict(list)
    for f in sorted(glob.glob(f"{D}/{tag}/*.out")):
        m = re.match(r".*/(%s)_(\w+?)_(\d+)\.out" % "|".join(names), f)
        if not m:
            continue
        try:
            d = json.loads(open(f).read().strip().splitlines()[-1])
        except Exception:
            continue
        t[m.group(2)].append((m.group(1), int(m.group(3)), d["roofline"]["avg_launch_us"]))
    out = {}
    for w, v in sorted(t.items()):
        out[w] = {n: [x for nn, _, x in sorted(v, key=lambda r: r[1]) if nn == n] for n in names if any(nn == n for nn, _, _ in v)}
        out[w]["median"] = {n: round(statistics.median(out[w][n]), 3) for n in out[w]}
        out[w]["min_max_spread"] = {n: round(max(out[w][n]) - min(out[w][n]), 3) for n in out[w] if n != "median"}
    return out


def prof(tag, lib):
    o = {}
    for kind in ("kt", "pmc"):
        p = f"{D}/{tag}/{kind}_{lib}.json"
        if os.path.exists(p):
            o["kernel_trace" if kind == "kt" else "pmc"] = json.load(open(p))
    return o


d = {
 "what": "The per-call two-wave 1v1 kernels (csrc/bsx_step_split.h, MANY = 0) and the cold scalar-cache fetches of a launch: kernel arguments and the atan2 table. "
         "us per step() by HIP events (bench.py --gpus 1 --steps 1000 --warmup 50 --repeats 3 --no-cpu-baseline --no-other-workloads --no-live-traffic "
         "[--envs-per-gpu E | --continuous | --action-mix shoot | --n-agents 4]; a run's figure is the median of its 3 blocks); the libraries of the forms alternate "
         "within ONE call on one box (BSX_LIB_PATH), run 1 of every form, then run 2 ...; every run listed in run order; workload keys: c2 = 65 536 x 1v1 (the headline), "
         "s20 = the --steps 20 form, E<games>, cont = continuous actions, shoot = action 1 every tick, n4 = 65 536 x 4v4 (one-wave kernel: untouched code, the control). "
         "Boxes differ by ~0.03 us between calls; compare within a call only.",
 "forms": {
  "parent": "the tree before this change: the first wave's scalar loads of kernarg offsets 0x38 (action kind), 0x40..0x67, 0xb0 are waited for in front of ALL six first vector loads; "
            "the rest of the argument block is fetched next to its use (0x70..0x8f behind the pose rendezvous; 0xb8..0x10f behind the shot); the geometry wave fetches the atan2 table behind the pose rendezvous",
  "i1": "parent + the geometry wave fetches the 20 atan2 coefficients at kernel entry (behind its record load), holds them in 40 SGPRs across the draw and the pose rendezvous and passes them into atan2_pixels_n",
  "i2a": "parent + every StepArgs field the first wave reads pinned in SGPRs (asm volatile \"+s\") at the existing pin: ONE batch of scalar loads at the wave's entry, waited for in front of the first vector loads; no s_load behind the first s_barrier",
  "i2": "as i2a, but the batch is read through the kernarg segment pointer made opaque BEHIND the six first vector loads (which then wait for offset 0x38 only), so that it overlaps the first data miss; no s_load behind the first s_barrier",
  "i12": "i1 + i2",
  "fl": "parent + the first wave's five record and pool loads (envc, envd, plane, pool entries, pool count: addresses from arguments preloaded into SGPRs) issued BEFORE the wait for the kernarg fetch; the action load (address selects on the action kind, offset 0x38) behind it.  THE FORM KEPT",
  "fl2": "fl + the action load without its select on the action kind (an empty call's dummy pointer is the state block, larger than 16 B per agent row): all six loads in front of the wait",
  "fl2p": "fl2 + i2a's pins: the whole argument block in one batch at the wave's entry, waited for behind the six vector loads; no s_load behind the first s_barrier",
  "new": "the committed tree: fl with the ring stride (p.E x A) named behind the first loads as well; rebuilt and measured against the parent in call 4"},
 "call1_items_1_and_2": table("c1", ["parent", "i12", "i1", "i2", "i2a"]),
 "call1_items_1_and_2_steps20": table("c1s", ["parent", "i12", "i1", "i2", "i2a"]),
 "call2_first_loads": table("c2", ["parent", "fl"]),
 "call3_first_loads_forms": table("c3", ["parent", "fl", "fl2", "fl2p"]),
 "call3_first_loads_forms_steps20": table("c3s", ["parent", "fl", "fl2", "fl2p"]),
 "call4_committed_vs_parent_all_regimes": table("c4", ["parent", "new"]),
 "call4_dump_outputs": "bench.py --steps 200 --warmup 20 --dump-outputs with the parent's and the committed library: obs.npy, rew.npy, done.npy identical array for array",
 "call5_profiler": {"what": "rocprofv3 --kernel-trace --stats, and in a run of its own rocprofv3 --pmc SQ_WAVES SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY, of bench.py --steps 300 --warmup 50 --repeats 3 "
                            "(tools/pmc_kernel.py: means per launch over the second half of the launches of bsx_step_split_kernel)",
                    "parent": prof("c5", "parent"), "new": prof("c5", "new")},
 "stamps": "not taken: the in-kernel stamp variant (tools/build_variant.py -DBSX_STAMPS) was not run; the question it was to answer -- whether items 1 and 2 have something to win -- the alternating runs of the built forms answered directly",
 "reading": [
  "issue items 1 and 2 (fetch the atan2 table and the argument block at entry) LOSE in every form built: C2 5.396 -> 5.418 (i1), 5.458 (i2a), 5.480 (i2), 5.522 (i12); on top of the kept form 5.344 -> 5.458 (fl2p). "
  "Spread of a form within a call: 0.005 ... 0.015 us.  The loads the compiler leaves mid-chain do not cost what a cold miss would: every workgroup reads the same argument lines, the lines are in the scalar cache "
  "long before the shot, and holding ~40 more SGPRs from entry costs instructions and schedule.  Items 3 (StepArgs hot-first) and 4 (the one-wave kernels) only serve item 2's batch: not built.",
  "the geometry wave has no room before the pose rendezvous beyond the Philox block (profiles/r06_experiments.json r06h, r06k): 15 more instructions there (i1) cost 0.02 us, whatever they save behind it is hidden under the first wave's bullet pass",
  "what the cold kernarg fetch does cost is its place IN FRONT of the first vector loads: with the five loads that need no kernarg data issued first (fl), C2 5.369 -> 5.291 (call 2), 5.394 -> 5.321 (call 3), 5.395 -> 5.317 (call 4): "
  "-0.075 us = -1.4 %, 5 ... 12 x the parent's min-max spread in each call; --steps 20 form 5.44 -> 5.36",
  "every listed regime gains or is unchanged (call 4, medians): 16 384 games 4.225 -> 4.163, 32 768 4.667 -> 4.553, 98 304 6.410 -> 6.350, 114 688 (DRAW = false) 7.173 -> 7.109, continuous 7.550 -> 7.433, all-shoot 6.802 -> 6.727, 4v4 (untouched one-wave kernel) 20.234 -> 20.227",
  "moving the action load in front of the wait as well (fl2) gives 0.02 us back: kept out",
  "profiler (call 5): kernel time by rocprofv3 --kernel-trace 5 861 -> 5 794 ns per launch; SQ_ACTIVE_INST_ANY 2.053 M both, SQ_WAIT_ANY / SQ_WAVE_CYCLES 61.3 % -> 60.7 % under the counters' own overhead: "
  "no instruction leaves the kernel, one wait moves behind five loads",
  "parity: tests/test_hip_split.py (21) on fl, fl2, fl2p and the committed build; tests/test_hip_entry_fetch.py (20) on the committed build; bench.py --dump-outputs identical to the parent's"]}
json.dump(d, open("profiles/kernarg_entry_fetch.json", "w"), indent=1)
print({k: v.get("median") for k, v in d["call4_committed_vs_parent_all_regimes"].items()})
