"""Where every step-kernel launch reads and writes its bullet pools, from the launcher's own arithmetic: a host program built from
include/battlespace_hip.h and csrc/bsx_state.h (step_geometry, the geometry launch_for_n launches; make_layout, wave_blocks) walks every
wave of every launch form over ragged and large batches and checks that the pool it indexes exists.  No GPU: a wave beyond the state
block's pools is a read the device tests cannot see (its pool count reads as 0 and no result changes), so it is checked here."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "battlespace_hip.h"
#include "bsx_state.h"
using namespace bsxk;

static long launches = 0, waves = 0, shown = 0, bad[3] = {0, 0, 0};
static long past_bytes[2049][BSX_MAX_N + 1];   // E <= 2048: the most bytes a first-row load of (E, n) reaches past the block's end
static const char* const FORM[3] = {"one-wave", "two-wave", "rollout"};

// Every wave of `geo` over the games [first, first + count) of a block laid out for E games of n-v-n: (0) its pool index is below the
// layout's pool count, (1) its unconditional first-row load [bent + wblk * POOL_CAP * 8, + 512) ends inside the block, (2) the pool
// count it reads (and, after a multi-tick launch, stores) lies inside the bcnt array.  Pool indices grow with the workgroup, so for the
// many range launches `ends_only` walks the first and the last workgroup only.
static void check(int form, int64_t E, int n, int64_t first, int64_t count, bool ends_only) {
    const StepGeometry geo = step_geometry(form, count, n);
    const Layout L = make_layout(E, n);
    const int64_t NB = wave_blocks(E, n), fb = first / (64 / group_width(n));
    ++launches;
    for (int64_t b = 0; b < geo.groups; ++b) {
        if (ends_only && b == 1 && geo.groups > 2) b = geo.groups - 1;
        for (int w = 0; w < geo.waves; ++w) {
            ++waves;
            const int64_t wblk = fb + b * geo.pools + int64_t(w) * geo.pools / geo.waves;
            const size_t row_end = L.bent + (size_t(wblk) * POOL_CAP + 64) * sizeof(uint2);
            const size_t cnt_end = L.bcnt + size_t(wblk + 1) * sizeof(uint32_t);
            const bool v[3] = {wblk >= NB, row_end > L.total, cnt_end > L.bcnt + size_t(NB) * sizeof(uint32_t)};
            for (int k = 0; k < 3; ++k) {
                if (!v[k]) continue;
                ++bad[k];
                if (shown < 24) {
                    ++shown;
                    printf("VIOLATION %s E=%lld n=%d first=%lld count=%lld: workgroup %lld wave %d -> pool %lld of %lld; ", FORM[form],
                           (long long)E, n, (long long)first, (long long)count, (long long)b, w, (long long)wblk, (long long)NB);
                    if (k == 0) printf("pool index out of range\n");
                    if (k == 1) printf("first row ends %zu bytes past the %zu-byte block\n", row_end - L.total, L.total);
                    if (k == 2) printf("bcnt entry ends %zu bytes past the %lld-entry bcnt array\n",
                                       cnt_end - (L.bcnt + size_t(NB) * sizeof(uint32_t)), (long long)NB);
                }
            }
            if (v[1] && E <= 2048 && long(row_end - L.total) > past_bytes[E][n]) past_bytes[E][n] = long(row_end - L.total);
        }
    }
}

static void sizes(int64_t E) {
    // range launches (bsx_step_*_range): `first` a multiple of 256, any count; at the large sizes the first two and the last 256-game
    // blocks, with counts up to 300 and within 300 of the rest
    const bool big = E > 2048;
    std::vector<int64_t> firsts;
    if (!big) for (int64_t f = 0; f < E; f += 256) firsts.push_back(f);
    else firsts = {0, 256, (E - 512) & ~int64_t(255)};
    for (int n = 1; n <= BSX_MAX_N; ++n) {
        check(FORM_ONE_WAVE, E, n, 0, E, false);
        if (n == 1) check(FORM_TWO_WAVE, E, n, 0, E, false);   // (a superset of the sizes split_applies picks it for)
        if (n <= ROLLOUT_MAX_N) check(FORM_ROLLOUT, E, n, 0, E, false);   // (no range form)
        for (const int64_t first : firsts)
            for (int64_t count = 1; count <= E - first - (first == 0); ++count) {
                if (big && count > 300 && count < E - first - 300) count = E - first - 300;
                check(FORM_ONE_WAVE, E, n, first, count, true);
                if (n == 1) check(FORM_TWO_WAVE, E, n, first, count, true);
            }
    }
}

int main() {
    for (int64_t E = 1; E <= 2048; ++E) sizes(E);
    for (int64_t E : {int64_t(65536), int64_t(114688), int64_t(131072), int64_t(1) << 20}) sizes(E);
    long pairs = 0;
    for (int n = 1; n <= BSX_MAX_N; ++n)
        for (int E = 1; E <= 2048; ++E)
            if (past_bytes[E][n]) {
                if (pairs++ < 40) printf("PAST E=%d n=%d %ld\n", E, n, past_bytes[E][n]);
            }
    printf("SUMMARY launches=%ld waves=%ld pool_index=%ld first_row=%ld bcnt=%ld past_pairs=%ld\n", launches, waves, bad[0], bad[1], bad[2], pairs);
    return (bad[0] || bad[1] || bad[2]) ? 1 : 0;
}
"""


def _build_module():
    spec = importlib.util.spec_from_file_location("_bsx_build", os.path.join(ROOT, "deep-rl-battlespace_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_wave_of_every_launch_indexes_a_pool_of_the_block(tmp_path):
    """Forms and sizes: the one-wave per-call / multi-tick kernels (n = 1 .. 16), the two-wave 1v1 kernels and the fused rollout
    (n = 1 .. 4), at E = 1 .. 2 048 and 65 536, 114 688, 131 072, 2^20 games; range launches at every first multiple of 256 with every
    count (at the large sizes: first = 0, 256 and one block from the end, counts up to 300 and within 300 of the rest).  The fused rollout's
    last workgroup covers 32 games, so a ragged 2v2 ... 4v4 batch starts waves wholly beyond it: wave_blocks must give them pools."""
    B = _build_module()
    src = tmp_path / "footprint.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "footprint"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *B.COMMON, "-I", B.INCLUDE, "-I", B.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    summary = [l for l in r.stdout.splitlines() if l.startswith("SUMMARY")]
    assert len(summary) == 1, r.stdout + r.stderr
    f = dict(kv.split("=") for kv in summary[0].split()[1:])
    assert r.returncode == 0 and f["pool_index"] == f["first_row"] == f["bcnt"] == f["past_pairs"] == "0", r.stdout
    # (the walk covered what it says: every size, every form, the range launches)
    assert int(f["launches"]) > 10_000_000 and int(f["waves"]) > int(f["launches"]), summary
