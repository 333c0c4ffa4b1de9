// bsx_replay_nstep.hip -- n-step returns for the replay ring (include/battlespace_hip.h: bsx_replay_nstep_*), gfx950.
//
// A rollout's T ticks, preceded by the n - 1 ticks the previous call carried over, are folded into T dense rows
// (obs[u], act[u], sum_j gamma^j rew[u+j], obs[u+m], done_n) that bsx_replay_append stores like any other source: the ring, its
// counter, the prioritised tree and the three learners' heads (given gamma^n) stay as they are.  Two launches, no host round trip:
//   1. fold  -- one workgroup per 256 emitted rows (u, e): a thread per row finds the row's window length m and its skip byte, a
//               thread per (row, agent) folds rew and done, then the tile's obs / obs_next / act words are walked flat as
//               bsx_replay.hip's scatter_field walks them (consecutive lanes load and store consecutive words);
//   2. carry -- the rollout's last n - 1 ticks into the carry (dense), carry_valid = 1.  The fold only reads the carry, this launch
//               only writes it: no launch reads and overwrites the same carry words.
// Built with -ffp-contract=off and an explicit fmaf: every float32 operation is rounded on its own, as tests/nstep_util.py restates.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"
#include "bsx_replay_ring.h"

namespace {

using namespace bsx_ring;        // TPB (threads per workgroup = rows per tile), MAX_ROWS, aligned

struct NstepArgs {
    BsxReplaySource src;          // the rollout record (obs_next unused; skip = env_done before each tick, T + 1 ticks)
    BsxNstepCarry carry;
    float *o_obs, *o_next, *o_act, *o_rew;   // the dense folded source inside the workspace (fold only): [rows][nA][D] twice, [rows][nA][k],
    uint8_t *o_done, *o_skip;                // [rows][nA] twice, [rows]
    int64_t E, rows, CE;          // rows = the launch's rows ((u, e) pairs); CE = (n - 1) * E = the carry's rows
    int T, nA, D, k, n;
    float gamma;
};

// Timeline row v * E + e: below CE a row of the carry (dense), from CE on row (v - (n - 1)) * E + e of the rollout record.
__device__ inline uint8_t before_flag(const NstepArgs& p, int64_t row) {
    return row < p.CE ? p.carry.env_done[row] : p.src.skip[(row - p.CE) * p.src.skip_row];
}

__device__ inline float rew_at(const NstepArgs& p, int64_t row, int a) {
    return row < p.CE ? p.carry.rew[row * p.nA + a] : p.src.rew[(row - p.CE) * p.src.rew_row + int64_t(a) * p.src.rew_col];
}

__device__ inline bool done_at(const NstepArgs& p, int64_t row, int a) {
    return (row < p.CE ? p.carry.done[row * p.nA + a] : p.src.done[(row - p.CE) * p.src.done_row + int64_t(a) * p.src.done_col]) != 0;
}

// bits are copied, never converted: float arrays as the words they are
__device__ inline uint32_t* words(float* p) { return reinterpret_cast<uint32_t*>(p); }
__device__ inline const uint32_t* words(const float* p) { return reinterpret_cast<const uint32_t*>(p); }

// rows r0 .. r0 + cnt - 1 of one field, dense [row][nA][width] at dst: row i <- timeline row row_of(i) -- from the carry (dense, nA * width
// words a row) below CE, else from the record (strides); CARRY = false: a timeline with no carry, the record's rows alone.  Flat over the
// cnt x nA x width words.
template <bool CARRY, typename RowOf>
__device__ inline void copy_field(uint32_t* __restrict__ dst, const uint32_t* __restrict__ dense, const uint32_t* __restrict__ rec, int64_t row_stride,
                                  int64_t col_stride, int nA, int width, int64_t r0, int cnt, int64_t CE, int tid, RowOf row_of) {
    const int W = nA * width;
    for (int j = tid; j < cnt * W; j += TPB) {
        const int i = j / W, rem = j - i * W;
        const int64_t row = row_of(i);
        const int c = rem / width, x = rem - c * width;
        uint32_t v;
        if (CARRY && row < CE) v = dense[row * W + rem];
        else v = rec[(row - CE) * row_stride + int64_t(c) * col_stride + x];
        dst[(r0 + i) * W + rem] = v;
    }
}

__global__ __launch_bounds__(TPB) void bsx_replay_nstep_fold_kernel(const NstepArgs p) {
    __shared__ int s_m[TPB];
    const int tid = threadIdx.x;
    const int64_t r0 = int64_t(blockIdx.x) * TPB;
    const int cnt = int(p.rows - r0 < TPB ? p.rows - r0 : TPB);
    if (tid < cnt) {
        const int64_t r = r0 + tid;                                    // = u * E + e, also the row's place on the timeline
        bool skip = before_flag(p, r) != 0;
        if (r < p.CE) skip = skip || p.carry.valid[r % p.E] == 0;
        int m = p.n;
        for (int j = p.n - 1; j >= 0; --j)                              // the first tick of the window after which the game is over
            if (before_flag(p, r + int64_t(j + 1) * p.E) != 0) m = j + 1;
        s_m[tid] = m;
        p.o_skip[r] = skip ? 1 : 0;
    }
    __syncthreads();
    for (int j = tid; j < cnt * p.nA; j += TPB) {
        const int i = j / p.nA, a = j - i * p.nA, m = s_m[i];
        const int64_t r = r0 + i;
        float R = rew_at(p, r, a), g = 1.0f;
        bool dead = done_at(p, r, a);
        for (int q = 1; q < m; ++q) {
            const int64_t row = r + int64_t(q) * p.E;
            g = g * p.gamma;
            if (!dead) R = fmaf(g, rew_at(p, row, a), R);
            dead = dead || done_at(p, row, a);
        }
        p.o_rew[r * p.nA + a] = R;
        p.o_done[r * p.nA + a] = (dead || m < p.n) ? 1 : 0;
    }
    const BsxReplaySource& s = p.src;
    const uint32_t *c_obs = words(p.carry.obs), *r_obs = words(s.obs);
    const auto cur = [&](int i) { return r0 + i; };
    const auto next = [&](int i) { return r0 + i + s_m[i] * p.E; };
    copy_field<true>(words(p.o_obs), c_obs, r_obs, s.obs_row, s.obs_col, p.nA, p.D, r0, cnt, p.CE, tid, cur);
    copy_field<true>(words(p.o_next), c_obs, r_obs, s.obs_row, s.obs_col, p.nA, p.D, r0, cnt, p.CE, tid, next);
    copy_field<true>(words(p.o_act), words(p.carry.act), words(s.act), s.act_row, s.act_col, p.nA, p.k, r0, cnt, p.CE, tid, cur);
}

// rows r = j * E + e of the carry <- tick T - (n - 1) + j of the record; the flags before those ticks; carry_valid = 1 for every game.
// The launch covers max(n - 1, 1) * E rows so that n = 1 (an empty carry) still sets carry_valid.
__global__ __launch_bounds__(TPB) void bsx_replay_nstep_carry_kernel(const NstepArgs p) {
    const int tid = threadIdx.x;
    const int64_t r0 = int64_t(blockIdx.x) * TPB;
    const int64_t r = r0 + tid;
    if (r < p.E) p.carry.valid[r] = 1;
    if (r0 >= p.CE) return;
    const int cnt = int(p.CE - r0 < TPB ? p.CE - r0 : TPB);
    const BsxReplaySource& s = p.src;
    const int64_t first = int64_t(p.T - (p.n - 1)) * p.E;               // the record's row of carry row 0
    if (tid < cnt) p.carry.env_done[r] = s.skip[(first + r) * s.skip_row] != 0;
    for (int j = tid; j < cnt * p.nA; j += TPB) {
        const int i = j / p.nA, a = j - i * p.nA;
        const int64_t row = first + r0 + i;
        p.carry.rew[(r0 + i) * p.nA + a] = s.rew[row * s.rew_row + int64_t(a) * s.rew_col];
        p.carry.done[(r0 + i) * p.nA + a] = s.done[row * s.done_row + int64_t(a) * s.done_col] != 0;
    }
    // the copies read the record only: a timeline whose carry is empty (CE = 0), so that row first + r0 + i is the record's own
    const auto rec = [&](int i) { return first + r0 + i; };
    copy_field<false>(words(p.carry.obs), nullptr, words(s.obs), s.obs_row, s.obs_col, p.nA, p.D, r0, cnt, 0, tid, rec);
    copy_field<false>(words(p.carry.act), nullptr, words(s.act), s.act_row, s.act_col, p.nA, p.k, r0, cnt, 0, tid, rec);
}

int64_t tiles_of(int64_t rows) { return (rows + TPB - 1) / TPB; }

// What the entry points share, in the order of their refusals: BSX_E_ARG for a size out of range (check_shapes), then for a missing
// pointer or a negative stride of the record or the carry (check_record); record_misaligned is the BSX_E_ALIGN that follows.
int check_shapes(int T, int64_t E, int nA, int D, int k, int n) {
    if (n < 1 || n > BSX_NSTEP_MAX || T < n || T > BSX_MAX_T || E < 1 || E > MAX_ROWS / T) return BSX_E_ARG;
    if (nA < 1 || nA > BSX_MAX_N || D < 1 || D > 3 * BSX_MAX_N + 2 || (k != 3 && k != 4)) return BSX_E_ARG;
    return 0;
}

int check_record(const BsxReplaySource* s, const BsxNstepCarry* c, int n) {
    if (!s || !c || !s->obs || !s->act || !s->rew || !s->done || !s->skip || !c->valid) return BSX_E_ARG;
    if (n > 1 && (!c->obs || !c->act || !c->rew || !c->done || !c->env_done)) return BSX_E_ARG;
    if (s->obs_row < 0 || s->obs_col < 0 || s->act_row < 0 || s->act_col < 0 || s->rew_row < 0 || s->rew_col < 0 || s->done_row < 0 ||
        s->done_col < 0 || s->skip_row < 0) return BSX_E_ARG;
    return 0;
}

bool record_misaligned(const BsxReplaySource* s, const BsxNstepCarry* c) {
    return !aligned(s->obs, 4) || !aligned(s->act, 4) || !aligned(s->rew, 4) || !aligned(c->obs, 4) || !aligned(c->act, 4) || !aligned(c->rew, 4);
}

}  // namespace

extern "C" {

int bsx_replay_nstep_workspace_bytes(int T, int64_t E, int nA, int D, int k, int n, size_t* bytes) {
    if (const int rc = check_shapes(T, E, nA, D, k, n)) return rc;
    if (!bytes) return BSX_E_ARG;
    const size_t rows = size_t(T) * size_t(E);
    *bytes = rows * size_t(nA) * (4 * size_t(2 * D + k + 1) + 1) + rows;
    return 0;
}

int bsx_replay_nstep_fold(const BsxReplaySource* rollout, const BsxNstepCarry* carry, int T, int64_t E, int nA, int D, int k, int n,
                          float gamma, void* workspace, BsxReplaySource* folded, void* stream) {
    if (const int rc = check_shapes(T, E, nA, D, k, n)) return rc;
    if (const int rc = check_record(rollout, carry, n)) return rc;
    if (!(gamma >= 0.0f && gamma <= 1.0f) || !workspace || !folded) return BSX_E_ARG;
    if (record_misaligned(rollout, carry) || !aligned(workspace, 4)) return BSX_E_ALIGN;
    const int64_t rows = int64_t(T) * E, cells = rows * nA;
    float* f = static_cast<float*>(workspace);
    float *o_obs = f, *o_next = f + cells * D, *o_act = f + 2 * cells * D, *o_rew = o_act + cells * k;
    uint8_t *o_done = reinterpret_cast<uint8_t*>(o_rew + cells), *o_skip = o_done + cells;
    *folded = BsxReplaySource{o_obs, int64_t(nA) * D, D, o_next, int64_t(nA) * D, D, o_act, int64_t(nA) * k, k, o_rew, nA, 1, o_done, nA, 1, o_skip, 1};
    NstepArgs a{*rollout, *carry, o_obs, o_next, o_act, o_rew, o_done, o_skip, E, rows, int64_t(n - 1) * E, T, nA, D, k, n, gamma};
    hipLaunchKernelGGL(bsx_replay_nstep_fold_kernel, dim3(unsigned(tiles_of(rows))), dim3(TPB), 0, static_cast<hipStream_t>(stream), a);
    return int(hipGetLastError());
}

int bsx_replay_nstep_carry(const BsxReplaySource* rollout, const BsxNstepCarry* carry, int T, int64_t E, int nA, int D, int k, int n,
                           void* stream) {
    if (const int rc = check_shapes(T, E, nA, D, k, n)) return rc;
    if (const int rc = check_record(rollout, carry, n)) return rc;
    if (record_misaligned(rollout, carry)) return BSX_E_ALIGN;
    const int64_t CE = int64_t(n - 1) * E;
    NstepArgs a{*rollout, *carry, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, E, CE, CE, T, nA, D, k, n, 0.0f};
    hipLaunchKernelGGL(bsx_replay_nstep_carry_kernel, dim3(unsigned(tiles_of(CE > E ? CE : E))), dim3(TPB), 0, static_cast<hipStream_t>(stream), a);
    return int(hipGetLastError());
}

}  // extern "C"
