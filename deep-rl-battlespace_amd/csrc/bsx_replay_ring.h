// bsx_replay_ring.h -- what the two translation units of the replay ring share (bsx_replay.hip: append and the uniform draw;
// bsx_replay_prio.hip: the prioritised draw): the ring's argument checks and the gather of the rows drawn.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"

namespace bsx_ring {

constexpr int TPB = 256;          // threads per workgroup = source rows per tile (append)
constexpr int64_t MAX_ROWS = (int64_t(1) << 31) - 1;

// n rows of one field: out row b0 + i <- ring row s_row[i]; both sides are dense rows of W words.
template <typename T>
__device__ inline void gather_field(T* __restrict__ out, const T* __restrict__ ring, int W, int64_t b0, int n, const int64_t* s_row, int tid) {
    for (int j = tid; j < n * W; j += TPB) {
        const int i = j / W, rem = j - i * W;
        out[(b0 + i) * W + rem] = ring[s_row[i] * W + rem];
    }
}

// the five fields of the n rows s_row names, into rows b0 .. b0 + n - 1 of a batch
__device__ inline void gather_rows(const BsxReplayRing& g, float* obs, float* obs_next, float* act, float* rew, uint8_t* done, int64_t b0, int n,
                                   const int64_t* s_row, int tid) {
    const int WD = g.nA * g.D;
    gather_field(reinterpret_cast<uint32_t*>(obs), reinterpret_cast<const uint32_t*>(g.obs), WD, b0, n, s_row, tid);
    gather_field(reinterpret_cast<uint32_t*>(obs_next), reinterpret_cast<const uint32_t*>(g.obs_next), WD, b0, n, s_row, tid);
    gather_field(reinterpret_cast<uint32_t*>(act), reinterpret_cast<const uint32_t*>(g.act), g.nA * g.n_act, b0, n, s_row, tid);
    gather_field(reinterpret_cast<uint32_t*>(rew), reinterpret_cast<const uint32_t*>(g.rew), g.nA, b0, n, s_row, tid);
    gather_field(done, g.done, g.nA, b0, n, s_row, tid);
}

// BSX_E_ARG for a ring that is missing a pointer or has a shape out of range; 0 otherwise (alignment: ring_misaligned)
inline int check_ring(const BsxReplayRing* g) {
    if (!g || !g->obs || !g->obs_next || !g->act || !g->rew || !g->done || !g->counter) return BSX_E_ARG;
    if (g->M < 1 || g->M > MAX_ROWS || g->nA < 1 || g->nA > BSX_MAX_N || g->D < 1 || g->D > 3 * BSX_MAX_N + 2) return BSX_E_ARG;
    if (g->n_act != 3 && g->n_act != 4) return BSX_E_ARG;
    return 0;
}

inline bool ring_misaligned(const BsxReplayRing* g) {
    return !aligned(g->obs, 4) || !aligned(g->obs_next, 4) || !aligned(g->act, 4) || !aligned(g->rew, 4) || !aligned(g->counter, 8);
}

}  // namespace bsx_ring
