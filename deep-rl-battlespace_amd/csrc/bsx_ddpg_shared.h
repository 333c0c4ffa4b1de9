// bsx_ddpg_shared.h -- what bsx_ddpg_head.hip and bsx_td3_head.hip share: the checked shape of a critic input and the copy kernels' grid,
// the launch plan of a TD head pass, a function of (B, nA) alone, and the one-workgroup merge of its partial rows.  Each translation
// unit gets its own copy (unnamed namespace).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MERGE_TPB = 1024;
constexpr int64_t HEAD_MAX_BLOCKS = 1024;      // the head: one tile per workgroup up to 1 024 workgroups (four per CU), then more tiles each
constexpr int STAT_COLS = 8;                   // a partial row: 0 | the sums of a head's terms, in the order of its statistics

constexpr int64_t COPY_MAX_BLOCKS = 65536;     // the copy kernels stride over their elements beyond 2^24 threads
constexpr int MAX_DO = 3 * BSX_MAX_N + 2;      // an observation row of the widest team

typedef float F4 __attribute__((ext_vector_type(4)));

struct Shape {                                 // a checked (B, nA, Do, k, central)
    int64_t B;
    int nA, Do, k, central, Dc, W;             // W: the observation columns of a critic row (Do, or nA Do)
};

// the ranges every bsx_ddpg_* entry shares -> false for anything outside them, Dc > BSX_MLP_MAX_D (4v4 central: 72) included
inline bool shape_of(int64_t B, int nA, int Do, int k, int central, Shape* s) {
    if (B < 1 || B >= (INT64_C(1) << 31) || nA < 1 || nA > BSX_MAX_N || Do < 1 || Do > MAX_DO || (k != 3 && k != 4)) return false;
    if (central != 0 && central != 1) return false;
    const int Dc = central ? nA * (Do + k) : Do + k;
    if (Dc > BSX_MLP_MAX_D) return false;
    *s = Shape{B, nA, Do, k, central, Dc, central ? nA * Do : Do};
    return true;
}

inline unsigned copy_blocks(int64_t threads) {
    const int64_t b = (threads + TPB - 1) / TPB;
    return unsigned(b < COPY_MAX_BLOCKS ? b : COPY_MAX_BLOCKS);
}

struct Plan {                                  // the head's launch shape: a function of (B, nA) alone
    int64_t M, tiles, blocks;
    int J;
};

inline Plan plan_of(int64_t B, int nA) {
    Plan p;
    p.M = B * nA;
    p.tiles = (p.M + TPB - 1) / TPB;
    const int64_t J = (p.tiles + HEAD_MAX_BLOCKS - 1) / HEAD_MAX_BLOCKS;
    p.blocks = (p.tiles + J - 1) / J;
    p.J = int(J);
    return p;
}

inline bool td_shape(int64_t B, int nA) { return B >= 1 && B < (INT64_C(1) << 31) && nA >= 1 && nA <= BSX_MAX_N; }

// Q = 1024 / 8 threads per column; thread (q, c) adds the partial rows q, q + Q, .. in order; then 16 threads per column add every
// 16th of those sums, and one thread the rest -- a fixed order throughout.  LAST: the last column is a mean like the others (0 if not)
template <bool LAST>
__global__ __launch_bounds__(MERGE_TPB) void bsx_td_merge_kernel(const double* part, int64_t blocks, int64_t M, double* stats) {
    constexpr int C = STAT_COLS, Q = MERGE_TPB / C, G = 16;
    __shared__ double s_q[MERGE_TPB], s_r[G * C];
    const int tid = threadIdx.x, c = tid % C, q = tid / C;
    double t = 0.0;
    for (int64_t b = q; b < blocks; b += Q) t += part[b * C + c];
    s_q[q * C + c] = t;
    __syncthreads();
    if (q < G) {
        double u = 0.0;
        for (int k = q; k < Q; k += G) u += s_q[k * C + c];
        s_r[q * C + c] = u;
    }
    __syncthreads();
    if (tid < C) {
        double u = 0.0;
        for (int k = 0; k < G; ++k) u += s_r[k * C + tid];
        stats[tid] = tid == 0 ? double(M) : (!LAST && tid == C - 1 ? 0.0 : u / double(M));
    }
}

}  // namespace
