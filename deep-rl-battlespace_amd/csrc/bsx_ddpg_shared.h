// bsx_ddpg_shared.h -- what bsx_ddpg_head.hip, bsx_td3_head.hip and bsx_sac_head.hip share.  The checked shape of a critic input, the
// copy kernels' grid and the address of an agent's action columns in a critic row; and the TD head, written ONCE: its launch plan (a
// function of (B, nA) alone), its per-element pass as a device function of the kind of head, the one-workgroup merge of its partial
// rows, and the part of the three C entries that does not depend on the kind.  Each translation unit gets its own copy (unnamed
// namespace) under its own flags: the head's body has no contractible expression, its multiply-adds are explicit fmafs, so it is the same
// arithmetic with and without -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"
#include "bsx_block_sum.h"

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

// Where agent j's action of batch row b goes in the critic input x: its k columns (central: slot j; own: the row's only slot) of critic
// row r = (b, i), or, with every, of all nA rows of b -- what bsx_ddpg_put_actions(own_only = 0) fills.  own: r = (b, j).
struct Slot {
    float* dst;
    int rows;                                  // that many rows, Dc floats apart
};

__device__ __forceinline__ Slot action_slot(const Shape s, float* x, int64_t b, int j, int64_t r, bool every) {
    return Slot{x + (every ? b * s.nA : r) * s.Dc + s.W + (s.central ? j * s.k : 0), every ? s.nA : 1};
}

__device__ __forceinline__ void store_row(float* dst, int k, float a0, float a1, float a2, float a3) {
    dst[0] = a0;
    dst[1] = a1;
    dst[2] = a2;
    if (k == 4) dst[3] = a3;
}

__device__ inline void store_actions(Slot t, int Dc, int k, float a0, float a1, float a2, float a3) {
    for (int i = 0; i < t.rows; ++i, t.dst += Dc) store_row(t.dst, k, a0, a1, a2, a3);
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

// The three heads (include/battlespace_hip.h: bsx_td_head, bsx_td3_head, bsx_sac_head) are one pass:
//   HEAD_ONE    one critic: the next state's value is q1_next; g_q1, g_pi; six statistics
//   HEAD_TWIN   HEAD_ONE with two critics: the smaller of q1_next and q2_next; g_q2 as well; |q1 - q2| as the seventh statistic
//   HEAD_SOFT   HEAD_TWIN with the soft value fmaf(-alpha, logp_next, m) for the smaller m, alpha = expf(log_alpha[agent]); no g_pi
enum HeadKind { HEAD_ONE, HEAD_TWIN, HEAD_SOFT };

struct HeadView {                              // the pass's view of a head kernel's argument: a kind reads only what its io struct has
    const float *q1, *q2, *q1_next, *q2_next, *logp_next, *log_alpha, *rew;
    const uint8_t* done;
    const float* weight;
    float *g_q1, *g_q2, *g_pi, *td;
    int64_t M, tiles;
    int J, nA;
    float gamma, s1, s2;                       // s1 = float(1.0 / B), s2 = float(2.0 / B)
    double* part;                              // workspace: [blocks][STAT_COLS] partial rows
};

// The end of every head kernel, the discrete heads' (bsx_q_head.h) included: a thread's NS float64 sums are added across the workgroup
// in a fixed order (bsx_block_sum.h) and stored as the workgroup's partial row, 0 | the NS sums | 0 up to STAT_COLS
template <int NS>
__device__ __forceinline__ void store_partial_row(const double (&acc)[NS], double* part) {
    __shared__ double s_w[NS][WAVES];
    const int tid = threadIdx.x;
    double sum[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) sum[c] = block_sum<double, WAVES>(acc[c], s_w[c]);
    if (tid < STAT_COLS) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < NS; ++c) t = tid == c + 1 ? sum[c] : t;
        part[int64_t(blockIdx.x) * STAT_COLS + tid] = t;
    }
}

// One thread per element and tile of 256, J consecutive tiles per workgroup; the float32 terms of the statistics are added in float64 per
// thread, then across the workgroup and stored (store_partial_row).  WEIGHT 1: weight is given
template <HeadKind KIND, int WEIGHT>
__device__ __forceinline__ void td_head_pass(const HeadView& p) {
    constexpr bool TWIN = KIND != HEAD_ONE, SOFT = KIND == HEAD_SOFT;
    constexpr int NS = TWIN ? 7 : 6;           // a partial row: 0 | w (d1^2 + d2^2) | q1 | y | |d1| | done | w | |q1 - q2| (0 with one critic)
    const int tid = threadIdx.x;
    double acc[NS] = {};
    F4* gq14 = reinterpret_cast<F4*>(p.g_q1);
    F4* gq24 = reinterpret_cast<F4*>(p.g_q2);
    F4* gpi4 = reinterpret_cast<F4*>(p.g_pi);
    const int64_t tile0 = int64_t(blockIdx.x) * p.J;
    for (int j = 0; j < p.J; ++j) {
        const int64_t tile = tile0 + j, i = tile * TPB + tid;
        if (tile >= p.tiles || i >= p.M) continue;
        const float q = p.q1[i], q2 = TWIN ? p.q2[i] : q, rew = p.rew[i];
        const float n1 = TWIN ? p.q1_next[i] : 0.0f, n2 = TWIN ? p.q2_next[i] : 0.0f;
        const bool over = p.done[i] != 0;
        const float alpha = SOFT ? expf(p.log_alpha[i % p.nA]) : 0.0f;
        const float m = (n1 < n2 || n1 != n1) ? n1 : n2;           // np.minimum's rule: a NaN in either is a NaN (fminf would drop it)
        const float v = SOFT ? fmaf(-alpha, p.logp_next[i], m) : m;    // the soft value of the next state
        const float qn = over ? 0.0f : (TWIN ? v : p.q1_next[i]);  // select, never multiply: a finished row's next-state terms stay out, NaN included
        const float w = WEIGHT ? p.weight[i] : 1.0f;
        const float y = fmaf(p.gamma, qn, rew);
        const float d = q - y, wd = w * d;
        const float d2 = q2 - y, wd2 = w * d2;
        F4 gq = F4(0.0f), gq2 = F4(0.0f), gp = F4(0.0f);
        gq[0] = wd * p.s2;
        gq2[0] = wd2 * p.s2;
        gp[0] = -(w * p.s1);
        gq14[i] = gq;
        if constexpr (TWIN) gq24[i] = gq2;
        if constexpr (!SOFT) gpi4[i] = gp;
        if (p.td) p.td[i] = y;
        acc[0] += TWIN ? double(wd * d) + double(wd2 * d2) : double(wd * d);
        acc[1] += double(q);
        acc[2] += double(y);
        acc[3] += double(fabsf(d));
        acc[4] += over ? 1.0 : 0.0;
        acc[5] += double(w);
        if constexpr (TWIN) acc[6] += double(fabsf(q - q2));
    }
    store_partial_row(acc, p.part);
}

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

// What a head entry does around its own lists of io pointers.  After the null list: the other BSX_E_ARG refusals
inline bool head_ranges(float gamma, int64_t B, int nA, const void* workspace, const void* stats) {
    return workspace && stats && gamma >= 0.0f && gamma <= 1.0f && td_shape(B, nA);                // (a NaN gamma fails both comparisons)
}

inline int head_workspace_bytes(int64_t B, int nA, size_t* bytes) {
    if (!bytes || !td_shape(B, nA)) return BSX_E_ARG;
    *bytes = size_t(plan_of(B, nA).blocks) * STAT_COLS * 8;
    return 0;
}

// After the alignment list: the last BSX_E_ALIGN refusal, the plan into the kernel's argument `a` (its io, gamma and scales are the
// entry's), the pass -- `weighted` when the io has a weight -- and the merge.  LAST: bsx_td_merge_kernel's
template <bool LAST, class Args>
inline int launch_head(void (*weighted)(Args), void (*plain)(Args), bool has_weight, Args a, int64_t B, int nA, void* workspace, double* stats,
                       void* stream) {
    if (!aligned(workspace, 8) || !aligned(stats, 8)) return BSX_E_ALIGN;
    const Plan p = plan_of(B, nA);
    a.M = p.M, a.tiles = p.tiles, a.J = p.J, a.part = static_cast<double*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(has_weight ? weighted : plain, dim3(unsigned(p.blocks)), dim3(TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(bsx_td_merge_kernel<LAST>, dim3(1), dim3(MERGE_TPB), 0, s, static_cast<const double*>(a.part), p.blocks, p.M, stats);
    return int(hipGetLastError());
}

}  // namespace
