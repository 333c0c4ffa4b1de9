// bsx_qmix_head.hip -- the head of a QMIX update for the discrete game (include/battlespace_hip.h: bsx_qmix_head), gfx950.
//
// Two networks meet here: the team's Q network (the network its rollout plays; y4 = the tanh row of bsx_mlp_forward) and the mixer, a
// StackedActor of Mh = nA m + 2 m + 1 members on the team's joint observation whose tanh rows hy[b][member][0..3] ARE the weights of the
// monotone mix of that batch row: |.| of nA m rows is W1 [nA][E], m rows are b1 [E], |.| of m rows is w2 [E], column 0 of the last is b2,
// E = 4 m.  This pass lies between the four forwards and the two bsx_mlp_grad(squash = 1) calls: per batch row the mix of the replayed
// actions' values on the online rows, the mix of the greedy next actions' values on the target rows, the TD target, and BOTH grad_out
// tensors -- g4 for the Q network, gh for the mixer -- with the statistics.
// The readers of a score row, the tail from the TD target down and the entry's common part are bsx_q_head.h's, the DQN head's own.
// One thread per batch row on the TD heads' plan (bsx_ddpg_shared.h: plan_of(B, 1)), sums and merge.  pre, h and the slopes live in
// registers under compile-time indices: the agent loop is unrolled to QMIX_MAX_AGENTS with a guard, and the agents' W1 rows are read a
// second time (from cache) for the gradients instead of being kept.  Built with -ffp-contract=off: every operation is one float32
// rounding, every multiply-add an explicit fmaf, the one division __fdiv_rn (tests/qmix_util.py restates it in numpy).  Every index is
// 64-bit.  No exchange between threads, no atomics, no flags or spins; the grid is a function of B alone.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"
#include "bsx_q_head.h"

namespace {

constexpr int QMIX_MAX_AGENTS = BSX_QMIX_MAX_AGENTS;

inline bool qmix_embed(int embed) { return embed == 4 || embed == 8 || embed == 16; }
inline bool qmix_team(int nA) { return nA >= 1 && nA <= QMIX_MAX_AGENTS; }
inline int members_of(int nA, int embed) { return nA * (embed / 4) + 2 * (embed / 4) + 1; }

typedef QHeadArgs<BsxQmixIo> HeadArgs;         // M = B: one thread per batch row

__device__ __forceinline__ float sgn(float t) { return float(t > 0.0f) - float(t < 0.0f); }

// The mix of u[0 .. nA) under the hypernet rows hy (one batch row's Mh rows) -> tot; h and the slopes of the E hidden units are left in
// h[] and sl[].  The header's steps 1 to 3, in their order.
template <int E>
__device__ __forceinline__ float mix_of(const F4* hy, int nA, const float (&u)[QMIX_MAX_AGENTS], float (&h)[E], float (&sl)[E]) {
    constexpr int m = E / 4;
    float pre[E];
#pragma unroll
    for (int j = 0; j < m; ++j) {
        const F4 b1 = hy[nA * m + j];
#pragma unroll
        for (int c = 0; c < 4; ++c) pre[4 * j + c] = b1[c];
    }
#pragma unroll
    for (int i = 0; i < QMIX_MAX_AGENTS; ++i) {
        if (i < nA) {
#pragma unroll
            for (int j = 0; j < m; ++j) {
                const F4 t = hy[i * m + j];
#pragma unroll
                for (int c = 0; c < 4; ++c) pre[4 * j + c] = fmaf(u[i], fabsf(t[c]), pre[4 * j + c]);
            }
        }
    }
    float tot = hy[nA * m + 2 * m][0];
#pragma unroll
    for (int j = 0; j < m; ++j) {
        const F4 w2 = hy[nA * m + m + j];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = 4 * j + c;
            const float x = pre[e];
            const bool up = x > 0.0f;                              // a NaN takes the second branch and stays a NaN
            const float r = __fdiv_rn(1.0f, 1.0f - x);             // ONE correctly rounded division
            h[e] = up ? x : x * r;
            sl[e] = up ? 1.0f : r * r;
            tot = fmaf(h[e], fabsf(w2[c]), tot);
        }
    }
    return tot;
}

// One thread per batch row and tile of 256, J consecutive tiles per workgroup (bsx_ddpg_shared.h: plan_of(B, 1)); the sums as
// td_head_pass takes them.  FORM: bit 0 io.weight is given, bit 1 double Q, bits 2 and 3 the embedding width E = 4 << (FORM >> 2)
template <int FORM>
__global__ __launch_bounds__(TPB) void bsx_qmix_head_kernel(const HeadArgs p) {
    constexpr int WEIGHT = FORM & 1, DOUBLE = (FORM >> 1) & 1, E = 4 << (FORM >> 2), m = E / 4;
    const int tid = threadIdx.x, nA = p.nA, Mh = nA * m + 2 * m + 1;
    double acc[Q_NS] = {};                     // Q: Q_tot; done: the whole team over; greedy: the row's share
    const F4* yc4 = reinterpret_cast<const F4*>(p.io.y_cur);
    const F4* yt4 = reinterpret_cast<const F4*>(p.io.y_next_target);
    const F4* yo4 = reinterpret_cast<const F4*>(DOUBLE ? p.io.y_next_online : p.io.y_next_target);
    const F4* act4 = reinterpret_cast<const F4*>(p.io.act);
    F4* g4 = reinterpret_cast<F4*>(p.io.g4);
    F4* gh = reinterpret_cast<F4*>(p.io.gh);
    const int64_t tile0 = int64_t(blockIdx.x) * p.J;
    for (int jt = 0; jt < p.J; ++jt) {
        const int64_t tile = tile0 + jt, b = tile * TPB + tid;
        if (tile >= p.tiles || b >= p.M) continue;
        const int64_t r0 = b * nA, h0 = b * Mh;
        float h[E], sl[E], u[QMIX_MAX_AGENTS];
        int a[QMIX_MAX_AGENTS];
        // the target: the mix of the greedy next actions' values on the TARGET mixer's rows
        bool over = true;
        float R = 0.0f;
#pragma unroll
        for (int i = 0; i < QMIX_MAX_AGENTS; ++i) {
            u[i] = 0.0f, a[i] = 0;
            if (i < nA) {
                const bool fin = p.io.done[r0 + i] != 0;
                u[i] = fin ? 0.0f : pick(yt4[r0 + i], argmax_row(yo4[r0 + i]));    // select, never multiply
                over = over && fin;
                const float rw = p.io.rew[r0 + i];
                R = i == 0 ? rw : R + rw;
            }
        }
        const float tot_n = mix_of<E>(reinterpret_cast<const F4*>(p.io.hy_next_target) + h0, nA, u, h, sl);
        const float N = over ? 0.0f : p.q_scale * tot_n;
        const float y = q_target(p, N, R);
        // the mix of the replayed actions' values on the online mixer's rows
        int greedy = 0;
#pragma unroll
        for (int i = 0; i < QMIX_MAX_AGENTS; ++i) {
            if (i < nA) {
                const F4 yc = yc4[r0 + i];
                a[i] = argmax_row(act4[r0 + i]);
                u[i] = pick(yc, a[i]);
                greedy += a[i] == argmax_row(yc) ? 1 : 0;
            }
        }
        const F4* hy = reinterpret_cast<const F4*>(p.io.hy_cur) + h0;
        const float tot = mix_of<E>(hy, nA, u, h, sl);
        const float Q = p.q_scale * tot;
        const float w = WEIGHT ? p.io.weight[r0] : 1.0f;
        const QTail t = q_tail(p, Q, y, w);
        const float G = t.g;
        // ws_e = w2_e * slope_e into sl[]; the rows of b1 and w2, then b2's
#pragma unroll
        for (int j = 0; j < m; ++j) {
            const F4 t = hy[nA * m + m + j];
            F4 gb, gw;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int e = 4 * j + cc;
                sl[e] = fabsf(t[cc]) * sl[e];
                gb[cc] = G * sl[e];
                gw[cc] = (G * h[e]) * sgn(t[cc]);
            }
            gh[h0 + nA * m + j] = gb;
            gh[h0 + nA * m + m + j] = gw;
        }
        F4 last = F4(0.0f);
        last[0] = G;
        gh[h0 + nA * m + 2 * m] = last;
        // the agents a second time: W1's rows again for g4 and for their own gradient
#pragma unroll
        for (int i = 0; i < QMIX_MAX_AGENTS; ++i) {
            if (i < nA) {
                float S = 0.0f;
#pragma unroll
                for (int j = 0; j < m; ++j) {
                    const F4 t = hy[i * m + j];
                    F4 gw1;
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        const int e = 4 * j + cc;
                        S = fmaf(sl[e], fabsf(t[cc]), S);
                        gw1[cc] = (G * (sl[e] * u[i])) * sgn(t[cc]);
                    }
                    gh[h0 + i * m + j] = gw1;
                }
                g4[r0 + i] = one_hot(a[i], G * S);
                p.io.q[r0 + i] = Q;
                if (p.io.td) p.io.td[r0 + i] = y;
            }
        }
        q_sums(p, t, Q, w, over, acc);
        acc[6] += double(greedy) / double(nA);
    }
    store_partial_row(acc, p.part);
}

typedef void (*HeadKernel)(HeadArgs);
const HeadKernel KERNELS[12] = {bsx_qmix_head_kernel<0>, bsx_qmix_head_kernel<1>, bsx_qmix_head_kernel<2>,  bsx_qmix_head_kernel<3>,
                                bsx_qmix_head_kernel<4>, bsx_qmix_head_kernel<5>, bsx_qmix_head_kernel<6>,  bsx_qmix_head_kernel<7>,
                                bsx_qmix_head_kernel<8>, bsx_qmix_head_kernel<9>, bsx_qmix_head_kernel<10>, bsx_qmix_head_kernel<11>};

// x_cur[b][member][s] = obs[b][s], x_next[b][member][s] = obs_next[b][s]: one thread per float of one of them, strided beyond the grid
__global__ __launch_bounds__(TPB) void bsx_qmix_inputs_kernel(const float* __restrict__ obs, const float* __restrict__ obs_next, int64_t B,
                                                              int Mh, int S, float* __restrict__ x_cur, float* __restrict__ x_next) {
    const int64_t row = int64_t(Mh) * S, total = B * row, stride = int64_t(gridDim.x) * TPB;
    for (int64_t t = int64_t(blockIdx.x) * TPB + threadIdx.x; t < total; t += stride) {
        const int64_t b = t / row, src = b * S + (t - b * row) % S;
        x_cur[t] = obs[src];
        x_next[t] = obs_next[src];
    }
}

}  // namespace

extern "C" {

int bsx_qmix_members(int nA, int embed, int* members) {
    if (!members || !qmix_team(nA) || !qmix_embed(embed)) return BSX_E_ARG;
    *members = members_of(nA, embed);
    return 0;
}

int bsx_qmix_inputs(const float* obs, const float* obs_next, int64_t B, int nA, int Do, int members, float* x_cur, float* x_next,
                    void* stream) {
    if (!obs || !obs_next || !x_cur || !x_next) return BSX_E_ARG;
    if (B < 1 || B >= (INT64_C(1) << 31) || !qmix_team(nA) || Do < 1 || Do > MAX_DO || nA * Do > BSX_MLP_MAX_D) return BSX_E_ARG;
    if (members < 1 || members > 2 * BSX_MAX_N) return BSX_E_ARG;
    if (!aligned(obs, 4) || !aligned(obs_next, 4) || !aligned(x_cur, 4) || !aligned(x_next, 4)) return BSX_E_ALIGN;
    const int S = nA * Do;
    hipLaunchKernelGGL(bsx_qmix_inputs_kernel, dim3(copy_blocks(B * members * S)), dim3(TPB), 0, static_cast<hipStream_t>(stream), obs, obs_next,
                       B, members, S, x_cur, x_next);
    return int(hipGetLastError());
}

int bsx_qmix_head_workspace_bytes(int64_t B, int nA, size_t* bytes) {
    if (!qmix_team(nA)) return BSX_E_ARG;
    return head_workspace_bytes(B, 1, bytes);
}

int bsx_qmix_head(const BsxQmixIo* io, int64_t B, int nA, int embed, float gamma, float q_scale, float huber_delta, int double_q,
                  void* workspace, double* stats, void* stream) {
    if (!io || !io->y_cur || !io->y_next_target || !io->hy_cur || !io->hy_next_target || !io->act || !io->rew || !io->done || !io->g4 ||
        !io->gh || !io->q)
        return BSX_E_ARG;
    if (!head_ranges(gamma, B, 1, workspace, stats) || !qmix_team(nA) || !qmix_embed(embed)) return BSX_E_ARG;
    if (const int e = q_head_refusal(io, q_scale, huber_delta, double_q)) return e;
    if (!aligned(io->hy_cur, 16) || !aligned(io->hy_next_target, 16) || !aligned(io->gh, 16)) return BSX_E_ALIGN;
    const HeadArgs a{*io, 0, 0, 0, nA, gamma, q_scale, huber_delta, float(2.0 / double(B)), nullptr};
    const int form = (double_q << 1) | ((embed == 4 ? 0 : (embed == 8 ? 1 : 2)) << 2);
    return launch_head<true, HeadArgs>(KERNELS[form | 1], KERNELS[form], io->weight != nullptr, a, B, 1, workspace, stats, stream);
}

}  // extern "C"
