// bsx_dqn_head.hip -- the head of a DQN update for the discrete game (include/battlespace_hip.h: bsx_dqn_head), gfx950.
//
// The Q network of a team is the network its rollout plays, Q_i(o, a) = q_scale * y4[i][a] with y4 the tanh row of bsx_mlp_forward; this
// pass lies between the forwards and bsx_mlp_grad(squash = 1).  Per element (b, i): the replayed action a = argmax4 of the replayed score
// row -- the step kernels' own argmax4 (bsx_argmax4.h) --, the next state's greedy action from the online rows (double Q) or the target
// rows, the TD target, its clipped error into column a of g4, the statistics.  mix = 1 (VDN): Q and the target are sums over the row's
// agents in agent order; every thread of a row adds them itself (nA <= 16 rows of 16 bytes, served from cache), so a row may lie across
// two tiles or workgroups and there is nothing to exchange.
// It is built on bsx_q_head.h, what the two discrete heads share (the tail from the TD target down among it), itself on
// bsx_ddpg_shared.h: the TD heads' plan, per-workgroup sums, merge kernel and entry helpers.  Built with -ffp-contract=off:
// every operation is one float32 rounding and the one multiply-add is an explicit fmaf (tests/dqn_util.py restates it in numpy).  Every
// index is 64-bit.  No floating-point atomics, no flags or spins; the grid is a function of (B, nA) alone.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"
#include "bsx_q_head.h"

namespace {

typedef QHeadArgs<BsxDqnIo> HeadArgs;

struct Elem {                                  // what element (b, i) contributes on its own
    float qc, qn;
    int a;
    bool over, greedy;
};

template <int DOUBLE>
__device__ __forceinline__ Elem elem_of(const HeadArgs& p, int64_t i) {
    const F4 yc = reinterpret_cast<const F4*>(p.io.y_cur)[i];
    const F4 yt = reinterpret_cast<const F4*>(p.io.y_next_target)[i];
    const F4 sel = DOUBLE ? reinterpret_cast<const F4*>(p.io.y_next_online)[i] : yt;
    Elem e;
    e.a = argmax_row(reinterpret_cast<const F4*>(p.io.act)[i]);
    e.over = p.io.done[i] != 0;
    e.qn = e.over ? 0.0f : p.q_scale * pick(yt, argmax_row(sel));     // select, never multiply: a finished row's next value stays out
    e.qc = p.q_scale * pick(yc, e.a);
    e.greedy = e.a == argmax_row(yc);
    return e;
}

// One thread per element and tile of 256, J consecutive tiles per workgroup (bsx_ddpg_shared.h: plan_of); the sums as td_head_pass takes them
// FORM: bit 0 io.weight is given, bit 1 double Q, bit 2 the VDN mix
template <int FORM>
__global__ __launch_bounds__(TPB) void bsx_dqn_head_kernel(const HeadArgs p) {
    constexpr int WEIGHT = FORM & 1, DOUBLE = (FORM >> 1) & 1, MIX = (FORM >> 2) & 1;
    const int tid = threadIdx.x;
    double acc[Q_NS] = {};
    F4* g4 = reinterpret_cast<F4*>(p.io.g4);
    const int64_t tile0 = int64_t(blockIdx.x) * p.J;
    for (int j = 0; j < p.J; ++j) {
        const int64_t tile = tile0 + j, i = tile * TPB + tid;
        if (tile >= p.tiles || i >= p.M) continue;
        const Elem e = elem_of<DOUBLE>(p, i);
        float Q = e.qc, N = e.qn, R = p.io.rew[i];
        int64_t wi = i;
        if constexpr (MIX) {                   // the row's sums, in agent order from agent 0
            const int64_t r0 = (i / p.nA) * p.nA;
            const Elem e0 = elem_of<DOUBLE>(p, r0);
            Q = e0.qc, N = e0.qn, R = p.io.rew[r0], wi = r0;
            for (int k = 1; k < p.nA; ++k) {
                const Elem ek = elem_of<DOUBLE>(p, r0 + k);
                Q = Q + ek.qc;
                N = N + ek.qn;
                R = R + p.io.rew[r0 + k];
            }
        }
        const float w = WEIGHT ? p.io.weight[wi] : 1.0f;
        const QTail t = q_tail(p, Q, q_target(p, N, R), w);
        g4[i] = one_hot(e.a, t.g);
        p.io.q[i] = Q;
        if (p.io.td) p.io.td[i] = t.y;
        q_sums(p, t, Q, w, e.over, acc);
        acc[6] += e.greedy ? 1.0 : 0.0;
    }
    store_partial_row(acc, p.part);
}

typedef void (*HeadKernel)(HeadArgs);
const HeadKernel KERNELS[8] = {bsx_dqn_head_kernel<0>, bsx_dqn_head_kernel<1>, bsx_dqn_head_kernel<2>, bsx_dqn_head_kernel<3>,
                               bsx_dqn_head_kernel<4>, bsx_dqn_head_kernel<5>, bsx_dqn_head_kernel<6>, bsx_dqn_head_kernel<7>};

}  // namespace

extern "C" {

int bsx_dqn_head_workspace_bytes(int64_t B, int nA, size_t* bytes) { return head_workspace_bytes(B, nA, bytes); }

int bsx_dqn_head(const BsxDqnIo* io, int64_t B, int nA, float gamma, float q_scale, float huber_delta, int double_q, int mix, void* workspace,
                 double* stats, void* stream) {
    if (!io || !io->y_cur || !io->y_next_target || !io->act || !io->rew || !io->done || !io->g4 || !io->q) return BSX_E_ARG;
    if (!head_ranges(gamma, B, nA, workspace, stats)) return BSX_E_ARG;
    if (mix != 0 && mix != 1) return BSX_E_ARG;
    if (const int e = q_head_refusal(io, q_scale, huber_delta, double_q)) return e;
    const HeadArgs a{*io, 0, 0, 0, nA, gamma, q_scale, huber_delta, float(2.0 / double(B)), nullptr};
    const int form = (double_q << 1) | (mix << 2);
    return launch_head<true, HeadArgs>(KERNELS[form | 1], KERNELS[form], io->weight != nullptr, a, B, nA, workspace, stats, stream);
}

}  // extern "C"
