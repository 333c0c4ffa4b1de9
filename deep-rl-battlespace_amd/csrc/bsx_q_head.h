// bsx_q_head.h -- what bsx_dqn_head.hip and bsx_qmix_head.hip share, on top of bsx_ddpg_shared.h: the readers of a row of four scores,
// the kernels' argument, the head's tail from the TD target down, written ONCE as functions of the mixed quantities (Q, N, R, w), the
// one-hot grad_out row, and the C entries' common refusals.  Each translation unit gets its own copy (unnamed namespace).  Unlike
// td_head_pass the tail DOES contain a contractible expression, 2 ad - delta of the Huber loss term: it is the same arithmetic only
// under -ffp-contract=off, which both translation units are built with (build.py) and must stay built with.
#pragma once

#include "bsx_argmax4.h"
#include "bsx_ddpg_shared.h"

namespace {

constexpr int Q_NS = 7;                        // a partial row: 0 | w l(d) | Q | y | |d| | done | w | greedy

// a row of four scores: the step kernels' choice, and column a of a row by selects -- a dynamically indexed vector would live in scratch
__device__ __forceinline__ int argmax_row(const F4 v) { return bsxk::argmax4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ float pick(const F4 v, int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : (a == 2 ? v[2] : v[3])); }
// g in column a and +0 in the other three: selects again, for the same reason
__device__ __forceinline__ F4 one_hot(int a, float g) { return F4{a == 0 ? g : 0.0f, a == 1 ? g : 0.0f, a == 2 ? g : 0.0f, a == 3 ? g : 0.0f}; }

template <class Io>
struct QHeadArgs {                             // a head kernel's argument; Io: BsxDqnIo or BsxQmixIo
    Io io;
    int64_t M, tiles;                          // M: the plan's elements, one thread each (DQN: B nA; QMIX: B)
    int J, nA;
    float gamma, q_scale, delta, s2;           // delta: huber_delta (0: none); s2 = float(2.0 / B)
    double* part;                              // workspace: [blocks][STAT_COLS] partial rows
};

// The tail in the order both kernels run it.  From the next state's value N and the reward R of an element (DQN) or a batch row (QMIX):
// the TD target; with the value Q and the weight w: the error, |error| and the clipped error's gradient g = d loss / d (Q / q_scale) ...
struct QTail { float y, d, ad, g; };
template <class Io>
__device__ __forceinline__ float q_target(const QHeadArgs<Io>& p, float N, float R) { return fmaf(p.gamma, N, R); }
template <class Io>
__device__ __forceinline__ QTail q_tail(const QHeadArgs<Io>& p, float Q, float y, float w) {
    const float d = Q - y, ad = fabsf(d);
    const float c = (p.delta > 0.0f && d == d) ? fminf(fmaxf(d, -p.delta), p.delta) : d;  // a NaN stays a NaN
    return QTail{y, d, ad, ((w * c) * p.s2) * p.q_scale};
}
// ... and, after the caller's stores, the terms of the first six statistics into acc; over: the element is done (DQN), the whole team
// is (QMIX).  acc[6], the greedy term, is the caller's: 0 or 1 per element for DQN, the row's greedy share for QMIX.
template <class Io>
__device__ __forceinline__ void q_sums(const QHeadArgs<Io>& p, const QTail t, float Q, float w, bool over, double (&acc)[Q_NS]) {
    const float loss = (!(p.delta > 0.0f) || t.ad <= p.delta) ? (w * t.d) * t.d : w * (p.delta * (2.0f * t.ad - p.delta));
    acc[0] += double(loss);
    acc[1] += double(Q);
    acc[2] += double(t.y);
    acc[3] += double(t.ad);
    acc[4] += over ? 1.0 : 0.0;
    acc[5] += double(w);
}

// What both C entries refuse after their own null lists and ranges -> 0 or the code: the hypers (a NaN fails the comparisons too),
// then the alignment of what both io structs hold: 16 bytes for the four row tensors and g4, 4 for rew, weight, q and td
template <class Io>
inline int q_head_refusal(const Io* io, float q_scale, float huber_delta, int double_q) {
    if (!(q_scale > 0.0f) || !(huber_delta >= 0.0f) || (double_q != 0 && double_q != 1) || (double_q && !io->y_next_online)) return BSX_E_ARG;
    const bool ok = aligned(io->y_cur, 16) && aligned(io->y_next_online, 16) && aligned(io->y_next_target, 16) && aligned(io->act, 16) &&
                    aligned(io->g4, 16) && aligned(io->rew, 4) && aligned(io->weight, 4) && aligned(io->q, 4) && aligned(io->td, 4);
    return ok ? 0 : BSX_E_ALIGN;
}

}  // namespace
