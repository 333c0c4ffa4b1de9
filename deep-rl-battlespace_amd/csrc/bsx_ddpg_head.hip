// bsx_ddpg_head.hip -- what lies between the fused MLP calls of a DDPG / MADDPG update (include/battlespace_hip.h: bsx_ddpg_*, bsx_td_head), gfx950.
//
// A sampled batch (obs, obs_next [B][nA][Do], act [B][nA][k]) becomes the critic's three inputs, a network's 4-wide output rows go into
// a critic input's action columns, the critic's outputs become the TD target and both grad_out tensors, and the critic's input gradient
// gives the actor's grad_out.  Row (b, i) of a critic input holds Dc floats:
//   own      obs[b][i] (+) a[b][i]                                     Dc = Do + k
//   central  obs[b][0] .. obs[b][nA-1] (+) a[b][0] .. a[b][nA-1]       Dc = nA (Do + k): the same row for every agent i of b
//   1. inputs       one thread per float of x_cur: the batch's part of x_cur, x_next and x_pi, one launch;
//   2. put_actions  one thread per (row, action slot): a 16-byte load of y4, k dword stores where bsx_ddpg_shared.h's action_slot says;
//   3. td_head      the shared head pass (bsx_ddpg_shared.h: td_head_pass) with ONE critic: the kernel here hands it its argument, the
//                   entry its own pointer lists; the plan, the sums, the merge and the rest of the entry are the header's;
//   4. action_grad  one thread per row: k dword loads of grad_x, a 16-byte store of g_a4.
// Rows of 9, 24 or 45 floats are not 16-byte aligned: the critic inputs and grad_x are read and written by the dword; the 16-byte
// accesses are those of the [..][4] tensors.  Every index is 64-bit: there is one path whatever the size.  No floating-point atomics,
// no flags or spins; every grid is a function of the sizes alone: the same inputs give the same bits on every call.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"
#include "bsx_ddpg_shared.h"         // TPB, the checked shape, action_slot, the head pass with its plan, merge and entry helpers

namespace {

__global__ __launch_bounds__(TPB) void bsx_ddpg_inputs_kernel(const BsxDdpgBatch batch, const Shape s, float* x_cur, float* x_next, float* x_pi) {
    const int64_t M = s.B * s.nA * s.Dc, stride = int64_t(gridDim.x) * TPB;
    for (int64_t e = int64_t(blockIdx.x) * TPB + threadIdx.x; e < M; e += stride) {
        const int64_t r = e / s.Dc, b = r / s.nA;
        const int c = int(e - r * s.Dc);
        const int64_t row = s.central ? b : r;                 // the batch row this critic row reads: its own, or the whole team's
        const int slots = s.central ? s.nA : 1;
        if (c < s.W) {
            const int64_t src = row * s.W + c;
            const float o = batch.obs[src];
            x_cur[e] = o;
            x_pi[e] = o;
            x_next[e] = batch.obs_next[src];
        } else {
            const float a = batch.act[row * (slots * s.k) + (c - s.W)];
            x_cur[e] = a;
            if (s.central) x_pi[e] = a;                        // the other agents' slots keep the replayed actions (put_actions fills slot i)
        }
    }
}

// thread (r, slot): own, or central with own_only: slot = the row's own agent, one per row; central without: every slot of every row
__global__ __launch_bounds__(TPB) void bsx_ddpg_put_actions_kernel(const float* y4, const Shape s, int every_slot, float* x) {
    const int S = every_slot ? s.nA : 1;
    const int64_t M = s.B * s.nA * S, stride = int64_t(gridDim.x) * TPB;
    const F4* y = reinterpret_cast<const F4*>(y4);
    for (int64_t e = int64_t(blockIdx.x) * TPB + threadIdx.x; e < M; e += stride) {
        const int64_t r = e / S, b = r / s.nA;
        const int i = int(r - b * s.nA), slot = every_slot ? int(e - r * S) : i;
        const F4 a = y[s.central ? b * s.nA + slot : r];
        store_row(action_slot(s, x, b, slot, r, false).dst, s.k, a[0], a[1], a[2], a[3]);      // one row per thread
    }
}

__global__ __launch_bounds__(TPB) void bsx_ddpg_action_grad_kernel(const float* gx, const Shape s, float* g_a4) {
    const int64_t M = s.B * s.nA, stride = int64_t(gridDim.x) * TPB;
    F4* g = reinterpret_cast<F4*>(g_a4);
    for (int64_t r = int64_t(blockIdx.x) * TPB + threadIdx.x; r < M; r += stride) {
        const int i = int(r % s.nA);
        const float* src = gx + r * s.Dc + s.W + (s.central ? i * s.k : 0);
        F4 a;
        a[0] = src[0];
        a[1] = src[1];
        a[2] = src[2];
        a[3] = s.k == 4 ? src[3] : 0.0f;
        g[r] = a;
    }
}

struct HeadArgs {
    BsxTdIo io;
    int64_t M, tiles;
    int J;
    float gamma, s1, s2;                       // s1 = float(1.0 / B), s2 = float(2.0 / B)
    double* part;                              // workspace: [blocks][STAT_COLS] partial rows
};

template <int WEIGHT>                          // 1: io.weight is given
__global__ __launch_bounds__(TPB) void bsx_td_head_kernel(const HeadArgs p) {
    const BsxTdIo& io = p.io;
    td_head_pass<HEAD_ONE, WEIGHT>(HeadView{io.q, nullptr, io.q_next, nullptr, nullptr, nullptr, io.rew, io.done, io.weight, io.g_q, nullptr, io.g_pi,
                                            io.td, p.M, p.tiles, p.J, 0, p.gamma, p.s1, p.s2, p.part});
}

}  // namespace

extern "C" {

int bsx_ddpg_inputs(const BsxDdpgBatch* batch, int64_t B, int nA, int Do, int k, int central, float* x_cur, float* x_next, float* x_pi,
                    void* stream) {
    Shape s;
    if (!batch || !batch->obs || !batch->obs_next || !batch->act || !x_cur || !x_next || !x_pi) return BSX_E_ARG;
    if (!shape_of(B, nA, Do, k, central, &s)) return BSX_E_ARG;
    if (!aligned(batch->obs, 4) || !aligned(batch->obs_next, 4) || !aligned(batch->act, 4) || !aligned(x_cur, 4) || !aligned(x_next, 4) ||
        !aligned(x_pi, 4))
        return BSX_E_ALIGN;
    hipLaunchKernelGGL(bsx_ddpg_inputs_kernel, dim3(copy_blocks(s.B * s.nA * s.Dc)), dim3(TPB), 0, static_cast<hipStream_t>(stream), *batch, s,
                       x_cur, x_next, x_pi);
    return int(hipGetLastError());
}

int bsx_ddpg_put_actions(const float* y4, int64_t B, int nA, int Do, int k, int central, int own_only, float* x, void* stream) {
    Shape s;
    if (!y4 || !x || (own_only != 0 && own_only != 1)) return BSX_E_ARG;
    if (!shape_of(B, nA, Do, k, central, &s)) return BSX_E_ARG;
    if (!aligned(y4, 16) || !aligned(x, 4)) return BSX_E_ALIGN;
    const int every_slot = central && !own_only;
    hipLaunchKernelGGL(bsx_ddpg_put_actions_kernel, dim3(copy_blocks(s.B * s.nA * (every_slot ? s.nA : 1))), dim3(TPB), 0,
                       static_cast<hipStream_t>(stream), y4, s, every_slot, x);
    return int(hipGetLastError());
}

int bsx_ddpg_action_grad(const float* gx, int64_t B, int nA, int Do, int k, int central, float* g_a4, void* stream) {
    Shape s;
    if (!gx || !g_a4) return BSX_E_ARG;
    if (!shape_of(B, nA, Do, k, central, &s)) return BSX_E_ARG;
    if (!aligned(g_a4, 16) || !aligned(gx, 4)) return BSX_E_ALIGN;
    hipLaunchKernelGGL(bsx_ddpg_action_grad_kernel, dim3(copy_blocks(s.B * s.nA)), dim3(TPB), 0, static_cast<hipStream_t>(stream), gx, s, g_a4);
    return int(hipGetLastError());
}

int bsx_td_head_workspace_bytes(int64_t B, int nA, size_t* bytes) { return head_workspace_bytes(B, nA, bytes); }

int bsx_td_head(const BsxTdIo* io, int64_t B, int nA, float gamma, void* workspace, double* stats, void* stream) {
    if (!io || !io->q || !io->q_next || !io->rew || !io->done || !io->g_q || !io->g_pi) return BSX_E_ARG;
    if (!head_ranges(gamma, B, nA, workspace, stats)) return BSX_E_ARG;
    if (!aligned(io->g_q, 16) || !aligned(io->g_pi, 16)) return BSX_E_ALIGN;
    if (!aligned(io->q, 4) || !aligned(io->q_next, 4) || !aligned(io->rew, 4) || !aligned(io->weight, 4) || !aligned(io->td, 4)) return BSX_E_ALIGN;
    const HeadArgs a{*io, 0, 0, 0, gamma, float(1.0 / double(B)), float(2.0 / double(B)), nullptr};
    return launch_head<false>(bsx_td_head_kernel<1>, bsx_td_head_kernel<0>, io->weight != nullptr, a, B, nA, workspace, stats, stream);
}

}  // extern "C"
