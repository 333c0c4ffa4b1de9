// bsx_td3_head.hip -- what TD3 / MATD3 adds between the fused MLP calls of a DDPG update (include/battlespace_hip.h: bsx_td3_*), gfx950.
//
//   1. smooth_actions  target policy smoothing: a' = clamp(y4 + clamp(sigma z, -clip, clip), -1, 1) into the action columns of x_next,
//                      the slots bsx_ddpg_put_actions(own_only = 0) writes.  One thread per (b, j): ONE draw (normals4 under TD3_SALT, or
//                      the injected row), a 16-byte load of y4, then k dword stores into agent j's slot of each of the nA rows of b
//                      (central), or of its own row (bsx_ddpg_shared.h: action_slot) -- the noise is keyed by (b, j), so the rows of b
//                      hold the same bits;
//   2. td3_head        clipped double-Q: y from the smaller of two target critics, both critics' grad_out, the actor's seed through
//                      critic 1.  It is bsx_td_head with two critics, and written as that: the shared head pass (bsx_ddpg_shared.h:
//                      td_head_pass) of kind HEAD_TWIN, with the header's plan, sums, merge and entry helpers.
// Built with -ffp-contract=off: every operation of the smoothing is one float32 rounding (tests/td3_util.py restates it in numpy), and
// the head's one multiply-add is an explicit fmaf; normals4 pins its own contraction mode.  Every index is 64-bit: there is one path
// whatever the size.  No floating-point atomics, no flags or spins; every grid is a function of the sizes alone.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_core.h"          // normals4: the project's pinned Box-Muller draw
#include "bsx_args.h"
#include "bsx_ddpg_shared.h"

namespace {

// distinct from the four in use (bsx_actor_core.h): 0x00000000, 0x80000000, 0x40000000 and GAUSS_SALT = 0xC0000000
constexpr uint32_t TD3_SALT = 0x20000000u;

struct SmoothArgs {
    const float* y4;
    const float* z_inject;
    const uint64_t* seq_base;
    float* x;
    uint64_t seed, seq;
    float sigma, clip;
};

__device__ inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // np.clip's rule: a NaN stays

__global__ __launch_bounds__(TPB) void bsx_td3_smooth_kernel(const SmoothArgs p, const Shape s) {
    const int64_t M = s.B * s.nA, stride = int64_t(gridDim.x) * TPB;
    const F4* y = reinterpret_cast<const F4*>(p.y4);
    const F4* zi = reinterpret_cast<const F4*>(p.z_inject);
    const uint64_t seq = p.seq + (p.seq_base ? *p.seq_base : 0ull);
    for (int64_t r = int64_t(blockIdx.x) * TPB + threadIdx.x; r < M; r += stride) {
        const int64_t b = r / s.nA;
        const int j = int(r - b * s.nA);
        F4 z;
        if (zi) {
            z = zi[r];
        } else {
            const float4 n4 = bsx_actor::normals4(p.seed, seq, uint64_t(r), TD3_SALT);
            z = F4{n4.x, n4.y, n4.z, n4.w};
        }
        const F4 a = y[r];
        float out[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float n = clampf(p.sigma * z[c], -p.clip, p.clip);
            out[c] = clampf(a[c] + n, -1.0f, 1.0f);
        }
        // central: slot j of every row (b, i); own: the row's own columns
        store_actions(action_slot(s, p.x, b, j, r, s.central), s.Dc, s.k, out[0], out[1], out[2], out[3]);
    }
}

struct HeadArgs {
    BsxTd3Io io;
    int64_t M, tiles;
    int J;
    float gamma, s1, s2;                       // s1 = float(1.0 / B), s2 = float(2.0 / B)
    double* part;                              // workspace: [blocks][STAT_COLS] partial rows
};

template <int WEIGHT>                          // 1: io.weight is given
__global__ __launch_bounds__(TPB) void bsx_td3_head_kernel(const HeadArgs p) {
    const BsxTd3Io& io = p.io;
    td_head_pass<HEAD_TWIN, WEIGHT>(HeadView{io.q1, io.q2, io.q1_next, io.q2_next, nullptr, nullptr, io.rew, io.done, io.weight, io.g_q1, io.g_q2,
                                             io.g_pi, io.td, p.M, p.tiles, p.J, 0, p.gamma, p.s1, p.s2, p.part});
}

}  // namespace

extern "C" {

int bsx_td3_smooth_actions(const float* y4, int64_t B, int nA, int Do, int k, int central, float sigma, float clip, uint64_t seed,
                           uint64_t seq, const uint64_t* seq_base, const float* z_inject, float* x, void* stream) {
    Shape s;
    if (!y4 || !x) return BSX_E_ARG;
    if (!shape_of(B, nA, Do, k, central, &s)) return BSX_E_ARG;
    if (!(sigma >= 0.0f) || !(clip >= 0.0f)) return BSX_E_ARG;                 // NaN too
    if (!aligned(y4, 16) || !aligned(z_inject, 16) || !aligned(x, 4) || !aligned(seq_base, 8)) return BSX_E_ALIGN;
    const SmoothArgs a{y4, z_inject, seq_base, x, seed, seq, sigma, clip};
    hipLaunchKernelGGL(bsx_td3_smooth_kernel, dim3(copy_blocks(s.B * s.nA)), dim3(TPB), 0, static_cast<hipStream_t>(stream), a, s);
    return int(hipGetLastError());
}

int bsx_td3_head_workspace_bytes(int64_t B, int nA, size_t* bytes) { return head_workspace_bytes(B, nA, bytes); }

int bsx_td3_head(const BsxTd3Io* io, int64_t B, int nA, float gamma, void* workspace, double* stats, void* stream) {
    if (!io || !io->q1 || !io->q2 || !io->q1_next || !io->q2_next || !io->rew || !io->done || !io->g_q1 || !io->g_q2 || !io->g_pi) return BSX_E_ARG;
    if (!head_ranges(gamma, B, nA, workspace, stats)) return BSX_E_ARG;
    if (!aligned(io->g_q1, 16) || !aligned(io->g_q2, 16) || !aligned(io->g_pi, 16)) return BSX_E_ALIGN;
    if (!aligned(io->q1, 4) || !aligned(io->q2, 4) || !aligned(io->q1_next, 4) || !aligned(io->q2_next, 4) || !aligned(io->rew, 4) ||
        !aligned(io->weight, 4) || !aligned(io->td, 4))
        return BSX_E_ALIGN;
    const HeadArgs a{*io, 0, 0, 0, gamma, float(1.0 / double(B)), float(2.0 / double(B)), nullptr};
    return launch_head<true>(bsx_td3_head_kernel<1>, bsx_td3_head_kernel<0>, io->weight != nullptr, a, B, nA, workspace, stats, stream);
}

}  // extern "C"
