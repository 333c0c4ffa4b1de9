// bsx_sac_head.hip -- what soft actor-critic adds between the fused MLP calls of a twin-critic update (include/battlespace_hip.h: bsx_sac_*), gfx950.
//
//   1. sample_actions  the reparameterised draw of the project's Gaussian policy (bsx_actor_core.h, finish_row<true>): a = mu + exp(log_std) z
//                      into the action columns of a critic input, where bsx_ddpg_put_actions(own_only) writes, and its log-probability.
//                      One thread per (b, j): ONE draw (normals4 under SAC_SALT, or the injected row), a 16-byte load of y4, three dword
//                      stores per row written (bsx_ddpg_shared.h: action_slot);
//   2. sac_head        bsx_td3_head with the entropy term in the target: y = r + gamma (1 - done) (min(Q1', Q2') - alpha logp'), and
//                      written as that: the shared head pass (bsx_ddpg_shared.h: td_head_pass) of kind HEAD_SOFT -- one fmaf more than
//                      HEAD_TWIN, no g_pi -- with the header's plan, sums, merge and entry helpers;
//   3. policy_seed     the seeds of the two critics' input-gradient passes on x_pi: -(w / B) at the smaller critic, +0 at the other;
//   4. policy_grad     the actor's grad_out from both critics' input gradients, log_std's and log_alpha's gradients and the policy's
//                      statistics.  A tile is S = (256 / nA) nA elements, so a thread keeps its agent over its J tiles; the float32 terms
//                      are added in float64 per thread, then across the workgroup in a fixed order (the statistics by block_sum, the
//                      per-agent sums through LDS, as bsx_ppo_head does log_std's), and stored to the workspace; ONE workgroup adds the
//                      workgroups' partial rows in a fixed order, writes the gradients and, when asked, takes log_alpha's Adam step.
// Built with -ffp-contract=off: every operation is one float32 rounding and every multiply-add an explicit fmaf (tests/sac_util.py
// restates them); normals4 pins its own contraction mode.  Every index is 64-bit: there is one path whatever the size.  No
// floating-point atomics, no flags or spins; every grid is a function of the sizes alone.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_core.h"          // normals4, HALF_LOG_2PI
#include "bsx_args.h"
#include "bsx_block_sum.h"
#include "bsx_ddpg_shared.h"

namespace {

constexpr uint32_t SAC_SALT = BSX_SAC_SALT;    // distinct from the five in use: 0x00000000, 0x80000000, 0x40000000, 0xC0000000, 0x20000000
constexpr int NP = 6;                          // policy_grad's: 0 | w (alpha logp - m) | m | logp | alpha | w | picked 1 | 0 | per agent [nA][AG]
constexpr int AG = 5;                          // per agent: g_a (sigma z) for the three columns | w s1 | (w s1) (logp + target_entropy)
constexpr int LS_PARTS_MAX = 8;

struct SampleArgs {
    const float* y4;
    const float* log_std;
    const float* z_inject;
    const uint64_t* seq_base;
    float* x;
    float* logp;
    float* z_out;
    uint64_t seed, seq;
    int own_only;
};

__global__ __launch_bounds__(TPB) void bsx_sac_sample_kernel(const SampleArgs p, const Shape s) {
    const int64_t M = s.B * s.nA, stride = int64_t(gridDim.x) * TPB;
    const F4* y = reinterpret_cast<const F4*>(p.y4);
    const F4* zi = reinterpret_cast<const F4*>(p.z_inject);
    F4* zo = reinterpret_cast<F4*>(p.z_out);
    const uint64_t seq = p.seq + (p.seq_base ? *p.seq_base : 0ull);
    for (int64_t r = int64_t(blockIdx.x) * TPB + threadIdx.x; r < M; r += stride) {
        const int64_t b = r / s.nA;
        const int j = int(r - b * s.nA);
        F4 z;
        if (zi) {
            z = zi[r];
        } else {
            const float4 n4 = bsx_actor::normals4(p.seed, seq, uint64_t(r), SAC_SALT);
            z = F4{n4.x, n4.y, n4.z, n4.w};
        }
        const F4 mu = y[r];
        const float l0 = p.log_std[3 * j], l1 = p.log_std[3 * j + 1], l2 = p.log_std[3 * j + 2];
        const float a0 = fmaf(expf(l0), z[0], mu[0]), a1 = fmaf(expf(l1), z[1], mu[1]), a2 = fmaf(expf(l2), z[2], mu[2]);
        const float q = (fmaf(-0.5f * z[0], z[0], -l0) + fmaf(-0.5f * z[1], z[1], -l1)) + fmaf(-0.5f * z[2], z[2], -l2);
        p.logp[r] = q - 3.0f * bsx_actor::HALF_LOG_2PI;
        if (zo) zo[r] = F4{z[0], z[1], z[2], 0.0f};
        // central without own_only: slot j of every row (b, i); central with it: slot j of row (b, j); own: the row's own columns
        store_actions(action_slot(s, p.x, b, j, r, s.central && !p.own_only), s.Dc, 3, a0, a1, a2, 0.0f);
    }
}

struct HeadArgs {
    BsxSacIo io;
    int64_t M, tiles;
    int J, nA;
    float gamma, s2;                           // s2 = float(2.0 / B)
    double* part;                              // workspace: [blocks][STAT_COLS] partial rows
};

template <int WEIGHT>                          // 1: io.weight is given
__global__ __launch_bounds__(TPB) void bsx_sac_head_kernel(const HeadArgs p) {
    const BsxSacIo& io = p.io;
    td_head_pass<HEAD_SOFT, WEIGHT>(HeadView{io.q1, io.q2, io.q1_next, io.q2_next, io.logp_next, io.log_alpha, io.rew, io.done, io.weight, io.g_q1,
                                             io.g_q2, nullptr, io.td, p.M, p.tiles, p.J, p.nA, p.gamma, 0.0f, p.s2, p.part});
}

__global__ __launch_bounds__(TPB) void bsx_sac_seed_kernel(const float* q1, const float* q2, const float* weight, int64_t M, float s1, float* g_pi1,
                                                           float* g_pi2) {
    const int64_t stride = int64_t(gridDim.x) * TPB;
    F4* g1 = reinterpret_cast<F4*>(g_pi1);
    F4* g2 = reinterpret_cast<F4*>(g_pi2);
    for (int64_t i = int64_t(blockIdx.x) * TPB + threadIdx.x; i < M; i += stride) {
        const float a = q1[i], b = q2[i];
        const bool first = a < b || a != a;                        // the head's rule for m
        const float seed = -((weight ? weight[i] : 1.0f) * s1);
        F4 o1 = F4(0.0f), o2 = F4(0.0f);
        if (first) o1[0] = seed;
        else o2[0] = seed;
        g1[i] = o1;
        g2[i] = o2;
    }
}

struct PiPlan {                                // policy_grad's launch shape: a function of (B, nA) alone
    int64_t M, tiles, blocks;
    int S, J, C;                               // S: elements per tile, a multiple of nA;  C: doubles per partial row
};

inline PiPlan pi_plan_of(int64_t B, int nA) {
    PiPlan p;
    p.M = B * nA;
    p.S = (TPB / nA) * nA;
    p.tiles = (p.M + p.S - 1) / p.S;
    const int64_t J = (p.tiles + HEAD_MAX_BLOCKS - 1) / HEAD_MAX_BLOCKS;
    p.blocks = (p.tiles + J - 1) / J;
    p.J = int(J);
    p.C = STAT_COLS + AG * nA;
    return p;
}

struct PiArgs {
    BsxSacPolicyIo io;
    Shape s;
    int64_t M, tiles;
    int S, J, C;
    float s1, target_entropy;                  // s1 = float(1.0 / B)
    double* part;                              // workspace: [blocks][C] partial rows
};

template <int WEIGHT>
__global__ __launch_bounds__(TPB) void bsx_sac_policy_kernel(const PiArgs p) {
    __shared__ double s_w[NP][WAVES];
    __shared__ double s_ag[AG][TPB];
    __shared__ double s_lp[TPB];                                   // [P][AG nA], AG nA P <= 256
    const int tid = threadIdx.x, nA = p.s.nA;
    const int a = tid % nA;                                        // a tile starts at a multiple of nA: the thread's agent in every tile
    double acc[NP] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double ag[AG] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const float l0 = p.io.log_std[3 * a], l1 = p.io.log_std[3 * a + 1], l2 = p.io.log_std[3 * a + 2];
    const float sd0 = expf(l0), sd1 = expf(l1), sd2 = expf(l2);
    const float alpha = expf(p.io.log_alpha[a]);
    const F4* z4 = reinterpret_cast<const F4*>(p.io.z);
    F4* ga4 = reinterpret_cast<F4*>(p.io.g_a4);
    const int64_t tile0 = int64_t(blockIdx.x) * p.J, col = p.s.W + (p.s.central ? a * p.s.k : 0);
    for (int j = 0; j < p.J; ++j) {
        const int64_t tile = tile0 + j, i = tile * p.S + tid;
        if (tid >= p.S || tile >= p.tiles || i >= p.M) continue;
        const float* g1 = p.io.gx1 + i * p.s.Dc + col;
        const float* g2 = p.io.gx2 + i * p.s.Dc + col;
        const float g0 = g1[0] + g2[0], g1c = g1[1] + g2[1], g2c = g1[2] + g2[2];
        ga4[i] = F4{g0, g1c, g2c, 0.0f};
        const F4 z = z4[i];
        const float w = WEIGHT ? p.io.weight[i] : 1.0f, ws = w * p.s1;
        const float lp = p.io.logp[i], qa = p.io.q1_pi[i], qb = p.io.q2_pi[i];
        const bool first = qa < qb || qa != qa;
        const float m = first ? qa : qb;
        ag[0] += double(g0 * (sd0 * z[0]));
        ag[1] += double(g1c * (sd1 * z[1]));
        ag[2] += double(g2c * (sd2 * z[2]));
        ag[3] += double(ws);
        ag[4] += double(ws * (lp + p.target_entropy));
        acc[0] += double(w * fmaf(alpha, lp, -m));
        acc[1] += double(m);
        acc[2] += double(lp);
        acc[3] += double(alpha);
        acc[4] += double(w);
        acc[5] += first ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < AG; ++k) s_ag[k][tid] = ag[k];
    double sum[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) sum[c] = block_sum<double, WAVES>(acc[c], s_w[c]);     // (its barrier also publishes s_ag)
    double* row = p.part + int64_t(blockIdx.x) * p.C;
    if (tid < STAT_COLS) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < NP; ++c) t = tid == c + 1 ? sum[c] : t;
        row[tid] = t;
    }
    // agent i's threads are i, i + nA, ..: P threads per (agent, term) add every P-th of them in order, one adds the P parts
    const int per = p.S / nA, cols = AG * nA;
    int P = TPB / cols;
    P = P > LS_PARTS_MAX ? LS_PARTS_MAX : P;                        // cols <= 80: P >= 3
    if (tid < cols * P) {
        const int part = tid / cols, c = tid % cols, i = c / AG, k = c % AG;
        double t = 0.0;
        for (int m = part; m < per; m += P) t += s_ag[k][i + nA * m];
        s_lp[part * cols + c] = t;
    }
    __syncthreads();
    if (tid < cols) {
        double t = 0.0;
        for (int q = 0; q < P; ++q) t += s_lp[q * cols + tid];
        row[STAT_COLS + tid] = t;
    }
}

// one element of Adam as bsx_adam_step_mlp takes it (bsx_adam_step.hip: adam_element and the scalars of its norm pass), without a clip
// coefficient: m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= step_size m / (sqrt(v) / sqrt(1 - b2^t) + eps)
__device__ inline float adam_element(const float* hyper, int64_t t, float g, float& m, float& v, float p) {
    const double lr = double(hyper[0]), b1 = double(hyper[1]), b2 = double(hyper[2]);
    const float step_size = float(lr / (1.0 - pow(b1, double(t)))), bc2_sqrt = float(sqrt(1.0 - pow(b2, double(t))));
    const float fb1 = float(b1), omb1 = float(1.0 - b1), fb2 = float(b2), omb2 = float(1.0 - b2), eps = hyper[3];
    m = fb1 * m + omb1 * g;
    v = fb2 * v + omb2 * (g * g);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    return p - step_size * (m / denom);
}

// Q = 1024 / C threads per column; thread (q, c) adds the partial rows q, q + Q, .. in order; then min(Q, 16) threads per column add
// every 16th of those sums, and one thread the rest -- a fixed order throughout.  Then the gradients, and log_alpha's step
__global__ __launch_bounds__(MERGE_TPB) void bsx_sac_policy_merge_kernel(const BsxSacPolicyIo io, const double* part, int64_t blocks, int C, int nA,
                                                                         int64_t M, double* stats) {
    __shared__ double s_q[MERGE_TPB], s_r[MERGE_TPB], s_t[STAT_COLS + AG * BSX_MAX_N];
    const int tid = threadIdx.x;
    const int Q = MERGE_TPB / C, c = tid % C, q = tid / C, G = Q < 16 ? Q : 16;
    if (q < Q) {
        double t = 0.0;
        for (int64_t b = q; b < blocks; b += Q) t += part[b * C + c];
        s_q[q * C + c] = t;
    }
    __syncthreads();
    if (q < G) {
        double t = 0.0;
        for (int k = q; k < Q; k += G) t += s_q[k * C + c];
        s_r[q * C + c] = t;
    }
    __syncthreads();
    if (tid < C) {
        double t = 0.0;
        for (int k = 0; k < G; ++k) t += s_r[k * C + tid];
        s_t[tid] = t;
    }
    // log_alpha and the step word are read by every thread that needs them BEFORE the barrier; the step writes them after it
    const float la3 = tid < 3 * nA ? io.log_alpha[tid / 3] : 0.0f;
    const float la = tid < nA ? io.log_alpha[tid] : 0.0f;
    const int64_t t1 = io.step ? *io.step + 1 : 0;
    __syncthreads();
    if (tid < STAT_COLS) stats[tid] = tid == 0 ? double(M) : (tid == STAT_COLS - 1 ? 0.0 : s_t[tid] / double(M));
    if (tid < 3 * nA) {
        const int i = tid / 3, k = tid - 3 * i;
        io.g_log_std[tid] = float(s_t[STAT_COLS + AG * i + k] - double(expf(la3)) * s_t[STAT_COLS + AG * i + 3]);
    }
    if (tid < nA) {
        const float g = float(-s_t[STAT_COLS + AG * tid + 4]);
        io.g_log_alpha[tid] = g;
        if (io.step) {
            float m = io.alpha_m[tid], v = io.alpha_v[tid];
            const float x = adam_element(io.hyper, t1, g, m, v, la);
            io.alpha_m[tid] = m;
            io.alpha_v[tid] = v;
            io.log_alpha[tid] = x;
            if (tid == 0) *io.step = t1;
        }
    }
}

inline bool sac_shape(int64_t B, int nA, int Do, int k, int central, Shape* s) { return k == 3 && shape_of(B, nA, Do, k, central, s); }

}  // namespace

extern "C" {

int bsx_sac_sample_actions(const float* y4, const float* log_std, int64_t B, int nA, int Do, int k, int central, int own_only, uint64_t seed,
                           uint64_t seq, const uint64_t* seq_base, const float* z_inject, float* x, float* logp, float* z_out, void* stream) {
    Shape s;
    if (!y4 || !log_std || !x || !logp || (own_only != 0 && own_only != 1)) return BSX_E_ARG;
    if (!sac_shape(B, nA, Do, k, central, &s)) return BSX_E_ARG;
    if (!aligned(y4, 16) || !aligned(z_inject, 16) || !aligned(z_out, 16)) return BSX_E_ALIGN;
    if (!aligned(log_std, 4) || !aligned(x, 4) || !aligned(logp, 4) || !aligned(seq_base, 8)) return BSX_E_ALIGN;
    const SampleArgs a{y4, log_std, z_inject, seq_base, x, logp, z_out, seed, seq, own_only};
    hipLaunchKernelGGL(bsx_sac_sample_kernel, dim3(copy_blocks(s.B * s.nA)), dim3(TPB), 0, static_cast<hipStream_t>(stream), a, s);
    return int(hipGetLastError());
}

int bsx_sac_head_workspace_bytes(int64_t B, int nA, size_t* bytes) { return head_workspace_bytes(B, nA, bytes); }

int bsx_sac_head(const BsxSacIo* io, int64_t B, int nA, float gamma, void* workspace, double* stats, void* stream) {
    if (!io || !io->q1 || !io->q2 || !io->q1_next || !io->q2_next || !io->logp_next || !io->rew || !io->done || !io->log_alpha || !io->g_q1 ||
        !io->g_q2)
        return BSX_E_ARG;
    if (!head_ranges(gamma, B, nA, workspace, stats)) return BSX_E_ARG;
    if (!aligned(io->g_q1, 16) || !aligned(io->g_q2, 16)) return BSX_E_ALIGN;
    if (!aligned(io->q1, 4) || !aligned(io->q2, 4) || !aligned(io->q1_next, 4) || !aligned(io->q2_next, 4) || !aligned(io->logp_next, 4) ||
        !aligned(io->rew, 4) || !aligned(io->weight, 4) || !aligned(io->log_alpha, 4) || !aligned(io->td, 4))
        return BSX_E_ALIGN;
    const HeadArgs a{*io, 0, 0, 0, nA, gamma, float(2.0 / double(B)), nullptr};
    return launch_head<true>(bsx_sac_head_kernel<1>, bsx_sac_head_kernel<0>, io->weight != nullptr, a, B, nA, workspace, stats, stream);
}

int bsx_sac_policy_seed(const float* q1_pi, const float* q2_pi, const float* weight, int64_t B, int nA, float* g_pi1, float* g_pi2, void* stream) {
    if (!q1_pi || !q2_pi || !g_pi1 || !g_pi2) return BSX_E_ARG;
    if (!td_shape(B, nA)) return BSX_E_ARG;
    if (!aligned(g_pi1, 16) || !aligned(g_pi2, 16)) return BSX_E_ALIGN;
    if (!aligned(q1_pi, 4) || !aligned(q2_pi, 4) || !aligned(weight, 4)) return BSX_E_ALIGN;
    hipLaunchKernelGGL(bsx_sac_seed_kernel, dim3(copy_blocks(B * nA)), dim3(TPB), 0, static_cast<hipStream_t>(stream), q1_pi, q2_pi, weight,
                       B * nA, float(1.0 / double(B)), g_pi1, g_pi2);
    return int(hipGetLastError());
}

int bsx_sac_policy_grad_workspace_bytes(int64_t B, int nA, size_t* bytes) {
    if (!bytes || !td_shape(B, nA)) return BSX_E_ARG;
    const PiPlan p = pi_plan_of(B, nA);
    *bytes = size_t(p.blocks) * size_t(p.C) * 8;
    return 0;
}

int bsx_sac_policy_grad(const BsxSacPolicyIo* io, int64_t B, int nA, int Do, int k, int central, float target_entropy, void* workspace,
                        double* stats, void* stream) {
    Shape sh;
    if (!io || !io->gx1 || !io->gx2 || !io->z || !io->logp || !io->q1_pi || !io->q2_pi || !io->log_std || !io->log_alpha || !io->g_a4 ||
        !io->g_log_std || !io->g_log_alpha || !workspace || !stats)
        return BSX_E_ARG;
    if (!sac_shape(B, nA, Do, k, central, &sh)) return BSX_E_ARG;
    if (!(fabsf(target_entropy) <= 3.0e38f)) return BSX_E_ARG;                 // NaN and infinities
    const int given = (io->alpha_m != nullptr) + (io->alpha_v != nullptr) + (io->hyper != nullptr) + (io->step != nullptr);
    if (given != 0 && given != 4) return BSX_E_ARG;
    if (!aligned(io->z, 16) || !aligned(io->g_a4, 16)) return BSX_E_ALIGN;
    if (!aligned(io->gx1, 4) || !aligned(io->gx2, 4) || !aligned(io->logp, 4) || !aligned(io->q1_pi, 4) || !aligned(io->q2_pi, 4) ||
        !aligned(io->weight, 4) || !aligned(io->log_std, 4) || !aligned(io->log_alpha, 4) || !aligned(io->g_log_std, 4) ||
        !aligned(io->g_log_alpha, 4) || !aligned(io->alpha_m, 4) || !aligned(io->alpha_v, 4) || !aligned(io->hyper, 4))
        return BSX_E_ALIGN;
    if (!aligned(workspace, 8) || !aligned(stats, 8) || !aligned(io->step, 8)) return BSX_E_ALIGN;
    const PiPlan p = pi_plan_of(B, nA);
    double* part = static_cast<double*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PiArgs a{*io, sh, p.M, p.tiles, p.S, p.J, p.C, float(1.0 / double(B)), target_entropy, part};
    if (io->weight) hipLaunchKernelGGL(bsx_sac_policy_kernel<1>, dim3(unsigned(p.blocks)), dim3(TPB), 0, s, a);
    else hipLaunchKernelGGL(bsx_sac_policy_kernel<0>, dim3(unsigned(p.blocks)), dim3(TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(bsx_sac_policy_merge_kernel, dim3(1), dim3(MERGE_TPB), 0, s, *io, static_cast<const double*>(part), p.blocks, p.C, nA, p.M,
                       stats);
    return int(hipGetLastError());
}

}  // extern "C"
