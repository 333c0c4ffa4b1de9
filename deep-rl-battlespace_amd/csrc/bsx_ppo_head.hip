// bsx_ppo_head.hip -- the PPO loss head between the actor's fused forward and its fused backward (include/battlespace_hip.h: bsx_ppo_head*), gfx950.
//
// From the forward's outputs (y, v) and a rollout's records (rec, logp_old, adv, ret, mask[, v_old]) to the two grad_out tensors
// bsx_actor_grad takes (g_pi, g_v), log_std's gradient and the loss statistics, in ONE pass over the R*A elements: 86 bytes of traffic per
// element and nothing saved, where the torch composition runs several dozen element-wise passes and keeps their intermediates for autograd.
//   1. count -- the elements with mask != 0, as integer partial counts of up to 256 workgroups (16 mask bytes per lane and load);
//   2. head  -- one thread per element and tile: a workgroup's 256 threads cover tiles of S = (256 / A) A consecutive elements (S a multiple of
//               A: thread t is agent t % A in every tile, whatever A -- 6, 10, .. are no powers of two), J consecutive tiles each.  Every
//               workgroup adds the partial counts to N first.  16-byte loads of y / rec, 16-byte stores of g_pi / g_v; the per-row
//               float32 terms of the statistics and of log_std's gradient are added in float64, per thread over its J tiles, then
//               across the workgroup in a fixed order (shuffle tree + LDS; log_std per agent through LDS), and stored to the workspace;
//   3. merge -- ONE workgroup adds the workgroups' partial rows in a fixed order and writes stats and g_log_std.
// No floating-point atomics, no flags or spins; the grid is a function of (R, A) alone: the same inputs give the same bits on every call.

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
constexpr int COUNT_MAX_BLOCKS = 256;          // partial counts: one per thread of a head workgroup
constexpr int64_t COUNT_BYTES_PER_BLOCK = 16 * TPB * 4;
constexpr int64_t HEAD_MAX_BLOCKS = 2048;
constexpr int STAT_COLS = 8;                   // a partial row: 0 | loss | -surr | lv | H | kl | clipped | 0 | log_std sums [A][3]
constexpr int LS_PARTS_MAX = 8;
constexpr float LOG_2PI = 1.8378770664093453f;
constexpr double LOG_2PI_64 = 1.8378770664093453;

typedef float F4 __attribute__((ext_vector_type(4)));

struct Plan {                                  // the launch shape: a function of (R, A) alone
    int64_t M, tiles, blocks;                  // elements, tiles of S elements, head workgroups
    int S, J, count_blocks;
};

Plan plan_of(int64_t R, int A) {
    Plan p;
    p.M = R * A;
    p.S = (TPB / A) * A;
    p.tiles = (p.M + p.S - 1) / p.S;
    const int64_t J = (p.tiles + HEAD_MAX_BLOCKS - 1) / HEAD_MAX_BLOCKS;     // one tile per workgroup up to 2 048 workgroups (eight per CU), then more tiles each
    p.blocks = (p.tiles + J - 1) / J;
    p.J = int(J);
    const int64_t cb = (p.M + COUNT_BYTES_PER_BLOCK - 1) / COUNT_BYTES_PER_BLOCK;
    p.count_blocks = int(cb < COUNT_MAX_BLOCKS ? cb : COUNT_MAX_BLOCKS);
    return p;
}

struct HeadArgs {
    BsxPpoIo io;
    int64_t M, tiles;
    int S, J, A, count_blocks;
    float temperature, lo, hi, vclip, c_v, c_e;   // lo = 1 - clip, hi = 1 + clip
    const int64_t* counts;                        // workspace: [COUNT_MAX_BLOCKS] partial counts
    double* part;                                 // workspace: [blocks][STAT_COLS + 3 A] partial rows
};

__device__ inline uint32_t nonzero_bytes(uint32_t x) {
    x = (x | (x >> 4)) & 0x0f0f0f0fu;
    x = (x | (x >> 2)) & 0x03030303u;
    x = (x | (x >> 1)) & 0x01010101u;
    return __popc(x);
}

// (e^x - 1) - x, the approximate KL of a row with log ratio x, without the cancellation against 1 and x: x^2 (1/2 + x/6 + .. + x^8/10!)
// for |x| < 1/2 (the first term left out is below 1e-9 of the result), expm1f(x) - x beyond
__device__ inline float kl_term(float x) {
    if (!(fabsf(x) < 0.5f)) return expm1f(x) - x;
    float q = 1.0f / 3628800.0f;
    q = q * x + 1.0f / 362880.0f;
    q = q * x + 1.0f / 40320.0f;
    q = q * x + 1.0f / 5040.0f;
    q = q * x + 1.0f / 720.0f;
    q = q * x + 1.0f / 120.0f;
    q = q * x + 1.0f / 24.0f;
    q = q * x + 1.0f / 6.0f;
    q = q * x + 0.5f;
    return (x * x) * q;
}

__global__ __launch_bounds__(TPB) void bsx_ppo_count_kernel(const uint8_t* mask, int64_t M, int64_t* counts) {
    __shared__ int64_t s_w[WAVES];
    const int64_t g = int64_t(blockIdx.x) * TPB + threadIdx.x, stride = int64_t(gridDim.x) * TPB;
    int64_t head = int64_t((16 - (reinterpret_cast<uintptr_t>(mask) & 15)) & 15);      // bytes before the first 16-byte boundary
    if (head > M) head = M;
    const int64_t groups = (M - head) / 16, tail0 = head + groups * 16;
    int64_t n = 0;
    if (g < head) n += mask[g] != 0;
    const uint4* body = reinterpret_cast<const uint4*>(mask + head);
    for (int64_t k = g; k < groups; k += stride) {
        const uint4 q = body[k];
        n += nonzero_bytes(q.x) + nonzero_bytes(q.y) + nonzero_bytes(q.z) + nonzero_bytes(q.w);
    }
    if (g < M - tail0) n += mask[tail0 + g] != 0;
    n = block_sum<int64_t, WAVES>(n, s_w);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// MODE = kind + 2 * (v_old given)
template <int MODE>
__global__ __launch_bounds__(TPB) void bsx_ppo_head_kernel(const HeadArgs p) {
    constexpr bool GAUSS = (MODE & 1) != 0, VOLD = (MODE & 2) != 0;
    constexpr int NS = 6;
    __shared__ int64_t s_cnt[WAVES];
    __shared__ double s_stat[WAVES][NS];
    __shared__ double s_ls[GAUSS ? 3 : 1][GAUSS ? TPB : 1];
    __shared__ double s_lp[GAUSS ? TPB : 1];                 // [P][3 A], 3 A P <= 256
    const int tid = threadIdx.x;
    const int64_t N = block_sum<int64_t, WAVES>(tid < p.count_blocks ? p.counts[tid] : 0, s_cnt);
    const double inv_n = N > 0 ? 1.0 / double(N) : 0.0;
    const bool lane_on = tid < p.S;
    const int a = tid % p.A;
    // the Gaussian log-probability is a sum of terms of size z^2 / 2: in float32 it would carry ~1e-6 into the ratio's exponent, so z,
    // z^2, the sum and its difference to logp_old are float64 (1 / sigma once per thread); everything from the ratio on is float32
    float ls[3] = {0.0f, 0.0f, 0.0f}, ent = 0.0f;
    double inv_sd[3] = {0.0, 0.0, 0.0};
    if constexpr (GAUSS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ls[k] = p.io.log_std[3 * a + k];
            inv_sd[k] = exp(-double(ls[k]));
        }
        ent = ((ls[0] + ls[1]) + ls[2]) + 1.5f * (1.0f + LOG_2PI);
    }
    double acc[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, acc_ls[3] = {0.0, 0.0, 0.0};
    const F4* y4 = reinterpret_cast<const F4*>(p.io.y);
    const F4* rec4 = reinterpret_cast<const F4*>(p.io.rec);
    F4* gpi4 = reinterpret_cast<F4*>(p.io.g_pi);
    F4* gv4 = reinterpret_cast<F4*>(p.io.g_v);
    const int64_t tile0 = int64_t(blockIdx.x) * p.J;
    for (int j = 0; j < p.J; ++j) {
        const int64_t tile = tile0 + j, i = tile * p.S + tid;
        if (tile >= p.tiles || !lane_on || i >= p.M) continue;
        const F4 y = y4[i], rec = rec4[i];
        const float v = p.io.v[i], lp_old = p.io.logp_old[i], adv = p.io.adv[i], ret = p.io.ret[i];
        const bool on = p.io.mask[i] != 0;
        float lr, H, dl[4], dh[4] = {0.0f, 0.0f, 0.0f, 0.0f}, zz[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (GAUSS) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double z = (double(rec[k]) - double(y[k])) * inv_sd[k], z2 = z * z;
                zz[k] = float(z2);
                s += -0.5 * z2 - double(ls[k]);
                dl[k] = float(z * inv_sd[k]);
            }
            dl[3] = 0.0f;
            lr = float((s - 1.5 * LOG_2PI_64) - double(lp_old));
            H = ent;
        } else {
            float logp;
            float s[4], e[4], lp[4], pr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = y[k] / p.temperature;
            const float m = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k) { s[k] -= m; e[k] = expf(s[k]); }
            const float lse = logf((e[0] + e[1]) + (e[2] + e[3]));
            float best = rec[0];
            logp = s[0] - lse;
            int star = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lp[k] = s[k] - lse;
                pr[k] = expf(lp[k]);
                if (k > 0 && rec[k] > best) { best = rec[k]; star = k; logp = lp[k]; }     // the FIRST maximum
            }
            H = -((pr[0] * lp[0] + pr[1] * lp[1]) + (pr[2] * lp[2] + pr[3] * lp[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                dl[k] = ((k == star ? 1.0f : 0.0f) - pr[k]) / p.temperature;
                dh[k] = -pr[k] * (lp[k] + H) / p.temperature;
            }
            lr = logp - lp_old;
        }
        const float ratio = expf(lr);
        const float cr = fminf(fmaxf(ratio, p.lo), p.hi);
        const float surr = fminf(ratio * adv, cr * adv);
        const bool clipped = (adv > 0.0f && ratio > p.hi) || (adv < 0.0f && ratio < p.lo);
        const float ds = clipped ? 0.0f : ratio * adv;
        const float d = v - ret;
        float lv = 0.5f * (d * d), dlv = d;
        if constexpr (VOLD) {
            const float vo = p.io.v_old[i], dv = v - vo;
            const float vc = vo + fminf(fmaxf(dv, -p.vclip), p.vclip), dc = vc - ret;
            if (fabsf(dv) > p.vclip && dc * dc > d * d) { lv = 0.5f * (dc * dc); dlv = 0.0f; }
        }
        const float loss = (-surr + p.c_v * lv) - p.c_e * H;
        F4 gp, gv = F4(0.0f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = -ds * dl[k] - p.c_e * dh[k];
            gp[k] = on ? float(double(t) * inv_n) : 0.0f;                                  // select, never multiply: a masked-out NaN stays out
        }
        if constexpr (GAUSS) gp[3] = 0.0f;
        gv[0] = on ? float(double(p.c_v * dlv) * inv_n) : 0.0f;
        gpi4[i] = gp;
        gv4[i] = gv;
        if (on) {
            acc[0] += double(loss); acc[1] += double(-surr); acc[2] += double(lv); acc[3] += double(H);
            acc[4] += double(kl_term(lr)); acc[5] += clipped ? 1.0 : 0.0;
            if constexpr (GAUSS) {
#pragma unroll
                for (int k = 0; k < 3; ++k) acc_ls[k] += double(-ds * (zz[k] - 1.0f) - p.c_e);
            }
        }
    }
    // the statistics: a fixed tree over the wave, then the four waves in order
#pragma unroll
    for (int c = 0; c < NS; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NS; ++c) s_stat[tid >> 6][c] = acc[c];
    }
    if constexpr (GAUSS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s_ls[k][tid] = acc_ls[k];
    }
    __syncthreads();
    const int C = STAT_COLS + (GAUSS ? 3 * p.A : 0);
    double* row = p.part + int64_t(blockIdx.x) * C;
    if (tid < STAT_COLS) {
        double t = 0.0;
        if (tid >= 1 && tid <= NS) t = ((s_stat[0][tid - 1] + s_stat[1][tid - 1]) + s_stat[2][tid - 1]) + s_stat[3][tid - 1];
        row[tid] = t;
    }
    if constexpr (GAUSS) {
        // log_std: agent a's threads are a, a + A, ..: P threads per (agent, column) add every P-th of them, one adds the P parts
        const int per = p.S / p.A, cols = 3 * p.A;
        int P = TPB / cols;
        P = P < 1 ? 1 : (P > LS_PARTS_MAX ? LS_PARTS_MAX : P);
        if (tid < cols * P) {
            const int part = tid / cols, c = tid % cols, ag = c / 3, k = c % 3;
            double t = 0.0;
            for (int m = part; m < per; m += P) t += s_ls[k][ag + p.A * m];
            s_lp[part * cols + c] = t;
        }
        __syncthreads();
        if (tid < cols) {
            double t = 0.0;
            for (int q = 0; q < P; ++q) t += s_lp[q * cols + tid];
            row[STAT_COLS + tid] = t;
        }
    }
}

// Q = 1024 / C threads per column; thread (q, c) adds the partial rows q, q + Q, .. (four loads in flight, added pairwise); then min(Q, 16)
// threads per column add every 16th of those sums, and one thread the rest -- a fixed order throughout
__global__ __launch_bounds__(MERGE_TPB) void bsx_ppo_merge_kernel(const int64_t* counts, int count_blocks, const double* part, int64_t blocks, int C,
                                                                  double* stats, float* g_log_std) {
    __shared__ int64_t s_cnt[MERGE_TPB / 64];
    __shared__ double s_q[MERGE_TPB], s_r[MERGE_TPB];
    const int tid = threadIdx.x;
    const int64_t N = block_sum<int64_t, MERGE_TPB / 64>(tid < count_blocks ? counts[tid] : 0, s_cnt);
    const int Q = MERGE_TPB / C, c = tid % C, q = tid / C, G = Q < 16 ? Q : 16;
    if (q < Q) {
        double t = 0.0;
        int64_t b = q;
        for (; b + 3 * Q < blocks; b += 4 * Q) {
            const double p0 = part[b * C + c], p1 = part[(b + Q) * C + c], p2 = part[(b + 2 * Q) * C + c], p3 = part[(b + 3 * Q) * C + c];
            t += (p0 + p1) + (p2 + p3);
        }
        for (; b < blocks; b += Q) t += part[b * C + c];
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
        const double mean = N > 0 ? t / double(N) : 0.0;
        if (tid == 0) stats[0] = double(N);
        else if (tid == STAT_COLS - 1) stats[tid] = 0.0;
        else if (tid < STAT_COLS) stats[tid] = mean;
        else g_log_std[tid - STAT_COLS] = float(mean);
    }
}

bool bad_share(float x) { return !(x > 0.0f && x < 1.0f); }          // NaN too
bool bad_weight(float x) { return !(x >= 0.0f && x <= 3.0e38f); }    // NaN, negative, infinite
bool bad_positive(float x) { return !(x > 0.0f && x <= 3.0e38f); }

template <int MODE>
void launch_head(const HeadArgs& a, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(bsx_ppo_head_kernel<MODE>, dim3(unsigned(blocks)), dim3(TPB), 0, s, a);
}

}  // namespace

extern "C" {

int bsx_ppo_head_workspace_bytes(int64_t R, int A, size_t* bytes) {
    if (!bytes || R < 1 || R > BSX_MAX_E || A < 2 || A % 2 != 0 || A / 2 > BSX_MAX_N) return BSX_E_ARG;
    const Plan p = plan_of(R, A);
    *bytes = size_t(8 * COUNT_MAX_BLOCKS) + size_t(p.blocks) * size_t(STAT_COLS + 3 * A) * 8;
    return 0;
}

int bsx_ppo_head(const BsxPpoIo* io, int64_t R, int A, int kind, float temperature, float clip, float vclip, float c_v, float c_e,
                 void* workspace, double* stats, void* stream) {
    if (!io || !io->y || !io->v || !io->rec || !io->logp_old || !io->adv || !io->ret || !io->mask || !io->g_pi || !io->g_v || !workspace || !stats)
        return BSX_E_ARG;
    if (kind != 0 && kind != 1) return BSX_E_ARG;
    if (bad_share(clip) || bad_weight(c_v) || bad_weight(c_e) || (kind == 0 && bad_positive(temperature)) || (io->v_old && bad_positive(vclip)))
        return BSX_E_ARG;
    if (R < 1 || R > BSX_MAX_E || A < 2 || A % 2 != 0 || A / 2 > BSX_MAX_N) return BSX_E_ARG;
    if (kind == 1 && (!io->log_std || !io->g_log_std)) return BSX_E_ARG;
    if (!aligned(io->y, 16) || !aligned(io->rec, 16) || !aligned(io->g_pi, 16) || !aligned(io->g_v, 16)) return BSX_E_ALIGN;
    if (!aligned(io->v, 4) || !aligned(io->logp_old, 4) || !aligned(io->adv, 4) || !aligned(io->ret, 4) || !aligned(io->v_old, 4)) return BSX_E_ALIGN;
    if (kind == 1 && (!aligned(io->log_std, 4) || !aligned(io->g_log_std, 4))) return BSX_E_ALIGN;
    if (!aligned(workspace, 8) || !aligned(stats, 8)) return BSX_E_ALIGN;
    const Plan p = plan_of(R, A);
    int64_t* counts = static_cast<int64_t*>(workspace);
    double* part = reinterpret_cast<double*>(counts + COUNT_MAX_BLOCKS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bsx_ppo_count_kernel, dim3(unsigned(p.count_blocks)), dim3(TPB), 0, s, io->mask, p.M, counts);
    if (const hipError_t e = hipGetLastError()) return int(e);
    HeadArgs a{*io, p.M, p.tiles, p.S, p.J, A, p.count_blocks, temperature, 1.0f - clip, 1.0f + clip, vclip, c_v, c_e, counts, part};
    switch (kind + (io->v_old ? 2 : 0)) {
        case 0: launch_head<0>(a, p.blocks, s); break;
        case 1: launch_head<1>(a, p.blocks, s); break;
        case 2: launch_head<2>(a, p.blocks, s); break;
        default: launch_head<3>(a, p.blocks, s); break;
    }
    if (const hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(bsx_ppo_merge_kernel, dim3(1), dim3(MERGE_TPB), 0, s, static_cast<const int64_t*>(counts), p.count_blocks,
                       static_cast<const double*>(part), p.blocks, STAT_COLS + (kind == 1 ? 3 * A : 0), stats, io->g_log_std);
    return int(hipGetLastError());
}

}  // extern "C"
