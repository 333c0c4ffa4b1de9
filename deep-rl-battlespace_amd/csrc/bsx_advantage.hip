// bsx_advantage.hip -- GAE(gamma, lambda) advantages and returns over a rollout's records, on device (include/battlespace_hip.h: bsx_gae*), gfx950.
//
// The on-policy counterpart of bsx_replay.hip: what a PPO update needs from a PolicyRollout's [T][E][A] records (rew, value, done,
// env_done) plus V(obs[T]), computed inside the rollout's graph with no host round trip.  The recurrence runs backwards over T, so a lane
// owns W adjacent columns (agent rows e*A + a) for all T ticks and walks them from T-1 down to 0:
// bsx_gae_agents adds a per-agent flag to the mask (a scripted opponent's agents have no decisions); bsx_gae is that call with no flag.
//   1. gae    -- (bsx_gae_kernel; bsx_gae_stats_kernel with normalisation) one wavefront per 64*W columns.  Each lane loads W columns at a time (f32 x W, u8 x W: 1 KiB / 256 B per wave instruction
//               at W = 4) and issues the loads of U ticks before the dependent adv chain consumes them.  With normalisation it also
//               reduces the masked advantages of its tile to (n, mean, M2) in float64 (per-chunk moments merged by Chan's formula, then a
//               fixed shuffle tree across the wave) and stores them to the workspace;
//   2. merge  -- ONE workgroup merges the tile partials in a fixed order and writes stats = (n, mean, unbiased std);
//   3. scale  -- adv = f32((f64(adv) - mean) / (std + 1e-8)) on the masked rows.
// No inter-workgroup flags or spins, no float atomics: a given input gives the same bits on every call and every graph replay.
// Built with -ffp-contract=off: every float32 operation of the recurrence is rounded on its own (tests/gae_util.py restates it in numpy).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"

namespace {

constexpr int WAVE = 64;          // the gae kernel's workgroup is one wavefront: 65 536 x 1v1 at W = 4 is only 512 of them, spread over all CUs
constexpr int U = 8;              // ticks whose loads are in flight ahead of the chain (~11 VGPRs each at W = 4)
constexpr int MERGE_TPB = 256;
constexpr int SCALE_TPB = 256;
constexpr int64_t SCALE_MAX_BLOCKS = 8192;

template <int W> struct Cols;     // W adjacent columns of one lane: W floats, W bytes in one word
template <> struct Cols<4> { typedef float F __attribute__((ext_vector_type(4))); typedef uint32_t B; };
template <> struct Cols<2> { typedef float F __attribute__((ext_vector_type(2))); typedef uint16_t B; };

struct GaeArgs {
    BsxGaeIo io;
    int64_t E, NW;                // games, column groups per tick (E*A / W)
    int T, A;
    float gamma, gl;              // gl = gamma * lam, rounded once
    double* part;                 // normalise: workspace [tiles][3] = (n, mean, M2) of each tile's masked advantages
    const uint8_t* agent_on;      // bsx_gae_agents: [A] flags, 0 = the actor does not play this agent (no decisions); NULL = every agent
};

__device__ inline uint32_t byte_of(uint32_t b, int j) { return (b >> (8 * j)) & 0xffu; }

// (n, mean, M2) <- the merge of itself with (nb, mb, m2b) (Chan, Golub & LeVeque); an empty side leaves the other unchanged
__device__ inline void chan_merge(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
    if (nb == 0.0) return;
    if (n == 0.0) { n = nb; mean = mb; m2 = m2b; return; }
    const double nn = n + nb, d = mb - mean;
    mean = mean + d * (nb / nn);
    m2 = (m2 + m2b) + d * d * (n * nb / nn);
    n = nn;
}

template <int W, bool NORM>
__device__ inline void gae_body(const GaeArgs& p) {
    using F = typename Cols<W>::F;
    using B = typename Cols<W>::B;
    const int64_t g = int64_t(blockIdx.x) * WAVE + threadIdx.x;     // this lane's column group: columns g*W .. g*W + W-1 of every tick
    const int64_t NW = p.NW;
    double sn = 0.0, smean = 0.0, sm2 = 0.0;                          // normalise: this lane's masked advantages so far
    if (g < NW) {
        const F* rew = reinterpret_cast<const F*>(p.io.rew) + g;
        const F* value = reinterpret_cast<const F*>(p.io.value) + g;
        const B* done = reinterpret_cast<const B*>(p.io.done) + g;
        F* adv = reinterpret_cast<F*>(p.io.adv) + g;
        F* ret = reinterpret_cast<F*>(p.io.ret) + g;
        B* mask = reinterpret_cast<B*>(p.io.mask) + g;
        B* done_prev = reinterpret_cast<B*>(p.io.done_prev) + g;
        // the W columns lie in at most two games (A >= 2 is even, W <= 4): columns j < split in game e0, the others in e1
        const int64_t c0 = g * W, e0 = c0 / p.A, e1 = (c0 + W - 1) / p.A;
        const int split = int(e1 * p.A - c0);
        const uint8_t* env_done = p.io.env_done;
        uint32_t on = 0xffffffffu;                                     // byte j: column j's agent is played by the actor
        if (p.agent_on) {
            on = 0u;
#pragma unroll
            for (int j = 0; j < W; ++j) {                              // column j's agent: (c0 + j) mod A.  One wrap is enough: c0 mod A + j <= A + 2 < 2A for A >= 4, and at A = 2 c0 (a multiple of the even W) is a multiple of A, so a = j <= 3 < 2A
                const int a = int(c0 - e0 * p.A) + j;
                on |= p.agent_on[a >= p.A ? a - p.A : a] != 0 ? 1u << (8 * j) : 0u;
            }
        }
        const float gamma = p.gamma, gl = p.gl;
        F vn = reinterpret_cast<const F*>(p.io.last_value)[g];         // value[t+1]; V(obs[T]) at t = T-1
        F an = F(0.0f);                                                // adv[t+1]; 0 at t = T-1
        const B dlast = done[int64_t(p.T - 1) * NW];
        B dn = dlast;                                                  // done[t]
        for (int t0 = p.T - 1; t0 >= 0; t0 -= U) {
            F r[U], v[U];
            B dp[U];
            uint8_t d0[U], d1[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {                              // the loads of U ticks first
                const int t = t0 - k;
                if (t >= 0) {
                    r[k] = rew[int64_t(t) * NW];
                    v[k] = value[int64_t(t) * NW];
                    dp[k] = t > 0 ? done[int64_t(t - 1) * NW] : *done_prev;      // the agent's flag before tick t
                    d0[k] = env_done[int64_t(t) * p.E + e0];
                    d1[k] = env_done[int64_t(t) * p.E + e1];
                }
            }
            F ak[U];
            B mk[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {                              // then the chain, t = t0 down to t0 - U + 1
                const int t = t0 - k;
                if (t >= 0) {
                    F a, rt;
                    B m = 0;
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const bool run = (j < split ? d0[k] : d1[k]) == 0 && byte_of(dp[k], j) == 0 && byte_of(on, j) != 0;
                        const bool term = byte_of(dn, j) != 0;
                        const float nv = term ? 0.0f : vn[j];
                        const float anj = term ? 0.0f : an[j];
                        const float delta = (r[k][j] + gamma * nv) - v[k][j];
                        const float aj = delta + gl * anj;
                        a[j] = run ? aj : 0.0f;
                        rt[j] = run ? aj + v[k][j] : 0.0f;
                        m |= B(run ? 1u << (8 * j) : 0u);
                    }
                    adv[int64_t(t) * NW] = a;
                    ret[int64_t(t) * NW] = rt;
                    mask[int64_t(t) * NW] = m;
                    an = a; vn = v[k]; dn = dp[k];
                    ak[k] = a; mk[k] = m;
                }
            }
            if constexpr (NORM) {                                      // this chunk's masked advantages: count, mean, M2, merged in
                double cn = 0.0, cs = 0.0;
#pragma unroll
                for (int k = 0; k < U; ++k)
                    if (t0 - k >= 0)
#pragma unroll
                        for (int j = 0; j < W; ++j)
                            if (byte_of(mk[k], j)) { cn += 1.0; cs += double(ak[k][j]); }
                if (cn > 0.0) {
                    const double cm = cs / cn;
                    double c2 = 0.0;
#pragma unroll
                    for (int k = 0; k < U; ++k)
                        if (t0 - k >= 0)
#pragma unroll
                            for (int j = 0; j < W; ++j)
                                if (byte_of(mk[k], j)) { const double d = double(ak[k][j]) - cm; c2 += d * d; }
                    chan_merge(sn, smean, sm2, cn, cm, c2);
                }
            }
        }
        *done_prev = dlast;                                            // the carry: the flag before tick 0 of the next call
    }
    if constexpr (NORM) {                                              // fixed tree across the wave: lane 0 ends with the tile's moments
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const double on = __shfl_down(sn, off), om = __shfl_down(smean, off), o2 = __shfl_down(sm2, off);
            chan_merge(sn, smean, sm2, on, om, o2);
        }
        if (threadIdx.x == 0) {
            double* q = p.part + 3 * int64_t(blockIdx.x);
            q[0] = sn; q[1] = smean; q[2] = sm2;
        }
    }
}

template <int W>
__global__ __launch_bounds__(WAVE) void bsx_gae_kernel(const GaeArgs p) { gae_body<W, false>(p); }

template <int W>
__global__ __launch_bounds__(WAVE) void bsx_gae_stats_kernel(const GaeArgs p) { gae_body<W, true>(p); }   // + the tile's moments

__global__ __launch_bounds__(MERGE_TPB) void bsx_gae_merge_kernel(const double* part, int64_t tiles, double* stats) {
    __shared__ double s_n[MERGE_TPB], s_m[MERGE_TPB], s_2[MERGE_TPB];
    const int tid = threadIdx.x;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int64_t i = tid; i < tiles; i += MERGE_TPB) chan_merge(n, mean, m2, part[3 * i], part[3 * i + 1], part[3 * i + 2]);
    s_n[tid] = n; s_m[tid] = mean; s_2[tid] = m2;
    __syncthreads();
    for (int off = MERGE_TPB / 2; off > 0; off >>= 1) {
        if (tid < off) {
            chan_merge(n, mean, m2, s_n[tid + off], s_m[tid + off], s_2[tid + off]);
            s_n[tid] = n; s_m[tid] = mean; s_2[tid] = m2;
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[0] = n;
        stats[1] = mean;
        stats[2] = n >= 2.0 ? sqrt(m2 / (n - 1.0)) : 0.0;
    }
}

template <int W>
__global__ __launch_bounds__(SCALE_TPB) void bsx_gae_scale_kernel(float* adv_f, const uint8_t* mask_b, int64_t groups, const double* stats) {
    using F = typename Cols<W>::F;
    using B = typename Cols<W>::B;
    if (stats[0] == 0.0) return;                                       // no masked row: nothing to scale
    const double mean = stats[1], den = stats[2] + 1e-8;
    F* adv = reinterpret_cast<F*>(adv_f);
    const B* mask = reinterpret_cast<const B*>(mask_b);
    for (int64_t g = int64_t(blockIdx.x) * SCALE_TPB + threadIdx.x; g < groups; g += int64_t(gridDim.x) * SCALE_TPB) {
        const B m = mask[g];
        if (m == 0) continue;
        F a = adv[g];
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (byte_of(m, j)) a[j] = float((double(a[j]) - mean) / den);
        adv[g] = a;
    }
}

// columns per lane: 4 where every tick's row starts on a 16-byte boundary (E*A a multiple of 4), else 2 (E*A is even)
int width_of(int64_t E, int A) { return (E * A) % 4 == 0 ? 4 : 2; }

int64_t tiles_of(int64_t E, int A) {
    const int64_t NW = E * A / width_of(E, A);
    return (NW + WAVE - 1) / WAVE;
}

bool bad_team(int A) { return A < 2 || A % 2 != 0; }                 // A = 2n; n itself is checked by check_games

bool bad_rate(float x) { return !(x >= 0.0f && x <= 1.0f); }           // NaN too

template <int W>
hipError_t launch_gae(const GaeArgs& a, int64_t tiles, bool normalize, hipStream_t s) {
    if (normalize) hipLaunchKernelGGL(bsx_gae_stats_kernel<W>, dim3(unsigned(tiles)), dim3(WAVE), 0, s, a);
    else hipLaunchKernelGGL(bsx_gae_kernel<W>, dim3(unsigned(tiles)), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int bsx_gae_workspace_bytes(int64_t E, int A, int T, size_t* bytes) {
    if (!bytes || bad_team(A) || A / 2 > BSX_MAX_N || E <= 0 || E > BSX_MAX_E || T < 1 || T > BSX_MAX_T) return BSX_E_ARG;
    *bytes = size_t(24 * tiles_of(E, A));
    return 0;
}

int bsx_gae(const BsxGaeIo* io, int T, int64_t E, int A, float gamma, float lam, int normalize, void* workspace, double* stats, void* stream) {
    return bsx_gae_agents(io, nullptr, T, E, A, gamma, lam, normalize, workspace, stats, stream);
}

int bsx_gae_agents(const BsxGaeIo* io, const uint8_t* agent_on, int T, int64_t E, int A, float gamma, float lam, int normalize, void* workspace,
                   double* stats, void* stream) {
    if (!io || !io->rew || !io->value || !io->done || !io->env_done || !io->last_value || !io->done_prev || !io->adv || !io->ret || !io->mask)
        return BSX_E_ARG;
    if (T < 1 || T > BSX_MAX_T || bad_team(A) || bad_rate(gamma) || bad_rate(lam)) return BSX_E_ARG;
    if (normalize != 0 && normalize != 1) return BSX_E_ARG;
    if (normalize && (!workspace || !stats)) return BSX_E_ARG;
    if (const int rc = check_games(io->rew, E, A / 2, 16)) return rc;
    if (!aligned(io->value, 16) || !aligned(io->last_value, 16) || !aligned(io->adv, 16) || !aligned(io->ret, 16) || !aligned(io->done, 4) ||
        !aligned(io->done_prev, 4) || !aligned(io->mask, 4) || !aligned(workspace, 8) || !aligned(stats, 8)) return BSX_E_ALIGN;
    const int W = width_of(E, A);
    const int64_t tiles = tiles_of(E, A), NW = E * A / W;
    GaeArgs a{*io, E, NW, T, A, gamma, gamma * lam, static_cast<double*>(workspace), agent_on};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = W == 4 ? launch_gae<4>(a, tiles, normalize, s) : launch_gae<2>(a, tiles, normalize, s);
    if (e || !normalize) return int(e);
    hipLaunchKernelGGL(bsx_gae_merge_kernel, dim3(1), dim3(MERGE_TPB), 0, s, static_cast<const double*>(workspace), tiles, stats);
    if (const hipError_t e2 = hipGetLastError()) return int(e2);
    const int64_t groups = int64_t(T) * NW;
    const int64_t blocks = (groups + SCALE_TPB - 1) / SCALE_TPB < SCALE_MAX_BLOCKS ? (groups + SCALE_TPB - 1) / SCALE_TPB : SCALE_MAX_BLOCKS;
    if (W == 4) hipLaunchKernelGGL(bsx_gae_scale_kernel<4>, dim3(unsigned(blocks)), dim3(SCALE_TPB), 0, s, io->adv, io->mask, groups, stats);
    else hipLaunchKernelGGL(bsx_gae_scale_kernel<2>, dim3(unsigned(blocks)), dim3(SCALE_TPB), 0, s, io->adv, io->mask, groups, stats);
    return int(hipGetLastError());
}

}  // extern "C"
