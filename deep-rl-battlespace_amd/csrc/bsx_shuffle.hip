// bsx_shuffle.hip -- a keyed permutation of a rollout's rows and the minibatch gather built on it (include/battlespace_hip.h:
// bsx_shuffle_rows, bsx_minibatch_gather), gfx950.
//
// PPO draws a fresh permutation of the T x E rows per epoch and cuts it into minibatches.  The permutation here is evaluated per position,
// with no sort, no workspace and no atomics: a balanced Feistel network over the smallest even-width power-of-two domain that holds
// [0, N), walked until the value falls below N (cycle walking: the network is a bijection of the domain, so the walk from a start below
// N returns below N, and the walked map is a bijection of [0, N)).  The eight round keys are the words of two Philox4x32-10 blocks
// (bsx_actor::philox4x32_10, the one the step, the actor and the replay sampler use) keyed by (seed, seq + *seq_base), so a captured
// call draws afresh at every replay once the caller advances the base word.  tests/shuffle_util.py restates it in numpy.
// The gather is shaped like bsx_replay_sample_kernel: a workgroup owns ROWS destination rows, its first lanes evaluate the permutation
// into LDS, then all 256 threads walk the rows' words flat, field by field.  Bits are copied, never converted: no -ffp-contract concern.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_core.h"
#include "bsx_args.h"

namespace {

constexpr int TPB = 256;
constexpr int ROWS = 32;                        // destination rows per gathering workgroup (bsx_replay.hip's DRAWS, for its reason)
constexpr int ROUNDS = 8;
constexpr uint32_t SHUFFLE_SALT = 0x5AFF1E00u;  // keeps the permutation's Philox stream apart from the actor's, the opponent's and the sampler's

struct ShuffleArgs {
    uint32_t N; int b;                          // rows, half the domain's bits
    int64_t first, R; uint64_t seed, seq; const uint64_t* seq_base; int64_t* idx;
};

struct GatherArgs {
    BsxMinibatchIo io; ShuffleArgs s; int A, D;
};

// The eight round keys into LDS, once per workgroup (they are uniform over the launch): thread j = 0, 1 computes the block of counter
// (j, 0, seq_lo, seq_hi).  The caller synchronises before reading.
__device__ inline void round_keys(uint32_t* s_key, const ShuffleArgs& p, int tid) {
    if (tid < ROUNDS / 4) {
        const uint64_t seq = p.seq + (p.seq_base ? *p.seq_base : 0ull);
        const uint4 w = bsx_actor::philox4x32_10(make_uint4(uint32_t(tid), 0u, uint32_t(seq), uint32_t(seq >> 32)),
                                                 make_uint2(uint32_t(p.seed), uint32_t(p.seed >> 32) ^ SHUFFLE_SALT));
        s_key[4 * tid] = w.x; s_key[4 * tid + 1] = w.y; s_key[4 * tid + 2] = w.z; s_key[4 * tid + 3] = w.w;
    }
}

// The source row of position `pos` < N.  At b = 16 the domain is 2^32: x is compared unsigned.
__device__ inline int64_t perm_at(uint32_t pos, uint32_t N, int b, const uint32_t* s_key) {
    const uint32_t mask = (1u << b) - 1u;
    uint32_t k[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) k[r] = s_key[r];
    uint32_t x = pos;
    do {
        uint32_t L = x >> b, R = x & mask;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            uint32_t h = (R ^ k[r]) * 0x9E3779B1u;
            h ^= h >> 15;
            h *= 0x85EBCA77u;
            h ^= h >> 13;
            const uint32_t next = (L ^ (h >> (32 - b))) & mask;
            L = R;
            R = next;
        }
        x = (L << b) | R;
    } while (x >= N);
    return int64_t(x);
}

__global__ __launch_bounds__(TPB) void bsx_shuffle_rows_kernel(const ShuffleArgs p) {
    __shared__ uint32_t s_key[ROUNDS];
    const int tid = threadIdx.x;
    round_keys(s_key, p, tid);
    __syncthreads();
    const int64_t r = int64_t(blockIdx.x) * TPB + tid;
    if (r < p.R) p.idx[r] = perm_at(uint32_t(p.first + r), p.N, p.b, s_key);
}

// n rows of one field: destination row r0 + i <- source row s_row[i]; both sides are dense rows of W elements (n <= ROWS).
template <typename T>
__device__ inline void gather_field(T* __restrict__ dst, const T* __restrict__ src, int W, int64_t r0, int n, const int64_t* s_row, int tid) {
    for (int j = tid; j < n * W; j += TPB) {
        const int i = j / W, rem = j - i * W;
        dst[(r0 + i) * W + rem] = src[s_row[i] * W + rem];
    }
}

// A row's pieces lie in seven arrays, each a short read at a random address: the memory side sees one request per (row, field) --
// measured, 7.0 per row at 1v1 -- whatever the order of the loads.  A form that had the mask bytes and four words per thread in flight
// before its first store took the same 82 us per 524 288 rows as this one, so the plain loops stay.
__global__ __launch_bounds__(TPB) void bsx_minibatch_gather_kernel(const GatherArgs p) {
    __shared__ uint32_t s_key[ROUNDS];
    __shared__ int64_t s_row[ROWS];
    const int tid = threadIdx.x;
    round_keys(s_key, p.s, tid);
    __syncthreads();
    const int64_t r0 = int64_t(blockIdx.x) * ROWS;
    const int n = int(p.s.R - r0 < ROWS ? p.s.R - r0 : ROWS);
    if (tid < n) {
        const int64_t row = perm_at(uint32_t(p.s.first + r0 + tid), p.s.N, p.s.b, s_key);
        s_row[tid] = row;
        p.s.idx[r0 + tid] = row;
    }
    __syncthreads();
    const BsxMinibatchIo& g = p.io;
    const auto words = [](const float* x) { return reinterpret_cast<const uint32_t*>(x); };
    const auto words_out = [](float* x) { return reinterpret_cast<uint32_t*>(x); };
    gather_field(words_out(g.dst_obs), words(g.obs), p.A * p.D, r0, n, s_row, tid);
    gather_field(words_out(g.dst_rec), words(g.rec), p.A * 4, r0, n, s_row, tid);
    gather_field(words_out(g.dst_logp), words(g.logp), p.A, r0, n, s_row, tid);
    gather_field(words_out(g.dst_adv), words(g.adv), p.A, r0, n, s_row, tid);
    gather_field(words_out(g.dst_ret), words(g.ret), p.A, r0, n, s_row, tid);
    if (g.value) gather_field(words_out(g.dst_value), words(g.value), p.A, r0, n, s_row, tid);
    gather_field(g.dst_mask, g.mask, p.A, r0, n, s_row, tid);          // bytewise: A bytes per row need not be a multiple of 4
}

constexpr int64_t MAX_ROWS = (int64_t(1) << 31) - 1;

// BSX_E_ARG unless 1 <= N < 2^31 and [first, first + R) is a non-empty range inside [0, N)
int check_range(int64_t N, int64_t first, int64_t R) {
    if (N < 1 || N > MAX_ROWS || R < 1 || first < 0 || first > N || R > N - first) return BSX_E_ARG;
    return 0;
}

// b of the domain 2^(2b): bits = max(2, bit_length(N - 1)), b = (bits + 1) / 2
int half_bits(int64_t N) {
    int bits = 0;
    for (uint64_t v = uint64_t(N - 1); v; v >>= 1) ++bits;
    if (bits < 2) bits = 2;
    return (bits + 1) / 2;
}

}  // namespace

extern "C" {

int bsx_shuffle_rows(int64_t N, int64_t first, int64_t R, uint64_t seed, uint64_t seq, const uint64_t* seq_base, int64_t* idx,
                     void* stream) {
    if (!idx) return BSX_E_ARG;
    if (const int rc = check_range(N, first, R)) return rc;
    if (!aligned(idx, 8) || !aligned(seq_base, 8)) return BSX_E_ALIGN;
    ShuffleArgs a{uint32_t(N), half_bits(N), first, R, seed, seq, seq_base, idx};
    hipLaunchKernelGGL(bsx_shuffle_rows_kernel, dim3(unsigned((R + TPB - 1) / TPB)), dim3(TPB), 0, static_cast<hipStream_t>(stream), a);
    return int(hipGetLastError());
}

int bsx_minibatch_gather(const BsxMinibatchIo* io, int64_t N, int64_t first, int64_t R, int A, int D, uint64_t seed, uint64_t seq,
                         const uint64_t* seq_base, void* stream) {
    if (!io) return BSX_E_ARG;
    if (!io->obs || !io->rec || !io->logp || !io->adv || !io->ret || !io->mask || !io->dst_obs || !io->dst_rec || !io->dst_logp ||
        !io->dst_adv || !io->dst_ret || !io->dst_mask || !io->idx || !io->value != !io->dst_value) return BSX_E_ARG;
    if (const int rc = check_range(N, first, R)) return rc;
    if (A < 2 || A > 2 * BSX_MAX_N || A % 2 || D < 1 || D > 3 * BSX_MAX_N + 2) return BSX_E_ARG;
    if (!aligned(io->obs, 4) || !aligned(io->rec, 4) || !aligned(io->logp, 4) || !aligned(io->adv, 4) || !aligned(io->ret, 4) ||
        !aligned(io->value, 4) || !aligned(io->dst_obs, 4) || !aligned(io->dst_rec, 4) || !aligned(io->dst_logp, 4) ||
        !aligned(io->dst_adv, 4) || !aligned(io->dst_ret, 4) || !aligned(io->dst_value, 4) || !aligned(io->idx, 8) ||
        !aligned(seq_base, 8)) return BSX_E_ALIGN;
    GatherArgs a{*io, ShuffleArgs{uint32_t(N), half_bits(N), first, R, seed, seq, seq_base, io->idx}, A, D};
    hipLaunchKernelGGL(bsx_minibatch_gather_kernel, dim3(unsigned((R + ROWS - 1) / ROWS)), dim3(TPB), 0, static_cast<hipStream_t>(stream), a);
    return int(hipGetLastError());
}

}  // extern "C"
