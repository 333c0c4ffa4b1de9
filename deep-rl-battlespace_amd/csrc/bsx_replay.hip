// bsx_replay.hip -- the replay ring on device (include/battlespace_hip.h: bsx_replay_*), gfx950.
//
// Replaces, on the learner's collect path, the host-driven ring of replay.py (ReplayBuffer._put / store_rollout / sample;
// reference maddpg/buffer.py:25-67).  The torch path learns the number of kept rows on the host (nonzero -> int) because the ring's
// counter is a Python int; here the counter is a device word and the whole store is three launches with no host round trip:
//   1. count   -- one workgroup per 256 source rows counts its kept rows (ballot + popcount per wave);
//   2. scan    -- ONE workgroup scans the tile counts into tile bases, reads the counter, moves it by R and publishes R;
//   3. scatter -- each tile ranks its kept rows (ballot + mbcnt + the wave prefix in LDS), compacts (source, ring row) pairs in LDS
//                 and then walks the tile's elements flat, so that consecutive lanes load and store consecutive words.
// Ranks are unique and, with R > M, only the newest M survive: every ring row is written at most once per append, no write races.
// No inter-workgroup flags or spins: three graph nodes cost far less than the data they move.
// The sampler draws with Philox4x32-10 (bsx_actor::philox4x32_10, the one the step and the actor use) and gathers in the same
// launch.  Bits are copied, never converted: no -ffp-contract concern.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_core.h"
#include "bsx_args.h"
#include "bsx_replay_ring.h"

namespace {

using namespace bsx_ring;        // TPB (threads per workgroup = source rows per tile of an append), gather_rows, the ring checks
// draws per sampling workgroup: its 256 lanes walk 32 rows' words (a 4v4 row is 56 words per observation), a few loads each instead of
// a long dependent chain -- with 256 draws per workgroup the gather was latency-bound (4v4, B = 512: two workgroups, 78 us)
constexpr int DRAWS = 32;
constexpr int SCAN_TPB = 1024;    // the one scanning workgroup
constexpr uint32_t SAMPLE_SALT = 0x5EED5A3Cu;   // keeps the sampler's Philox stream apart from the step's and the actor's under one seed

struct AppendArgs {
    BsxReplayRing ring; BsxReplaySource src; int64_t rows;
    int64_t* head;                // workspace: [0] = counter before the append, [1] = R
    int32_t* counts;              // workspace: kept rows per tile
    int32_t* bases;               // workspace: rank of each tile's first kept row
    int64_t* stored; int tiles;
};

struct SampleArgs {
    BsxReplayRing ring; int64_t B; uint64_t seed, seq; const uint64_t* seq_base;
    int64_t* idx; float* obs; float* obs_next; float* act; float* rew; uint8_t* done;
};

__device__ inline bool kept_row(const AppendArgs& p, int64_t r) {
    return r < p.rows && (!p.src.skip || p.src.skip[r * p.src.skip_row] == 0);
}

// The kept rows of the tile before this wave, and in the whole tile (s_w: per-wave counts of the 256 / 64 waves).
__device__ inline void tile_prefix(const int* s_w, int wave, int& before, int& total) {
    before = 0; total = 0;
#pragma unroll
    for (int j = 0; j < TPB / 64; ++j) { before += j < wave ? s_w[j] : 0; total += s_w[j]; }
}

__global__ __launch_bounds__(TPB) void bsx_replay_count_kernel(const AppendArgs p) {
    __shared__ int s_w[TPB / 64];
    const int tid = threadIdx.x;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(kept_row(p, int64_t(blockIdx.x) * TPB + tid));
    if ((tid & 63) == 0) s_w[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int before, total;
        tile_prefix(s_w, TPB / 64, before, total);
        p.counts[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(SCAN_TPB) void bsx_replay_scan_kernel(const AppendArgs p) {
    __shared__ int s_w[SCAN_TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;                                            // rows < 2^31: every rank fits an int
    for (int first = 0; first < p.tiles; first += SCAN_TPB) {
        const int i = first + tid;
        const int v = i < p.tiles ? p.counts[i] : 0;
        int x = v;                                            // inclusive scan across the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < SCAN_TPB / 64; ++j) { before += j < wave ? s_w[j] : 0; total += s_w[j]; }
        if (i < p.tiles) p.bases[i] = carry + before + x - v;
        carry += total;
        __syncthreads();                                      // s_w is written again by the next chunk
    }
    if (tid == 0) {
        const int64_t old = *p.ring.counter;
        p.head[0] = old;
        p.head[1] = carry;
        *p.ring.counter = old + carry;
        if (p.stored) *p.stored = carry;
    }
}

// n rows of one field: ring row s_dst[i] <- source row s_src[i], nA columns of `width` elements each.  The loop runs over the n x nA x width
// elements flat: consecutive lanes store consecutive words of the ring (and load consecutive words of a source row's column).
template <typename T>
__device__ inline void scatter_field(T* __restrict__ dst, const T* __restrict__ src, int64_t row_stride, int64_t col_stride, int nA, int width,
                                     int n, const int64_t* s_src, const int64_t* s_dst, int tid) {
    const int W = nA * width;
    for (int j = tid; j < n * W; j += TPB) {
        const int i = j / W, rem = j - i * W, c = rem / width, x = rem - c * width;
        const T v = src[s_src[i] * row_stride + int64_t(c) * col_stride + x];
        if constexpr (sizeof(T) == 1) dst[s_dst[i] * W + rem] = T(v != 0);
        else dst[s_dst[i] * W + rem] = v;
    }
}

__global__ __launch_bounds__(TPB) void bsx_replay_scatter_kernel(const AppendArgs p) {
    __shared__ int64_t s_src[TPB], s_dst[TPB];
    __shared__ int s_w[TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = int64_t(blockIdx.x) * TPB + tid;
    const bool keep = kept_row(p, r);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
    const int in_wave = int(__builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u)));
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int before, total;
    tile_prefix(s_w, wave, before, total);
    const int64_t old = p.head[0], R = p.head[1], M = p.ring.M, rank0 = p.bases[blockIdx.x];
    // with R > M only ranks >= R - M are written (the newest M rows): within the tile those are a suffix of its kept rows
    const int64_t lost = R > M ? R - M : 0;
    const int lo = int(lost <= rank0 ? 0 : (lost - rank0 < total ? lost - rank0 : total));
    if (keep) {
        const int i = before + in_wave;
        if (i >= lo) {
            s_src[i - lo] = r;
            const int64_t d = (old + rank0 + i) % M;
            s_dst[i - lo] = d < 0 ? d + M : d;           // a counter the caller set negative still lands inside the ring
        }
    }
    __syncthreads();
    const int n = total - lo;
    if (n == 0) return;
    const BsxReplayRing& g = p.ring;
    const BsxReplaySource& s = p.src;
    scatter_field(reinterpret_cast<uint32_t*>(g.obs), reinterpret_cast<const uint32_t*>(s.obs), s.obs_row, s.obs_col, g.nA, g.D, n, s_src, s_dst, tid);
    scatter_field(reinterpret_cast<uint32_t*>(g.obs_next), reinterpret_cast<const uint32_t*>(s.obs_next), s.obs_next_row, s.obs_next_col, g.nA, g.D,
                  n, s_src, s_dst, tid);
    scatter_field(reinterpret_cast<uint32_t*>(g.act), reinterpret_cast<const uint32_t*>(s.act), s.act_row, s.act_col, g.nA, g.n_act, n, s_src, s_dst, tid);
    scatter_field(reinterpret_cast<uint32_t*>(g.rew), reinterpret_cast<const uint32_t*>(s.rew), s.rew_row, s.rew_col, g.nA, 1, n, s_src, s_dst, tid);
    scatter_field(g.done, s.done, s.done_row, s.done_col, g.nA, 1, n, s_src, s_dst, tid);
}

__global__ __launch_bounds__(TPB) void bsx_replay_sample_kernel(const SampleArgs p) {
    __shared__ int64_t s_row[DRAWS];
    const int tid = threadIdx.x;
    const int64_t b0 = int64_t(blockIdx.x) * DRAWS, b = b0 + tid;
    const int n = int(p.B - b0 < DRAWS ? p.B - b0 : DRAWS);
    if (tid < n) {
        const int64_t cnt = *p.ring.counter;
        const uint32_t max_mem = uint32_t(cnt <= 0 ? 0 : (cnt < p.ring.M ? cnt : p.ring.M));    // M < 2^31; a negative counter = empty
        const uint64_t seq = p.seq + (p.seq_base ? *p.seq_base : 0ull);
        const uint4 w = bsx_actor::philox4x32_10(make_uint4(uint32_t(b), uint32_t(uint64_t(b) >> 32), uint32_t(seq), uint32_t(seq >> 32)),
                                                 make_uint2(uint32_t(p.seed), uint32_t(p.seed >> 32) ^ SAMPLE_SALT));
        const int64_t row = int64_t(__umulhi(w.x, max_mem));                    // multiply-shift onto [0, max_mem); 0 for an empty ring
        s_row[tid] = row;
        p.idx[b] = row;
    }
    __syncthreads();
    gather_rows(p.ring, p.obs, p.obs_next, p.act, p.rew, p.done, b0, n, s_row, tid);
}

int64_t tiles_of(int64_t rows) { return (rows + TPB - 1) / TPB; }

}  // namespace

extern "C" {

int bsx_replay_workspace_bytes(int64_t rows, size_t* bytes) {
    if (rows < 1 || rows > MAX_ROWS || !bytes) return BSX_E_ARG;
    *bytes = size_t(16 + 8 * tiles_of(rows));
    return 0;
}

int bsx_replay_append(const BsxReplayRing* ring, const BsxReplaySource* src, int64_t rows, void* workspace, int64_t* stored,
                      void* stream) {
    if (const int rc = check_ring(ring)) return rc;
    if (!src || !workspace || rows < 1 || rows > MAX_ROWS) return BSX_E_ARG;
    if (!src->obs || !src->obs_next || !src->act || !src->rew || !src->done) return BSX_E_ARG;
    if (src->obs_row < 0 || src->obs_col < 0 || src->obs_next_row < 0 || src->obs_next_col < 0 || src->act_row < 0 || src->act_col < 0 ||
        src->rew_row < 0 || src->rew_col < 0 || src->done_row < 0 || src->done_col < 0 || src->skip_row < 0) return BSX_E_ARG;
    if (ring_misaligned(ring) || !aligned(src->obs, 4) || !aligned(src->obs_next, 4) || !aligned(src->act, 4) || !aligned(src->rew, 4) ||
        !aligned(workspace, 8) || !aligned(stored, 8)) return BSX_E_ALIGN;
    const int64_t tiles = tiles_of(rows);
    int64_t* head = static_cast<int64_t*>(workspace);
    int32_t* counts = reinterpret_cast<int32_t*>(head + 2);
    AppendArgs a{*ring, *src, rows, head, counts, counts + tiles, stored, int(tiles)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bsx_replay_count_kernel, dim3(unsigned(tiles)), dim3(TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(bsx_replay_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(bsx_replay_scatter_kernel, dim3(unsigned(tiles)), dim3(TPB), 0, s, a);
    return int(hipGetLastError());
}

int bsx_replay_sample(const BsxReplayRing* ring, int64_t B, uint64_t seed, uint64_t seq, const uint64_t* seq_base, int64_t* idx,
                      float* obs, float* obs_next, float* act, float* rew, uint8_t* done, void* stream) {
    if (const int rc = check_ring(ring)) return rc;
    if (B < 1 || B > MAX_ROWS || !idx || !obs || !obs_next || !act || !rew || !done) return BSX_E_ARG;
    if (ring_misaligned(ring) || !aligned(seq_base, 8) || !aligned(idx, 8) || !aligned(obs, 4) || !aligned(obs_next, 4) || !aligned(act, 4) ||
        !aligned(rew, 4)) return BSX_E_ALIGN;
    SampleArgs a{*ring, B, seed, seq, seq_base, idx, obs, obs_next, act, rew, done};
    hipLaunchKernelGGL(bsx_replay_sample_kernel, dim3(unsigned((B + DRAWS - 1) / DRAWS)), dim3(TPB), 0, static_cast<hipStream_t>(stream), a);
    return int(hipGetLastError());
}

}  // extern "C"
