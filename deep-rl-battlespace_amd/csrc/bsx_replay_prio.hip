// bsx_replay_prio.hip -- proportional prioritised replay on the device ring (include/battlespace_hip.h: bsx_replay_prio_*), gfx950.
//
// A sum tree of fan-out 64 over uint32 fixed-point priorities (scale 2^16), every inner node the int64 sum of its children: integer
// sums are exact and order-free, so the tree has ONE right value and the draw is searchsorted(cumsum(leaves), u) bit for bit.
// One wavefront reads one node: its 64 children are one coalesced load (one per lane), the prefix is a 6-step wave scan, the child
// taken is a ballot and a find-first.  A draw is a chain of `levels` dependent loads (four at 1 M rows): each draw has a wave of its
// own and many waves overlap -- the lesson bsx_replay.hip records at DRAWS.
// Nodes are never added to: a touched parent is recomputed from its 64 children (64-bit add-atomics execute at the memory side,
// uncached), one launch per level because a level reads the one below it; the levels of at most 64 nodes -- the top of the tree --
// are recomputed whole by ONE workgroup between __syncthreads().  The only atomics are an integer max on the leaves a batch names
// and on the max_priority word.  No inter-workgroup flags or spins.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_core.h"
#include "bsx_args.h"
#include "bsx_replay_ring.h"

namespace {

using namespace bsx_ring;

constexpr int FAN = BSX_PRIO_FANOUT;            // 64: the wavefront
constexpr int MAX_LEVELS = 6;                   // M < 2^31: 2^25, 2^19, 2^13, 2^7, 2, 1 nodes at the most
constexpr int WAVES = TPB / 64;                 // draws (and nodes) per 256-thread workgroup: one per wave
constexpr int TAIL_TPB = 1024, W_TPB = 1024;
constexpr uint32_t P_MAX = 0x80000000u;         // the largest stored priority, 2^31

// level k of the node buffer: cnt[k] int64 nodes from nodes[off[k]]; level 0 sums the leaves, level n - 1 is the root
struct Levels { int n; int64_t off[MAX_LEVELS], cnt[MAX_LEVELS]; };

Levels levels_of(int64_t M) {
    Levels lv{};
    int64_t c = (M + FAN - 1) / FAN, o = 0;
    for (;;) {
        lv.off[lv.n] = o; lv.cnt[lv.n] = c; ++lv.n;
        if (c == 1) return lv;
        o += c; c = (c + FAN - 1) / FAN;
    }
}

// the first level of at most 64 nodes: it and every level above it belong to the tail workgroup
int tail_level(const Levels& lv) {
    int k = 0;
    while (lv.cnt[k] > FAN) ++k;
    return k;
}

__device__ inline int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ inline int64_t wave_scan(int64_t v, int lane) {            // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(v, d);
        if (lane >= d) v += y;
    }
    return v;
}

// lane's child of node `node`: a leaf (leaves are padded to a multiple of 64 with zeros) or an int64 node of the level below (`cnt` of them)
__device__ inline int64_t leaf_child(const uint32_t* leaves, int64_t node, int lane) { return int64_t(leaves[node * FAN + lane]); }
__device__ inline int64_t node_child(const int64_t* below, int64_t cnt, int64_t node, int lane) {
    const int64_t i = node * FAN + lane;
    return i < cnt ? below[i] : 0;
}

// ---------------------------------------------------------------------------------------------------------------- repair
enum { WHOLE = 0, BY_IDX = 1, BY_RANGE = 2 };

struct RepairArgs {
    const uint32_t* leaves;       // level 0: the children are leaves
    const int64_t* below;         // level k > 0: the level below, below_cnt nodes
    int64_t below_cnt;
    int64_t* level;               // the level repaired, level_cnt nodes
    int64_t level_cnt;
    int64_t waves;                // the call's upper bound of nodes to repair: surplus waves exit
    int mode, shift;              // a leaf row r lies under node r >> shift of this level
    const int64_t* idx;           // BY_IDX: the rows touched, `waves` of them
    const int64_t* counter; const int64_t* stored; int64_t M;     // BY_RANGE: the rows (counter - s + j) mod M, j < s = min(stored, M)
};

// The node of this level that wave w repairs, -1 for none.
__device__ inline int64_t repair_node(const RepairArgs& p, int64_t w) {
    if (p.mode == WHOLE) return w < p.level_cnt ? w : -1;
    if (p.mode == BY_IDX) {
        const int64_t r = p.idx[w];
        return r >= 0 && r < p.M ? r >> p.shift : -1;
    }
    const int64_t R = *p.stored, M = p.M, s = R < M ? R : M;
    if (s <= 0) return -1;
    if (s == M) return w < p.level_cnt ? w : -1;
    int64_t a = (*p.counter - s) % M;
    if (a < 0) a += M;
    const int64_t e = a + s;                                          // [a, min(e, M)) and, past the wrap, [0, e - M)
    const int64_t first = a >> p.shift, n1 = (((e < M ? e : M) - 1) >> p.shift) - first + 1;
    const int64_t n2 = e > M ? ((e - M - 1) >> p.shift) + 1 : 0;
    return w < n1 ? first + w : (w < n1 + n2 ? w - n1 : -1);
}

__global__ __launch_bounds__(TPB) void bsx_prio_repair_kernel(const RepairArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t w = int64_t(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    if (w >= p.waves) return;
    const int64_t node = repair_node(p, w);
    if (node < 0) return;
    const int64_t s = wave_sum(p.leaves ? leaf_child(p.leaves, node, lane) : node_child(p.below, p.below_cnt, node, lane));
    if (lane == 0) p.level[node] = s;          // two waves on one node (a row drawn twice, the wrap's shared node) write the same sum
}

struct TailArgs { BsxPrioTree t; Levels lv; int first; };

// Levels first .. n - 1 (at most 64 nodes each) recomputed whole by one workgroup, bottom-up.
__global__ __launch_bounds__(TAIL_TPB) void bsx_prio_tail_kernel(const TailArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MAX_LEVELS; ++k) {
        if (k < p.first || k >= p.lv.n) continue;
        for (int64_t node = wave; node < p.lv.cnt[k]; node += TAIL_TPB / 64) {
            const int64_t s = wave_sum(k == 0 ? leaf_child(p.t.leaves, node, lane)
                                              : node_child(p.t.nodes + p.lv.off[k > 0 ? k - 1 : 0], p.lv.cnt[k > 0 ? k - 1 : 0], node, lane));
            if (lane == 0) p.t.nodes[p.lv.off[k] + node] = s;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- update
struct UpdateArgs { BsxPrioTree t; const int64_t* idx; const float* q; const float* y; int64_t B; int nA; };

__global__ __launch_bounds__(TPB) void bsx_prio_clear_kernel(const UpdateArgs p) {
    const int64_t b = int64_t(blockIdx.x) * TPB + threadIdx.x;
    if (b >= p.B) return;
    const int64_t r = p.idx[b];
    if (r >= 0 && r < p.t.M) p.t.leaves[r] = 0u;
}

// p = clamp(rint(powf(fminf(delta, delta_max) + eps, alpha) * 65536), 1, 2^31), delta the largest |q - y| of the row's agents
__device__ inline uint32_t priority_of(const float* q, const float* y, int nA, float alpha, float eps, float delta_max) {
    float delta = 0.0f;
    for (int i = 0; i < nA; ++i) delta = fmaxf(delta, fminf(fabsf(q[i] - y[i]), delta_max));     // fminf: a NaN error counts as delta_max
    const float x = rintf(powf(delta + eps, alpha) * 65536.0f);
    return !(x >= 1.0f) ? 1u : (x >= 2147483648.0f ? P_MAX : uint32_t(x));
}

__global__ __launch_bounds__(TPB) void bsx_prio_max_kernel(const UpdateArgs p) {
    __shared__ uint32_t s_w[WAVES];
    const int tid = threadIdx.x;
    const int64_t b = int64_t(blockIdx.x) * TPB + tid;
    uint32_t pr = 0u;
    if (b < p.B) {
        const int64_t r = p.idx[b];
        if (r >= 0 && r < p.t.M) {
            pr = priority_of(p.q + b * p.nA, p.y + b * p.nA, p.nA, p.t.hyper[0], p.t.hyper[2], p.t.hyper[3]);
            atomicMax(p.t.leaves + r, pr);
        }
    }
    uint32_t m = pr;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(m, d); m = o > m ? o : m; }
    if ((tid & 63) == 0) s_w[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < WAVES; ++j) m = s_w[j] > m ? s_w[j] : m;
        if (m > *p.t.max_priority) atomicMax(p.t.max_priority, m);    // the word only grows: the plain read spares the atomic in the steady state
    }
}

// ---------------------------------------------------------------------------------------------------------------- append
struct AppendArgs { BsxPrioTree t; const int64_t* counter; const int64_t* stored; int64_t rows; };

__global__ __launch_bounds__(TPB) void bsx_prio_append_kernel(const AppendArgs p) {
    const int64_t j = int64_t(blockIdx.x) * TPB + threadIdx.x, M = p.t.M, R = *p.stored, s = R < M ? R : M;
    if (j >= s) return;
    int64_t r = (*p.counter - s + j) % M;
    if (r < 0) r += M;
    p.t.leaves[r] = *p.t.max_priority;
}

// ---------------------------------------------------------------------------------------------------------------- draw
struct DrawArgs {
    BsxReplayRing ring; BsxPrioTree t; Levels lv; int64_t root; int64_t B; uint64_t seed, seq; const uint64_t* seq_base;
    int64_t* idx; uint32_t* drawn; float* obs; float* obs_next; float* act; float* rew; uint8_t* done;
};

__global__ __launch_bounds__(TPB) void bsx_prio_draw_kernel(const DrawArgs p) {
    __shared__ int64_t s_row[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = int64_t(blockIdx.x) * WAVES, b = b0 + wave;
    const int n = int(p.B - b0 < WAVES ? p.B - b0 : WAVES);
    if (wave < n) {
        const uint64_t seq = p.seq + (p.seq_base ? *p.seq_base : 0ull);
        const uint4 w = bsx_actor::philox4x32_10(make_uint4(uint32_t(b), uint32_t(uint64_t(b) >> 32), uint32_t(seq), uint32_t(seq >> 32)),
                                                 make_uint2(uint32_t(p.seed), uint32_t(p.seed >> 32) ^ BSX_PRIO_SALT));
        const int64_t total = p.t.nodes[p.root];
        int64_t u = int64_t(__umul64hi((uint64_t(w.y) << 32) | w.x, uint64_t(total)));       // total < 2^62: u < total fits
        int64_t node = 0, v = 0;
        int j = 0;
#pragma unroll
        for (int k = MAX_LEVELS - 1; k >= 0; --k) {
            if (k >= p.lv.n) continue;
            v = k == 0 ? leaf_child(p.t.leaves, node, lane) : node_child(p.t.nodes + p.lv.off[k > 0 ? k - 1 : 0], p.lv.cnt[k > 0 ? k - 1 : 0], node, lane);
            const int64_t incl = wave_scan(v, lane);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(incl > u);
            // the first child whose inclusive prefix exceeds u; it has v > 0, so it exists.  No such child (an empty ring, or a tree that
            // no longer sums its leaves): child 0, which exists under every node -- never an address outside the tree
            j = m ? __builtin_ctzll(m) : 0;
            const int64_t before = __shfl(incl - v, j);
            u -= m ? before : 0;
            node = node * FAN + j;
        }
        const int64_t pb = __shfl(v, j);
        if (lane == 0) {
            const int64_t row = total > 0 ? (node < p.ring.M ? node : p.ring.M - 1) : 0;
            s_row[wave] = row;
            p.idx[b] = row;
            p.drawn[b] = total > 0 ? uint32_t(pb) : 0u;
        }
    }
    __syncthreads();
    gather_rows(p.ring, p.obs, p.obs_next, p.act, p.rew, p.done, b0, n, s_row, tid);
}

// ---------------------------------------------------------------------------------------------------------------- weights
struct WeightArgs { BsxPrioTree t; const int64_t* idx; uint32_t* drawn; int64_t B; int nA; float* w; };

__global__ __launch_bounds__(TPB) void bsx_prio_leaves_kernel(const WeightArgs p) {
    const int64_t b = int64_t(blockIdx.x) * TPB + threadIdx.x;
    if (b >= p.B) return;
    const int64_t r = p.idx[b];
    p.drawn[b] = r >= 0 && r < p.t.M ? p.t.leaves[r] : 0u;
}

// w = (p_min / p_b) ^ beta, p_min the smallest non-zero drawn leaf: every workgroup finds it over the whole batch (B words, L2 hits
// after the first) instead of a second reduction launch, then writes its 1024 rows.  The power is taken in binary64, where both
// integers and their quotient's 53 bits are exact, and rounded to float32 once: the device's powf is within an ulp but not correctly
// rounded, and a batch that names a handful of rows has a handful of weights -- their mean error then sits at twice a correctly
// rounded evaluation's by luck (measured 2.13 x at M = 64, B = 512).  One pow per batch row is nothing next to the draw.
__global__ __launch_bounds__(W_TPB) void bsx_prio_weights_kernel(const WeightArgs p) {
    __shared__ uint32_t s_w[W_TPB / 64];
    const int tid = threadIdx.x;
    uint32_t m = 0xFFFFFFFFu;
    for (int64_t i = tid; i < p.B; i += W_TPB) {
        const uint32_t v = p.drawn[i];
        m = v != 0u && v < m ? v : m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(m, d); m = o < m ? o : m; }
    if ((tid & 63) == 0) s_w[tid >> 6] = m;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < W_TPB / 64; ++j) m = s_w[j] < m ? s_w[j] : m;
    const int64_t b = int64_t(blockIdx.x) * W_TPB + tid;
    if (b >= p.B) return;
    const uint32_t pb = p.drawn[b];
    const float w = pb != 0u ? float(pow(double(m) / double(pb), double(p.t.hyper[1]))) : 0.0f;      // a row never stored (an empty ring's draw): +0
    for (int i = 0; i < p.nA; ++i) p.w[b * p.nA + i] = w;
}

// ---------------------------------------------------------------------------------------------------------------- host
int check_tree(const BsxPrioTree* t) {
    if (!t || !t->leaves || !t->nodes || !t->max_priority || !t->hyper || t->M < 1 || t->M > MAX_ROWS) return BSX_E_ARG;
    return 0;
}

bool tree_misaligned(const BsxPrioTree* t) {
    return !aligned(t->leaves, 4) || !aligned(t->nodes, 8) || !aligned(t->max_priority, 4) || !aligned(t->hyper, 16);
}

unsigned blocks(int64_t items, int per) { return unsigned((items + per - 1) / per); }

// The levels below the tail, one launch each -- `touched(args)` sets the level's mode and its bound of waves (WHOLE is the default) --, then
// the tail.  -> the first HIP error, 0 for none
template <typename F>
int repair(const BsxPrioTree& t, const Levels& lv, hipStream_t s, F touched) {
    const int first = tail_level(lv);
    for (int k = 0; k < first; ++k) {
        RepairArgs a{k == 0 ? t.leaves : nullptr, k ? t.nodes + lv.off[k - 1] : nullptr, k ? lv.cnt[k - 1] : 0, t.nodes + lv.off[k], lv.cnt[k],
                     0, WHOLE, 6 * (k + 1), nullptr, nullptr, nullptr, t.M};
        touched(a);
        hipLaunchKernelGGL(bsx_prio_repair_kernel, dim3(blocks(a.waves, WAVES)), dim3(TPB), 0, s, a);
        if (const hipError_t e = hipGetLastError()) return int(e);
    }
    hipLaunchKernelGGL(bsx_prio_tail_kernel, dim3(1), dim3(TAIL_TPB), 0, s, TailArgs{t, lv, first});
    return int(hipGetLastError());
}

int weights(const WeightArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(bsx_prio_weights_kernel, dim3(blocks(a.B, W_TPB)), dim3(W_TPB), 0, s, a);
    return int(hipGetLastError());
}

}  // namespace

extern "C" {

int bsx_replay_prio_bytes(int64_t M, size_t* bytes) {
    if (M < 1 || M > MAX_ROWS || !bytes) return BSX_E_ARG;
    const Levels lv = levels_of(M);
    *bytes = size_t(8 * (lv.off[lv.n - 1] + 1));
    return 0;
}

int bsx_replay_prio_rebuild(const BsxPrioTree* tree, void* stream) {
    if (const int rc = check_tree(tree)) return rc;
    if (tree_misaligned(tree)) return BSX_E_ALIGN;
    return repair(*tree, levels_of(tree->M), static_cast<hipStream_t>(stream), [](RepairArgs& a) { a.waves = a.level_cnt; });
}

int bsx_replay_prio_update(const BsxPrioTree* tree, const int64_t* idx, const float* q, const float* y, int64_t B, int nA, void* stream) {
    if (const int rc = check_tree(tree)) return rc;
    if (!idx || !q || !y || B < 1 || B > MAX_ROWS || nA < 1 || nA > BSX_MAX_N) return BSX_E_ARG;
    if (tree_misaligned(tree) || !aligned(idx, 8) || !aligned(q, 4) || !aligned(y, 4)) return BSX_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const UpdateArgs a{*tree, idx, q, y, B, nA};
    hipLaunchKernelGGL(bsx_prio_clear_kernel, dim3(blocks(B, TPB)), dim3(TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(bsx_prio_max_kernel, dim3(blocks(B, TPB)), dim3(TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    // a level with no more nodes than the batch has rows is recomputed whole: one wave per node instead of one per row
    return repair(*tree, levels_of(tree->M), s, [&](RepairArgs& r) {
        if (r.level_cnt > B) { r.mode = BY_IDX; r.idx = idx; r.waves = B; } else r.waves = r.level_cnt;
    });
}

int bsx_replay_prio_append(const BsxPrioTree* tree, const int64_t* counter, const int64_t* stored, int64_t rows, void* stream) {
    if (const int rc = check_tree(tree)) return rc;
    if (!counter || !stored || rows < 1 || rows > MAX_ROWS) return BSX_E_ARG;
    if (tree_misaligned(tree) || !aligned(counter, 8) || !aligned(stored, 8)) return BSX_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t M = tree->M;
    hipLaunchKernelGGL(bsx_prio_append_kernel, dim3(blocks(rows < M ? rows : M, TPB)), dim3(TPB), 0, s, AppendArgs{*tree, counter, stored, rows});
    if (const hipError_t e = hipGetLastError()) return int(e);
    // s <= rows rows, contiguous mod M, lie under at most (rows >> shift) + 3 nodes of a level (two segments, one of them starting at
    // node 0), and under at most all of them plus the one both segments share
    return repair(*tree, levels_of(M), s, [&](RepairArgs& r) {
        const int64_t bound = (rows >> r.shift) + 3;
        r.mode = BY_RANGE; r.counter = counter; r.stored = stored;
        r.waves = bound < r.level_cnt + 1 ? bound : r.level_cnt + 1;
    });
}

int bsx_replay_prio_weights(const BsxPrioTree* tree, const int64_t* idx, int64_t B, int nA, float* weights_out, void* workspace, void* stream) {
    if (const int rc = check_tree(tree)) return rc;
    if (!idx || !weights_out || !workspace || B < 1 || B > MAX_ROWS || nA < 1 || nA > BSX_MAX_N) return BSX_E_ARG;
    if (tree_misaligned(tree) || !aligned(idx, 8) || !aligned(weights_out, 4) || !aligned(workspace, 4)) return BSX_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const WeightArgs a{*tree, idx, static_cast<uint32_t*>(workspace), B, nA, weights_out};
    hipLaunchKernelGGL(bsx_prio_leaves_kernel, dim3(blocks(B, TPB)), dim3(TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    return weights(a, s);
}

int bsx_replay_prio_sample(const BsxReplayRing* ring, const BsxPrioTree* tree, int64_t B, uint64_t seed, uint64_t seq, const uint64_t* seq_base,
                           int64_t* idx, float* obs, float* obs_next, float* act, float* rew, uint8_t* done, float* weights_out, void* workspace,
                           void* stream) {
    if (const int rc = check_ring(ring)) return rc;
    if (const int rc = check_tree(tree)) return rc;
    if (tree->M != ring->M || B < 1 || B > MAX_ROWS || !idx || !obs || !obs_next || !act || !rew || !done || !weights_out || !workspace)
        return BSX_E_ARG;
    if (ring_misaligned(ring) || tree_misaligned(tree) || !aligned(seq_base, 8) || !aligned(idx, 8) || !aligned(obs, 4) || !aligned(obs_next, 4) ||
        !aligned(act, 4) || !aligned(rew, 4) || !aligned(weights_out, 4) || !aligned(workspace, 4)) return BSX_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* drawn = static_cast<uint32_t*>(workspace);
    const Levels lv = levels_of(tree->M);
    const DrawArgs a{*ring, *tree, lv, lv.off[lv.n - 1], B, seed, seq, seq_base, idx, drawn, obs, obs_next, act, rew, done};
    hipLaunchKernelGGL(bsx_prio_draw_kernel, dim3(blocks(B, WAVES)), dim3(TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    return weights(WeightArgs{*tree, idx, drawn, B, ring->nA, weights_out}, s);
}

}  // extern "C"
