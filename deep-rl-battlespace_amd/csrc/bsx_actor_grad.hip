// bsx_actor_grad.hip -- the training pass of the per-agent actor / value MLP (bsx_actor.hip's network) for an on-device learner, gfx950:
// the gradient of sum_rows <grad_out, y> in the ten parameter tensors, with the forward RECOMPUTED in registers (no activation is saved
// by the forward and none is read here) and every weight gradient reduced over the rows without a floating-point atomic.
//
// A workgroup = 4 waves of ONE agent (blockIdx.y); a wave takes one 32-row tile per ROUND, a workgroup four, and blockIdx.x strides
// over the rounds.  Per round and wave, everything in float32:
//   1. forward as tile_forward<BSX_ACTOR_F32> computes it (same operations in the same K order: layer 1 from the blob's W1A section,
//      the 64 x 64 layer with the layer-1 accumulator registers as the B operand), keeping x^ = (a - mean) * rstd and rstd of both
//      LayerNorms; head, tanh, ds = grad_out * (1 - y^2);
//   2. backward on the same register layout (rows on lanes, neurons on registers): dh2 = W3 ds, ReLU mask = (LayerNorm output > 0),
//      LayerNorm backward, dh1^T = W2 * da2^T on the matrix cores with the da2 registers as the B operand as they stand;
//   3. the sums over ROWS.  Rows sit on lanes, so each operand goes once through LDS as a [row][neuron] float32 image (row stride 65
//      floats: the lane-per-row writes fall on 32 different banks) and is read back with lane = neuron:
//        * dW2 = h1^T da2 and dW1 = x^T da1 on the matrix cores (A: lane = neuron of the left image, k = row; B: the same of the right
//          image).  The four waves SHARE their images for these two products: each wave owns one 32 x 32 tile of dW2 (16 accumulator
//          registers instead of 64) and one of dW1 and contracts it over the workgroup's 128 rows.  With D <= 32 there are only two dW1
//          tiles: the waves pair up and each takes the rows of two of the four images.
//        * the per-neuron vectors (db, dg, dbeta of both layers) and the 64 x 4 head (dW3, db3): one register per value with lane = neuron,
//          a vector pass over the wave's own 32 image rows (ds_read_b32, conflict-free; the row's ds as a broadcast 16-byte read).
//   The natural-order W2 that step 2 wants as the A operand (the blob's W2A section holds the other orientation) is un-permuted once per
//   workgroup into LDS, [k][j] with row stride 65; layer 2 of the forward reads its A operand from the same copy.
// The accumulators live in registers across the rounds; at the end the workgroup adds its four waves' vectors as (0 + 1) + (2 + 3) and writes
// ONE partial [G] row into the caller's workspace.  bsx_actor_grad_merge_kernel adds the partial rows of an agent in a fixed blocked order.
// The partition (workgroups per agent) is a function of (R, A) alone: the same inputs give the same bits on every call.
//
// The input gradient (bsx_mlp_grad with a grad_x; bsx_mlp_grad_kernel, the same body with DX): once the wave holds da1, one more transposed
// product on the matrix cores, dx^T[k][row] = sum_j W1[k][j] da1[row][j], with the da1 registers as the B operand as they stand -- the shape
// of the dh1 step -- and A = W1[k = 32 m + c][j = nid(mt, v, hh)], m < MT1 output tiles.  The A operand is read from the blob's W1A
// section in global memory: that section holds W1[2s + hh'][32 mo + c'], so the four j of a register quad (v & 3) are 16 contiguous
// bytes and a lane's 32 values of one m are eight 16-byte loads, the two lane halves of a k sharing each 128-byte line.  Not from LDS:
// the 9 456 bytes left hold a natural-order copy (row stride 65) only up to D = 36, and an image that is dead by then would have to be
// filled again every round (the images are overwritten every round), D x 64 LDS writes for as many reads.  The section is at most
// 16 KB per agent, a workgroup reads the same one every round, and nothing else of the round streams through the vector cache but x and
// grad_out: it stays resident.  dX has no sum over rows, so the weight gradients' order does not move and dX itself is deterministic.
// Lane (c, hh) holds dx[row c][k = nid(m, v, hh)] and stores it to grad_x[(row A + a) D + k] for k < D and row < R: plain dword stores
// (D may be odd: 4-byte alignment is all a row has), nothing beyond the R A D floats.
//
// Rows beyond R: the lane reads row R - 1 instead (inside the buffer) and takes grad_out = 0, so that all it contributes is an exact 0.
// LDS: 154 384 bytes per workgroup (four images per wave, 133 KB; W2 17 KB), dynamic: one workgroup per CU, one wave per SIMD -- the
// float32 matrix instruction reaches its rate from one wave.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_core.h"
#include "bsx_args.h"

namespace {

using namespace bsx_actor;

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int IS = 65;                         // image row stride (floats)
constexpr int IMG = 32 * IS;                   // one [32 rows][64 neurons] image
constexpr int NIMG = 4;                        // images per wave
constexpr int VEC = 6 * H + H * NA + NA;       // b1 g1 h1 b2 g2 h2 | w3[64][4] | b3: a wave's vector accumulators, in the order of `grad`
constexpr int LDS_SMALL = 0, LDS_W2 = LDS_SMALL + SMALL, LDS_DS = LDS_W2 + H * IS, LDS_IMG = LDS_DS + WAVES * 32 * NA;
constexpr int LDS_FLOATS = LDS_IMG + WAVES * NIMG * IMG;
static_assert(LDS_W2 % 4 == 0 && LDS_DS % 4 == 0 && LDS_FLOATS * 4 <= 163840, "LDS carve");
constexpr int MAX_WG_PER_AGENT_TOTAL = 512;    // workgroups of a launch, over all agents: two per CU

struct GradArgs {
    const float* weights; const float* obs; const float* go; float* ws;
    int64_t R; int A; int D; int squash; int rounds;
};

// workgroups per agent: a function of (R, A) alone
inline int partials(int64_t R, int A) {
    const int64_t rounds = ((R + 31) / 32 + WAVES - 1) / WAVES;
    const int64_t cap = MAX_WG_PER_AGENT_TOTAL / A > 0 ? MAX_WG_PER_AGENT_TOTAL / A : 1;
    return int(rounds < cap ? rounds : cap);
}

// a wave's LDS writes, ordered before its own later reads from other lanes (the LDS executes one wave's instructions in order)
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// LayerNorm backward on one tile, in place: d = dy in, da out.  dx^ = dy g,  da = rstd (dx^ - mean64(dx^) - x^ mean64(dx^ x^))
__device__ inline void ln_backward(f32x16& d0, f32x16& d1, const f32x16& x0, const f32x16& x1, float rstd, const float* __restrict__ gp) {
#pragma clang fp contract(fast)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) { d0[v] *= gp[v]; s1 += d0[v]; s2 += d0[v] * x0[v]; }
#pragma unroll
    for (int v = 0; v < 16; ++v) { d1[v] *= gp[16 + v]; s1 += d1[v]; s2 += d1[v] * x1[v]; }
    s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
    const float m1 = s1 * (1.0f / H), m2 = s2 * (1.0f / H);
#pragma unroll
    for (int v = 0; v < 16; ++v) d0[v] = rstd * (d0[v] - m1 - x0[v] * m2);
#pragma unroll
    for (int v = 0; v < 16; ++v) d1[v] = rstd * (d1[v] - m1 - x1[v] * m2);
}

// the lane's 32 values (row c = lane & 31, neurons nid(mo, v, hh)) to / from a [row][neuron] image
// An LDS index made opaque where it is used: left to itself the compiler keeps some fifty loop-invariant addresses of the unrolled
// accesses (one per far offset of a paired read) in registers across the whole round loop, which the register file has no room for.
// (The INDEX, not the pointer: a pointer that went through an asm statement is a generic one, and its accesses become flat_ ones.)
__device__ inline int here(int i) {
    asm volatile("" : "+v"(i));
    return i;
}

__device__ inline void img_write(float* lds, int I, int c, int hh, const f32x16& t0, const f32x16& t1) {
    float* q = lds + here(I + c * IS + 4 * hh);
#pragma unroll
    for (int v = 0; v < 16; ++v) { q[nid(0, v, 0)] = t0[v]; q[nid(1, v, 0)] = t1[v]; }
}
__device__ inline void img_read(const float* lds, int I, int c, int hh, f32x16& t0, f32x16& t1) {
    const float* q = lds + here(I + c * IS + 4 * hh);
#pragma unroll
    for (int v = 0; v < 16; ++v) { t0[v] = q[nid(0, v, 0)]; t1[v] = q[nid(1, v, 0)]; }
}

// the workgroup's LDS (LDS_FLOATS floats), sized at the launch.  Dynamic and not a static array so that the register budget below holds:
// told that one workgroup fills the LDS of a CU, the compiler plans for one wave per SIMD and lets the kernel's vector registers run
// past 256 into the accumulation file (some thirty long-lived addresses and lane constants parked there, a copy at every use)
extern __shared__ __attribute__((aligned(16))) float lds[];

// MT1: 32-row tiles of dW1 (D <= 32: 1, else 2).  (TPB, 2): two waves per SIMD = at most 256 vector registers
template <int MT1>
__global__ __launch_bounds__(TPB, 2) void bsx_actor_grad_kernel(const GradArgs p) {
#pragma clang fp contract(fast)
    constexpr bool DX = false;
    [[maybe_unused]] float* const gx = nullptr;
#include "bsx_actor_grad_body.inl"
}

// The same pass with the input gradient written as well (bsx_mlp_grad with a grad_x): a kernel of its own and not a runtime branch, so
// that the kernels above stay the binaries they were.  (A distinct name, not a second template parameter: the ISA table keys these
// kernels by their first one.)
struct MlpGradArgs { GradArgs g; float* gx; };
template <int MT1>
__global__ __launch_bounds__(TPB, 2) void bsx_mlp_grad_kernel(const MlpGradArgs pm) {
#pragma clang fp contract(fast)
    constexpr bool DX = true;
    const GradArgs& p = pm.g;
    float* const gx = pm.gx;
#include "bsx_actor_grad_body.inl"
}

// grad[a][i] = the sum of the agent's partial rows in a fixed order (overwrites grad): element i belongs to four threads, thread j adds
// the rows q = j, j + 4, j + 8, .. in runs of eight (each run summed from 0, then added to the thread's sum), and the four sums are
// added as (0 + 1) + (2 + 3) -- chains of 8 and P / 32 instead of one of P
__global__ __launch_bounds__(256) void bsx_actor_grad_merge_kernel(const float* __restrict__ ws, float* __restrict__ grad, int G, int P) {
    __shared__ float part[4][64];
    const int e = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + e, a = blockIdx.y;
    float g = 0.f;
    if (i < G) {
        const float* src = ws + size_t(a) * P * G + i;
        for (int q0 = j; q0 < P; q0 += 32) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (q0 + 4 * k < P) t += src[size_t(q0 + 4 * k) * G];
            g += t;
        }
    }
    part[j][e] = g;
    __syncthreads();
    if (j == 0 && i < G) grad[size_t(a) * G + i] = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
}

// more than 64 KB of dynamic LDS has to be allowed per kernel, once per process (not a stream operation)
int allow_lds() {
    static const int rc = [] {
        int r = 0;
        for (const void* k : {reinterpret_cast<const void*>(&bsx_actor_grad_kernel<1>), reinterpret_cast<const void*>(&bsx_actor_grad_kernel<2>),
                              reinterpret_cast<const void*>(&bsx_mlp_grad_kernel<1>), reinterpret_cast<const void*>(&bsx_mlp_grad_kernel<2>)})
            if (r == 0) r = int(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, int(LDS_FLOATS * sizeof(float))));
        return r;
    }();
    return rc;
}

// one training pass on checked arguments: the round kernel (with gx, the form that writes the input gradient), then the merge
int launch_grad(const float* weights, const float* x, const float* grad_out, int64_t R, int A, int D, int squash, float* grad, float* gx,
                void* workspace, void* stream) {
    const int P = partials(R, A), G = grad_floats(D);
    const int64_t tiles = (R + 31) / 32;
    const int rounds = int((tiles + int64_t(WAVES) * P - 1) / (int64_t(WAVES) * P));
    const GradArgs g{weights, x, grad_out, static_cast<float*>(workspace), R, A, D, squash, rounds};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = allow_lds()) return rc;
    const dim3 grid = dim3(unsigned(P), unsigned(A));
    if (gx) {
        const MlpGradArgs m{g, gx};
        if (D <= 32) hipLaunchKernelGGL(bsx_mlp_grad_kernel<1>, grid, dim3(TPB), LDS_FLOATS * sizeof(float), s, m);
        else hipLaunchKernelGGL(bsx_mlp_grad_kernel<2>, grid, dim3(TPB), LDS_FLOATS * sizeof(float), s, m);
    } else {
        if (D <= 32) hipLaunchKernelGGL(bsx_actor_grad_kernel<1>, grid, dim3(TPB), LDS_FLOATS * sizeof(float), s, g);
        else hipLaunchKernelGGL(bsx_actor_grad_kernel<2>, grid, dim3(TPB), LDS_FLOATS * sizeof(float), s, g);
    }
    if (const int rc = int(hipGetLastError())) return rc;
    hipLaunchKernelGGL(bsx_actor_grad_merge_kernel, dim3(unsigned((G + 63) / 64), unsigned(A)), dim3(256), 0, s,
                       static_cast<const float*>(workspace), grad, G, P);
    return int(hipGetLastError());
}

}  // namespace

extern "C" {

int bsx_actor_grad_floats(int obs_len, int* floats_per_agent) {
    if (obs_len < 1 || obs_len > 3 * BSX_MAX_N + 2 || !floats_per_agent) return BSX_E_ARG;
    *floats_per_agent = grad_floats(obs_len);
    return 0;
}

// The two observation-shaped entries are bsx_mlp_grad's at (A, D) = (2n, 3n + 2) with no grad_x: the team size is checked here (it is
// what 2n and 3n + 2 are made of), everything else there -- every BSX_E_ARG before every BSX_E_ALIGN, weights and grad_out at 16 bytes.
int bsx_actor_grad_workspace_bytes(int64_t R, int n, size_t* bytes) {
    if (n < 1 || n > BSX_MAX_N) return BSX_E_ARG;
    return bsx_mlp_grad_workspace_bytes(R, 2 * n, 3 * n + 2, bytes);
}

int bsx_actor_grad(const float* weights, const float* obs, const float* grad_out, int64_t R, int n, int squash,
                   float* grad, void* workspace, void* stream) {
    if (n < 1 || n > BSX_MAX_N) return BSX_E_ARG;
    return bsx_mlp_grad(weights, obs, grad_out, R, 2 * n, 3 * n + 2, squash, grad, nullptr, workspace, stream);
}

int bsx_mlp_grad_workspace_bytes(int64_t R, int A, int D, size_t* bytes) {
    if (!bytes || !mlp_shape(R, A, D)) return BSX_E_ARG;
    *bytes = size_t(A) * size_t(partials(R, A)) * size_t(grad_floats(D)) * sizeof(float);
    return 0;
}

int bsx_mlp_grad(const float* weights, const float* x, const float* grad_out, int64_t R, int A, int D, int squash,
                 float* grad, float* grad_x, void* workspace, void* stream) {
    if (!x || !grad_out || !grad || !workspace || (squash != 0 && squash != 1)) return BSX_E_ARG;
    if (!weights || !mlp_shape(R, A, D)) return BSX_E_ARG;
    if (!aligned(weights, 16) || !aligned(grad_out, 16) || !aligned(x, 4) || !aligned(grad, 4) || !aligned(grad_x, 4) || !aligned(workspace, 4))
        return BSX_E_ALIGN;
    return launch_grad(weights, x, grad_out, R, A, D, squash, grad, grad_x, workspace, stream);
}

}  // extern "C"
