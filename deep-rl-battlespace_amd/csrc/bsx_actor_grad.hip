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
// The partition (workgroups per agent) is a function of (R, n) alone: the same inputs give the same bits on every call.
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

// workgroups per agent: a function of (R, n) alone
inline int partials(int64_t R, int n) {
    const int64_t rounds = ((R + 31) / 32 + WAVES - 1) / WAVES;
    const int64_t cap = MAX_WG_PER_AGENT_TOTAL / (2 * n) > 0 ? MAX_WG_PER_AGENT_TOTAL / (2 * n) : 1;
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
    const int D = p.D, Dp = dpad(D), G = grad_floats(D);
    const int a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, c = lane & 31;
    const float* __restrict__ W = p.weights + size_t(a) * blob_floats(D);

    float* s_small = lds + LDS_SMALL;
    float* s_w2 = lds + LDS_W2;                                   // W2[k][j], natural order, row stride IS
    // (indices into lds, not pointers: see here())
    const int DS = LDS_DS + wave * 32 * NA;                       // this wave's ds rows, [row][4]
    const int I0 = LDS_IMG + (wave * NIMG + 0) * IMG;             // x^1
    const int I1 = I0 + IMG;                                      // h1, then x          (shared: left operand of dW2, dW1)
    const int I2 = I1 + IMG;                                      // x^2, then da2, da1  (shared: right operand of dW2, dW1)
    const int I3 = I2 + IMG;                                      // h2, dy2, dy1
    for (int i = tid; i < SMALL / 4; i += TPB)
        reinterpret_cast<float4*>(s_small)[i] = reinterpret_cast<const float4*>(W + off_small(D))[i];
    for (int i = tid; i < H * H; i += TPB) s_w2[w2a_k(i) * IS + w2a_j(i)] = W[off_w2(D) + i];     // the W2A section, un-permuted
    __syncthreads();
    const float4 b3 = *reinterpret_cast<const float4*>(s_small + 6 * H + H * NA);

    f32x16 accW2, accW1;
    float4 accW3 = make_float4(0.f, 0.f, 0.f, 0.f), accB3 = accW3;
    float db1 = 0.f, dg1 = 0.f, dh1v = 0.f, db2 = 0.f, dg2 = 0.f, dh2v = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) { accW2[v] = 0.f; accW1[v] = 0.f; }

#pragma nounroll
    for (int round = 0; round < p.rounds; ++round) {
        const int64_t en = ((int64_t(round) * gridDim.x + blockIdx.x) * WAVES + wave) * 32 + c;
        const bool valid = en < p.R;
        const size_t row = size_t(valid ? en : p.R - 1) * p.A + a;
        const float* __restrict__ xr = p.obs + row * D;
        float4 go = reinterpret_cast<const float4*>(p.go)[row];
        if (!valid) go = make_float4(0.f, 0.f, 0.f, 0.f);
        // the per-neuron vectors are read where they are used, every round: hoisted out of the loop (~300 loop-invariant LDS values)
        // they would not fit the register file
        const float* ssm = lds + here(LDS_SMALL);
        const float* sm = ssm + hh * 32;                          // this lane half's [mo][v] slice of each 64-float vector

        // ---- forward, layer 1
        f32x16 t0, t1, x0, x1;                                    // t: a tile's 64 neurons (two 32-neuron halves); x: its x^
#pragma unroll
        for (int v = 0; v < 16; ++v) { t0[v] = sm[0 * H + v]; t1[v] = sm[0 * H + 16 + v]; }
        for (int s = 0; s < Dp / 2; ++s) {
            const int k = 2 * s + hh;
            const float a0 = W[(0 * (Dp / 2) + s) * 64 + lane], a1 = W[(1 * (Dp / 2) + s) * 64 + lane];
            const float b = k < D ? xr[k] : 0.f;
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, t1, 0, 0, 0);
        }
        const float rstd1 = ln_relu_tile(t0, t1, sm + 1 * H, sm + 2 * H, ln_keep{x0, x1});
        img_write(lds, I0, c, hh, x0, x1);
        img_write(lds, I1, c, hh, t0, t1);
        // ---- layer 2: the K index runs over layer 1's accumulator registers, in tile_forward's order
        f32x16 u0, u1;
#pragma unroll
        for (int v = 0; v < 16; ++v) { u0[v] = sm[3 * H + v]; u1[v] = sm[3 * H + 16 + v]; }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const float* wq = lds + here(LDS_W2 + (32 * mt + 4 * hh) * IS + c);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float* wrow = wq + nid(0, v, 0) * IS;
                const float hv = mt == 0 ? t0[v] : t1[v];
                u0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[0], hv, u0, 0, 0, 0);
                u1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[32], hv, u1, 0, 0, 0);
            }
        }
        const float rstd2 = ln_relu_tile(u0, u1, sm + 4 * H, sm + 5 * H, ln_keep{x0, x1});
        img_write(lds, I3, c, hh, u0, u1);
        // ---- head, ds
        const float4* w3 = reinterpret_cast<const float4*>(ssm + 6 * H) + hh * 32;   // [hh][mt][v] float4
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float4 ww = w3[v];
            o.x = fmaf(u0[v], ww.x, o.x); o.y = fmaf(u0[v], ww.y, o.y); o.z = fmaf(u0[v], ww.z, o.z); o.w = fmaf(u0[v], ww.w, o.w);
            if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (four head rows in flight, not all 32: 128 registers)
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float4 ww = w3[16 + v];
            o.x = fmaf(u1[v], ww.x, o.x); o.y = fmaf(u1[v], ww.y, o.y); o.z = fmaf(u1[v], ww.z, o.z); o.w = fmaf(u1[v], ww.w, o.w);
            if ((v & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        o.x += __shfl_xor(o.x, 32); o.y += __shfl_xor(o.y, 32); o.z += __shfl_xor(o.z, 32); o.w += __shfl_xor(o.w, 32);
        float4 ds = go;
        if (p.squash) {
            const float y0 = tanhf(o.x + b3.x), y1 = tanhf(o.y + b3.y), y2 = tanhf(o.z + b3.z), y3 = tanhf(o.w + b3.w);
            ds.x *= fmaf(-y0, y0, 1.0f); ds.y *= fmaf(-y1, y1, 1.0f); ds.z *= fmaf(-y2, y2, 1.0f); ds.w *= fmaf(-y3, y3, 1.0f);
        }
        if (hh == 0) reinterpret_cast<float4*>(lds + DS)[c] = ds;
        wave_lds_sync();
        // ---- dW3 = h2^T ds, db3 = sum ds: lane = neuron over the wave's 32 rows
        //      (every vector pass sums its 32 rows from 0, as interleaved chains added pairwise, and adds the tile's sum to the
        //       accumulator: the chains stay short)
        {
            float4 tw[2], tb[2];                                  // (two chains of 16 here: four would take 32 registers)
            const float* pa = lds + here(I3 + lane);
            const float4* pd = reinterpret_cast<const float4*>(lds + here(DS));
#pragma unroll
            for (int j = 0; j < 2; ++j) { tw[j] = make_float4(0.f, 0.f, 0.f, 0.f); tb[j] = tw[j]; }
#pragma unroll 2
            for (int r = 0; r < 32; r += 2)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float hv = pa[(r + j) * IS];
                    const float4 d4 = pd[r + j];
                    float4& w = tw[j]; float4& b = tb[j];
                    w.x = fmaf(hv, d4.x, w.x); w.y = fmaf(hv, d4.y, w.y); w.z = fmaf(hv, d4.z, w.z); w.w = fmaf(hv, d4.w, w.w);
                    b.x += d4.x; b.y += d4.y; b.z += d4.z; b.w += d4.w;
                }
            accW3.x += tw[0].x + tw[1].x; accW3.y += tw[0].y + tw[1].y; accW3.z += tw[0].z + tw[1].z; accW3.w += tw[0].w + tw[1].w;
            accB3.x += tb[0].x + tb[1].x; accB3.y += tb[0].y + tb[1].y; accB3.z += tb[0].z + tb[1].z; accB3.w += tb[0].w + tb[1].w;
        }
        // ---- dy2 = (h2 > 0) * W3 ds, in place of h2
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float4 w0 = w3[v], w1 = w3[16 + v];
            const float e0 = fmaf(w0.w, ds.w, fmaf(w0.z, ds.z, fmaf(w0.y, ds.y, w0.x * ds.x)));
            const float e1 = fmaf(w1.w, ds.w, fmaf(w1.z, ds.z, fmaf(w1.y, ds.y, w1.x * ds.x)));
            u0[v] = u0[v] > 0.f ? e0 : 0.f;
            u1[v] = u1[v] > 0.f ? e1 : 0.f;
            if ((v & 1) == 1) __builtin_amdgcn_sched_barrier(0);
        }
        wave_lds_sync();                                          // (the pass over h2 is done with I3)
        img_write(lds, I3, c, hh, u0, u1);
        img_write(lds, I2, c, hh, x0, x1);
        wave_lds_sync();
        // ---- dbeta2 = sum dy2, dg2 = sum dy2 x^2
        {
            float tb[4] = {0.f, 0.f, 0.f, 0.f}, tg[4] = {0.f, 0.f, 0.f, 0.f};
            const float* pa = lds + here(I3 + lane);
            const float* pb = lds + here(I2 + lane);
#pragma unroll 2
            for (int r = 0; r < 32; r += 4)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dy = pa[(r + j) * IS], xh = pb[(r + j) * IS];
                    tb[j] += dy; tg[j] = fmaf(dy, xh, tg[j]);
                }
            dh2v += (tb[0] + tb[1]) + (tb[2] + tb[3]); dg2 += (tg[0] + tg[1]) + (tg[2] + tg[3]);
        }
        ln_backward(u0, u1, x0, x1, rstd2, sm + 4 * H);           // u = da2
        wave_lds_sync();
        img_write(lds, I2, c, hh, u0, u1);
        wave_lds_sync();
        {
            float tb[4] = {0.f, 0.f, 0.f, 0.f};
            const float* pa = lds + here(I2 + lane);
#pragma unroll 2
            for (int r = 0; r < 32; r += 4)
#pragma unroll
                for (int j = 0; j < 4; ++j) tb[j] += pa[(r + j) * IS];
            db2 += (tb[0] + tb[1]) + (tb[2] + tb[3]);
        }
        // ---- dh1^T = W2 da2^T: the da2 registers are the B operand as they stand; A = W2[k = 32 mo + c][j = nid(mt, v, hh)]
#pragma unroll
        for (int v = 0; v < 16; ++v) { t0[v] = 0.f; t1[v] = 0.f; }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const float* wq = lds + here(LDS_W2 + c * IS + 32 * mt + 4 * hh);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float* wcol = wq + nid(0, v, 0);
                const float dv = mt == 0 ? u0[v] : u1[v];
                t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[0], dv, t0, 0, 0, 0);
                t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[32 * IS], dv, t1, 0, 0, 0);
            }
        }
        __syncthreads();                                          // every wave's h1 (I1) and da2 (I2) are in place
        // ---- dW2 = h1^T da2 over the workgroup's 128 rows: this wave's tile (rows 32 (wave>>1) .. of dW2, columns 32 (wave&1) ..)
        {
            int L = LDS_IMG + 1 * IMG + hh * IS + 32 * (wave >> 1) + c, Rr = LDS_IMG + 2 * IMG + hh * IS + 32 * (wave & 1) + c;
#pragma nounroll
            for (int w = 0; w < WAVES; ++w) {
                const float* lp = lds + here(L);
                const float* rp = lds + here(Rr);
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    accW2 = __builtin_amdgcn_mfma_f32_32x32x2f32(lp[2 * s * IS], rp[2 * s * IS], accW2, 0, 0, 0);
                L += NIMG * IMG; Rr += NIMG * IMG;
            }
        }
        __syncthreads();                                          // I1 / I2 may be overwritten
        // ---- layer 1 backward: dy1 = (h1 > 0) * dh1 (the mask from the stored LayerNorm output itself)
        img_read(lds, I1, c, hh, u0, u1);
#pragma unroll
        for (int v = 0; v < 16; ++v) { t0[v] = u0[v] > 0.f ? t0[v] : 0.f; t1[v] = u1[v] > 0.f ? t1[v] : 0.f; }
        img_read(lds, I0, c, hh, x0, x1);
        img_write(lds, I3, c, hh, t0, t1);
        wave_lds_sync();                                          // (both lanes of a row are done reading its h1)
        float* px = lds + here(I1 + c * IS + hh);
        for (int s = 0; s < 16 * MT1; ++s) {                    // x as a [row][k] image, 0 for D <= k < 32 MT1
            const int k = 2 * s + hh;
            px[2 * s] = k < D ? xr[k] : 0.f;
        }
        wave_lds_sync();
        {
            float tb[4] = {0.f, 0.f, 0.f, 0.f}, tg[4] = {0.f, 0.f, 0.f, 0.f};
            const float* pa = lds + here(I3 + lane);
            const float* pb = lds + here(I0 + lane);
#pragma unroll 2
            for (int r = 0; r < 32; r += 4)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dy = pa[(r + j) * IS], xh = pb[(r + j) * IS];
                    tb[j] += dy; tg[j] = fmaf(dy, xh, tg[j]);
                }
            dh1v += (tb[0] + tb[1]) + (tb[2] + tb[3]); dg1 += (tg[0] + tg[1]) + (tg[2] + tg[3]);
        }
        ln_backward(t0, t1, x0, x1, rstd1, sm + 1 * H);           // t = da1
        img_write(lds, I2, c, hh, t0, t1);
        wave_lds_sync();
        {
            float tb[4] = {0.f, 0.f, 0.f, 0.f};
            const float* pa = lds + here(I2 + lane);
#pragma unroll 2
            for (int r = 0; r < 32; r += 4)
#pragma unroll
                for (int j = 0; j < 4; ++j) tb[j] += pa[(r + j) * IS];
            db1 += (tb[0] + tb[1]) + (tb[2] + tb[3]);
        }
        __syncthreads();                                          // every wave's x (I1) and da1 (I2) are in place
        // ---- dW1 = x^T da1.  MT1 = 2: one of the four tiles per wave over all 128 rows; MT1 = 1: tile (wave & 1) over the rows of
        //      the images of waves 2 (wave >> 1) and 2 (wave >> 1) + 1 -- the two halves are added at the end
        {
            const int mt = MT1 == 2 ? wave >> 1 : 0, w0 = MT1 == 2 ? 0 : 2 * (wave >> 1);
            int L = LDS_IMG + (w0 * NIMG + 1) * IMG + hh * IS + 32 * mt + c, Rr = LDS_IMG + (w0 * NIMG + 2) * IMG + hh * IS + 32 * (wave & 1) + c;
#pragma nounroll
            for (int w = 0; w < (MT1 == 2 ? WAVES : 2); ++w) {
                const float* lp = lds + here(L);
                const float* rp = lds + here(Rr);
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    accW1 = __builtin_amdgcn_mfma_f32_32x32x2f32(lp[2 * s * IS], rp[2 * s * IS], accW1, 0, 0, 0);
                L += NIMG * IMG; Rr += NIMG * IMG;
            }
        }
        __syncthreads();                                          // the images may be overwritten by the next round
    }

    // ---- this workgroup's partial row: [w1 | b1 g1 h1 | w2 | b2 g2 h2 | w3 | b3]
    // (the thread's indices are derived again here: kept from the top they would be live, in registers, across the whole round loop)
    const int etid = here(int(threadIdx.x)), el = etid & 63, ew = etid >> 6, eh = el >> 5, ec = el & 31;
    float* __restrict__ out = p.ws + (size_t(a) * gridDim.x + blockIdx.x) * G;
    float* red = lds + LDS_IMG;                                   // [wave][VEC], then the upper waves' dW1 tiles
#pragma unroll
    for (int v = 0; v < 16; ++v)
        out[row_w2(D) + nid(ew >> 1, v, eh) * H + 32 * (ew & 1) + ec] = accW2[v];
    red[ew * VEC + 0 * H + el] = db1; red[ew * VEC + 1 * H + el] = dg1; red[ew * VEC + 2 * H + el] = dh1v;
    red[ew * VEC + 3 * H + el] = db2; red[ew * VEC + 4 * H + el] = dg2; red[ew * VEC + 5 * H + el] = dh2v;
    red[ew * VEC + 6 * H + el * NA + 0] = accW3.x; red[ew * VEC + 6 * H + el * NA + 1] = accW3.y;
    red[ew * VEC + 6 * H + el * NA + 2] = accW3.z; red[ew * VEC + 6 * H + el * NA + 3] = accW3.w;
    if (el == 0) {
        red[ew * VEC + 6 * H + H * NA + 0] = accB3.x; red[ew * VEC + 6 * H + H * NA + 1] = accB3.y;
        red[ew * VEC + 6 * H + H * NA + 2] = accB3.z; red[ew * VEC + 6 * H + H * NA + 3] = accB3.w;
    }
    float* red1 = red + WAVES * VEC;                              // [wave - 2][v][lane]
    if (MT1 == 1 && ew >= 2) {
#pragma unroll
        for (int v = 0; v < 16; ++v) red1[((ew - 2) * 16 + v) * 64 + el] = accW1[v];
    }
    __syncthreads();
    if (MT1 == 2 || ew < 2) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int k = nid(MT1 == 2 ? ew >> 1 : 0, v, eh);
            float g = accW1[v];
            if (MT1 == 1) g += red1[(ew * 16 + v) * 64 + el];
            if (k < D) out[k * H + 32 * (ew & 1) + ec] = g;
        }
    }
    for (int i = etid; i < VEC; i += TPB) {
        const float g = (red[0 * VEC + i] + red[1 * VEC + i]) + (red[2 * VEC + i] + red[3 * VEC + i]);
        out[i < 3 * H ? row_b1(D) + i : row_b1(D) + H * H + i] = g;           // VEC is the row from b1 on with w2 (H * H floats) taken out
    }
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
        int r = int(hipFuncSetAttribute(reinterpret_cast<const void*>(&bsx_actor_grad_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        int(LDS_FLOATS * sizeof(float))));
        if (r == 0)
            r = int(hipFuncSetAttribute(reinterpret_cast<const void*>(&bsx_actor_grad_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        int(LDS_FLOATS * sizeof(float))));
        return r;
    }();
    return rc;
}

}  // namespace

extern "C" {

int bsx_actor_grad_floats(int obs_len, int* floats_per_agent) {
    if (obs_len < 1 || obs_len > 3 * BSX_MAX_N + 2 || !floats_per_agent) return BSX_E_ARG;
    *floats_per_agent = grad_floats(obs_len);
    return 0;
}

int bsx_actor_grad_workspace_bytes(int64_t R, int n, size_t* bytes) {
    if (!bytes || R < 1 || R > BSX_MAX_E || n < 1 || n > BSX_MAX_N) return BSX_E_ARG;
    *bytes = size_t(2 * n) * size_t(partials(R, n)) * size_t(grad_floats(3 * n + 2)) * sizeof(float);
    return 0;
}

int bsx_actor_grad(const float* weights, const float* obs, const float* grad_out, int64_t R, int n, int squash,
                   float* grad, void* workspace, void* stream) {
    if (!obs || !grad_out || !grad || !workspace || (squash != 0 && squash != 1)) return BSX_E_ARG;
    if (const int rc = check_games(weights, R, n, 16)) return rc;
    if (!aligned(grad_out, 16) || !aligned(obs, 4) || !aligned(grad, 4) || !aligned(workspace, 4)) return BSX_E_ALIGN;
    const int A = 2 * n, D = 3 * n + 2, P = partials(R, n), G = grad_floats(D);
    const int64_t tiles = (R + 31) / 32;
    const int rounds = int((tiles + int64_t(WAVES) * P - 1) / (int64_t(WAVES) * P));
    const GradArgs g{weights, obs, grad_out, static_cast<float*>(workspace), R, A, D, squash, rounds};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = allow_lds()) return rc;
    if (D <= 32) hipLaunchKernelGGL(bsx_actor_grad_kernel<1>, dim3(unsigned(P), unsigned(A)), dim3(TPB), LDS_FLOATS * sizeof(float), s, g);
    else hipLaunchKernelGGL(bsx_actor_grad_kernel<2>, dim3(unsigned(P), unsigned(A)), dim3(TPB), LDS_FLOATS * sizeof(float), s, g);
    if (const int rc = int(hipGetLastError())) return rc;
    hipLaunchKernelGGL(bsx_actor_grad_merge_kernel, dim3(unsigned((G + 63) / 64), unsigned(A)), dim3(256), 0, s,
                       static_cast<const float*>(workspace), grad, G, P);
    return int(hipGetLastError());
}

}  // extern "C"
