// bsx_actor_layout.h -- the two memory layouts of the per-agent actor MLP, as host + device constexpr and nothing else: the packed weight
// blob the forward kernels read (StackedActor.pack() writes it, bsx_adam_step re-writes it) and the [A, G] gradient row bsx_actor_grad
// writes (bsx_adam_step reads it and keeps its moments in it; learner.py's _TABLE is the same row on the Python side).
// include/battlespace_hip.h states both as the public contract; the static_asserts below tie these functions to it.
#pragma once

#include "battlespace_hip.h"

namespace bsx_actor {

constexpr int H = 64;            // fc1_dims = fc2_dims = 64 (main.py:15-16)
constexpr int NA = 4;            // discrete action scores

// nid(m, v, hh): the neuron held by accumulator register v of 32-neuron MFMA tile m in lane half hh
__host__ __device__ constexpr int nid(int m, int v, int hh) { return 32 * m + (v & 3) + 8 * (v >> 2) + 4 * hh; }

// packed blob per agent (floats); Dp = obs_len rounded up to even
//   W1A[mo 2][s Dp/2][lane 64]                 W1[k = 2s + (lane>>5)][32*mo + (lane&31)], 0 for k >= D
//   W2A[mo 2][mt 2][vq 4][lane 64][t 4]        W2[k = nid(mt, 4*vq+t, lane>>5)][32*mo + (lane&31)]
//   small: b1p g1p be1p b2p g2p be2p, each [hh 2][mo 2][v 16] = value[nid(mo, v, hh)]
//   W3P[hh 2][mt 2][v 16][4]                   W3[k = nid(mt, v, hh)][0..3]
//   b3[4]
//   W2B[mo 2][s 4][term 3][lane 64][i 8] bf16  the 64 x 64 layer once more, split in bf16 terms: term 0 = bf16(W2), term 1 =
//                                              bf16(W2 - term 0), term 2 = bf16(W2 - term 0 - term 1), of
//                                              W2[k = nid(s>>1, 8*(s&1) + i, lane>>5)][32*mo + (lane&31)]
//                                              (BSX_ACTOR_BF16X3 reads terms 0-1, BSX_ACTOR_BF16X6 all three)
__host__ __device__ constexpr int dpad(int D) { return (D + 1) & ~1; }
__host__ __device__ constexpr int off_w2(int D) { return H * dpad(D); }
__host__ __device__ constexpr int off_small(int D) { return off_w2(D) + H * H; }
__host__ __device__ constexpr int off_w3(int D) { return off_small(D) + 6 * H; }
__host__ __device__ constexpr int off_b3(int D) { return off_w3(D) + H * NA; }
__host__ __device__ constexpr int off_w2b(int D) { return off_b3(D) + NA; }            // 16-byte aligned: every section is a multiple of 4 floats
__host__ __device__ constexpr int blob_floats(int D) { return off_w2b(D) + H * H * 3 / 2; }     // 3 bf16 terms = 6 bytes per weight

// float i of the W2A section holds W2[w2a_k(i)][w2a_j(i)]
__host__ __device__ constexpr int w2a_k(int i) { return nid((i >> 10) & 1, 4 * ((i >> 8) & 3) + (i & 3), (i >> 7) & 1); }
__host__ __device__ constexpr int w2a_j(int i) { return 32 * (i >> 11) + ((i >> 2) & 31); }

// gradient row per agent (floats), every tensor in its natural order: w1[D][64] | b1 g1 h1 | w2[64][64] | b2 g2 h2 | w3[64][4] | b3[4]
// (g = a LayerNorm's gain, h = its bias; w3 / b3 keep four columns whatever the head's n_actions: the pad columns hold +0)
__host__ __device__ constexpr int row_b1(int D) { return H * D; }
__host__ __device__ constexpr int row_w2(int D) { return row_b1(D) + 3 * H; }
__host__ __device__ constexpr int row_b2(int D) { return row_w2(D) + H * H; }
__host__ __device__ constexpr int row_w3(int D) { return row_b2(D) + 3 * H; }
__host__ __device__ constexpr int row_b3(int D) { return row_w3(D) + H * NA; }
__host__ __device__ constexpr int grad_floats(int D) { return H * D + H * H + 6 * H + H * NA + NA; }

static_assert(grad_floats(5) == 64 * 5 + 4096 + 6 * 64 + 260 && row_b3(5) + NA == grad_floats(5), "the gradient row of battlespace_hip.h");
static_assert(blob_floats(5) == 64 * 6 + 4096 + 6 * 64 + 260 + 6144 && blob_floats(8) == 64 * 8 + 4096 + 6 * 64 + 260 + 6144,
              "the blob of battlespace_hip.h: obs_len padded to even, then 3 bf16 terms per weight of the 64 x 64 layer");
static_assert(off_w2b(5) % 4 == 0 && off_w2b(8) % 4 == 0, "W2B is read with 16-byte loads");
static_assert(w2a_k(0) == 0 && w2a_k(3) == 3 && w2a_k(4 * 32) == 4 && w2a_k(4 * 64) == 8 && w2a_j(4 * 31) == 31 && w2a_j(2048) == 32,
              "W2A[mo][mt][vq][lane][t]");

}  // namespace bsx_actor
