// bsx_actor.hip -- fused per-agent actor MLP for the on-device policy rollout (BASELINE.json configs[4]), gfx950.
//
// Replaces, for the rollout path, the reference's per-agent `ActorNetwork.forward` + noise + clamp
// (maddpg/networks.py:81-85, maddpg/agent.py:25-33): obs[D] -> Linear 64 -> LayerNorm -> ReLU -> Linear 64 ->
// LayerNorm -> ReLU -> Linear 4 -> tanh (-> + N(0, std) -> clamp(-1, 1)), one independent weight set per agent.
// Composed from torch ops this is ~20 memory-bound passes over [A, E, 64] activations (420 us per tick at
// 65 536 x 1v1); fused, a row never leaves the register file: 4*D bytes in, 16 bytes out.
//
// This is the one GEMM-shaped op of the project, so it runs on the matrix cores: v_mfma_f32_32x32x2_f32 (f32 in, f32
// accumulate -- bit-for-bit an fmaf chain, no reduced precision).  Everything is computed TRANSPOSED,
//     H^T [64 neurons x 64 rows] = W^T [64 x K] * X^T [K x 64 rows],
// so that a wave's 64 observation rows sit on the N (lane) axis and neurons on the M (register) axis:
//   * A operand = weights, one VGPR per k-step and 32-neuron tile, loaded once per wave (the 64x64 layer is 64 VGPRs);
//   * B operand of layer 1 = observation values straight from memory;
//   * B operand of layer 2 = the ACCUMULATOR REGISTERS of layer 1 as they stand: register v of tile mt in lane l holds
//     neuron 32*mt + (v&3) + 8*(v>>2) + 4*(l>>5) of row (l&31) -- exactly a (k_lo, k_hi) pair of a K=2 step.  The K order
//     is therefore permuted; the host packs W2 in the same order, and a sum does not care.  No LDS, no shuffles.
//   * LayerNorm needs a row's 64 neurons: 32 registers of the lane plus the partner lane l^32 -> one xor-32 shuffle.
//   * the 64 -> 4 head is 128 VALU FMAs per lane on the accumulator registers plus the same xor-32 add.
// A workgroup = 4 waves x 64 rows of ONE agent (blockIdx.y); the small per-neuron vectors and the head weights are
// staged once in LDS.  Checked against a float64 reference at a small multiple of float32's own error (tests/test_hip_actor_float64.py), not bit-exact with torch; bit-exact with the fused
// rollout kernel, which runs the same per-tile arithmetic (bsx_actor_core.h): both files are built with -ffp-contract=off
// (so that library code such as tanhf compiles the same in both) and the core functions pin contraction themselves.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_core.h"
#include "bsx_args.h"

namespace {

using namespace bsx_actor;       // H, NA, SMALL, blob layout, ln_relu_tile, finish_row (shared with the fused rollout kernel)

constexpr int TPB = 256;
constexpr int ROWS_PER_WAVE = 64;

struct ActorArgs {
    const float* weights; const float* obs; float* scores;
    int64_t E; int A; int D; BsxActorNoise nz; uint64_t seed; uint64_t seq; const uint64_t* seq_base; int64_t env_offset;
};

// PREC = BSX_ACTOR_F32: exact f32, both 32-row tiles of the wave interleaved (four independent accumulators).
// PREC = BSX_ACTOR_BF16X3 / _BF16X6: the 64 x 64 layer as split-bf16 MFMAs (bsx_actor_core.h), one tile after the other.
template <int PREC>
__global__ __launch_bounds__(TPB) void bsx_actor_kernel(const ActorArgs p) {
#pragma clang fp contract(fast)
    constexpr bool GAUSS = false;
    [[maybe_unused]] constexpr BsxGaussianHead gh = {nullptr, nullptr};
#include "bsx_actor_body.inl"
}

// The same rows finished by the Gaussian policy head (finish_row<true>, bsx_actor_forward_gaussian): a kernel of its own and not a runtime
// branch of bsx_actor_kernel, so that the plain kernels keep their registers -- the bf16 forms sit a few below 128, past which a SIMD holds
// one wave fewer.  (A distinct name, not a second template parameter: the ISA table keys these kernels by their first one.)
struct GaussianArgs { ActorArgs a; BsxGaussianHead gh; };
template <int PREC>
__global__ __launch_bounds__(TPB) void bsx_actor_gaussian_kernel(const GaussianArgs pg) {
#pragma clang fp contract(fast)
    constexpr bool GAUSS = true;
    const ActorArgs& p = pg.a;
    const BsxGaussianHead& gh = pg.gh;
#include "bsx_actor_body.inl"
}

}  // namespace

extern "C" {

int bsx_actor_blob_floats(int obs_len, int* floats_per_agent) {
    if (obs_len < 1 || obs_len > 3 * BSX_MAX_N + 2 || !floats_per_agent) return BSX_E_ARG;
    *floats_per_agent = blob_floats(obs_len);
    return 0;
}

// bsx_actor_forward and, with `gauss`, bsx_actor_forward_gaussian (the head's checks interleaved with the plain ones in a fixed order)
static int actor_forward(const float* weights, const float* obs, float* scores, int64_t E, int n, int precision, const BsxActorNoise* noise,
                         bool gauss, const BsxGaussianHead* head, uint64_t seed, uint64_t seq, const uint64_t* seq_base, int64_t env_offset,
                         void* stream) {
    if (!obs || !scores || (precision != BSX_ACTOR_F32 && precision != BSX_ACTOR_BF16X3 && precision != BSX_ACTOR_BF16X6)) return BSX_E_ARG;
    if (gauss && (!head || !head->log_std)) return BSX_E_ARG;
    if (const int rc = check_games(weights, E, n, 16)) return rc;
    if (!aligned(scores, 16) || !aligned(obs, 4)) return BSX_E_ALIGN;
    BsxActorNoise nz = {};
    if (noise) nz = *noise;
    if (gauss) {
        if (nz.gaussian_std > 0.f || nz.ou_scale > 0.f || nz.sample_mode != 0 || nz.u_inject || nz.logp) return BSX_E_ARG;
        if (!aligned(head->log_std, 4) || (head->logp && !aligned(head->logp, 4))) return BSX_E_ALIGN;
    }
    // epsilon-greedy replaces the exploration noise and both stochastic heads; the record of its draws needs it
    if (nz.epsilon ? (nz.gaussian_std > 0.f || nz.ou_scale > 0.f || nz.sample_mode != 0 || gauss) : nz.explored != nullptr) return BSX_E_ARG;
    if (nz.ou_scale > 0.f && (!nz.ou_state || !aligned(nz.ou_state, 16))) return nz.ou_state ? BSX_E_ALIGN : BSX_E_ARG;
    if (nz.z_inject && !aligned(nz.z_inject, 16)) return BSX_E_ALIGN;
    if (nz.sample_mode != 0 && (nz.sample_mode != 1 || !(nz.temperature > 0.f))) return BSX_E_ARG;
    if ((nz.u_inject && !aligned(nz.u_inject, 16)) || (nz.logp && !aligned(nz.logp, 4)) || (nz.value_weights && !aligned(nz.value_weights, 16)) ||
        (nz.epsilon && !aligned(nz.epsilon, 4))) return BSX_E_ALIGN;
    if (nz.value_weights && (!nz.value || !aligned(nz.value, 4))) return nz.value ? BSX_E_ALIGN : BSX_E_ARG;
    if (env_offset < 0) return BSX_E_ARG;
    const int A = 2 * n, D = 3 * n + 2;
    ActorArgs a{weights, obs, scores, E, A, D, nz, seed, seq, seq_base, env_offset};
    const int rows_per_block = (TPB / 64) * ROWS_PER_WAVE;
    const dim3 grid(unsigned((E + rows_per_block - 1) / rows_per_block), unsigned(A)), block(TPB);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (gauss) {
        const GaussianArgs g{a, *head};
        if (precision == BSX_ACTOR_BF16X6) hipLaunchKernelGGL(bsx_actor_gaussian_kernel<BSX_ACTOR_BF16X6>, grid, block, 0, s, g);
        else if (precision == BSX_ACTOR_BF16X3) hipLaunchKernelGGL(bsx_actor_gaussian_kernel<BSX_ACTOR_BF16X3>, grid, block, 0, s, g);
        else hipLaunchKernelGGL(bsx_actor_gaussian_kernel<BSX_ACTOR_F32>, grid, block, 0, s, g);
    } else {
        if (precision == BSX_ACTOR_BF16X6) hipLaunchKernelGGL(bsx_actor_kernel<BSX_ACTOR_BF16X6>, grid, block, 0, s, a);
        else if (precision == BSX_ACTOR_BF16X3) hipLaunchKernelGGL(bsx_actor_kernel<BSX_ACTOR_BF16X3>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(bsx_actor_kernel<BSX_ACTOR_F32>, grid, block, 0, s, a);
    }
    return int(hipGetLastError());
}

int bsx_actor_forward(const float* weights, const float* obs, float* scores, int64_t E, int n, int precision,
                      const BsxActorNoise* noise, uint64_t seed, uint64_t seq, const uint64_t* seq_base, int64_t env_offset,
                      void* stream) {
    return actor_forward(weights, obs, scores, E, n, precision, noise, false, nullptr, seed, seq, seq_base, env_offset, stream);
}

int bsx_actor_forward_gaussian(const float* weights, const float* obs, float* scores, int64_t E, int n, int precision,
                               const BsxActorNoise* noise, const BsxGaussianHead* head, uint64_t seed, uint64_t seq,
                               const uint64_t* seq_base, int64_t env_offset, void* stream) {
    return actor_forward(weights, obs, scores, E, n, precision, noise, true, head, seed, seq, seq_base, env_offset, stream);
}

// The float32 kernel without noise on any agent count and input width (the kernel reads A and D at run time); with `raw`, the value path
// on the same blob: head column 0 before tanh.
int bsx_mlp_forward(const float* weights, const float* x, float* y, float* raw, int64_t R, int A, int D, void* stream) {
    if (!x || !y) return BSX_E_ARG;
    if (!weights || !mlp_shape(R, A, D)) return BSX_E_ARG;
    if (!aligned(weights, 16) || !aligned(y, 16) || !aligned(x, 4) || !aligned(raw, 4)) return BSX_E_ALIGN;
    BsxActorNoise nz = {};
    if (raw) { nz.value_weights = weights; nz.value = raw; }
    const ActorArgs a{weights, x, y, R, A, D, nz, 0, 0, nullptr, 0};
    const int rows_per_block = (TPB / 64) * ROWS_PER_WAVE;
    const dim3 grid(unsigned((R + rows_per_block - 1) / rows_per_block), unsigned(A)), block(TPB);
    hipLaunchKernelGGL(bsx_actor_kernel<BSX_ACTOR_F32>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return int(hipGetLastError());
}

}  // extern "C"
