// bsx_ppo_central.hip -- the input rows of a centralised PPO critic (MAPPO) from a rollout's observation records
// (include/battlespace_hip.h: bsx_ppo_joint_obs), gfx950.
//
// Row (r, i) of x is plane i's agent-specific joint observation: its own observation first, then its team-mates' in ascending plane
// index.  Pure bandwidth: R A Do floats in, n times that out, bits copied and never converted (no -ffp-contract concern).
// One record row r owns W = A n Do contiguous floats of x, cut into P = W / VEC vectors of VEC floats.  A thread owns ONE vector
// position p of the row -- its VEC source offsets inside obs[r] are worked out once, the only divisions of the kernel -- and RP =
// TPB / P rows are written per pass: thread (rr, p) = (tid / P, tid % P) writes vector rr P + p of the pass, so consecutive lanes store
// consecutive vectors and a wave's stores are one contiguous stretch of x.  A workgroup owns S = RP * passes consecutive rows: their
// obs floats are read once, coalesced, into LDS, and every float of x is then an LDS read at a precomputed offset.
// VEC is 4 where W is a multiple of 4 (n = 2, n = 4, and even Do) and x sits on a 16-byte boundary, else 2 (W is always even) on an
// 8-byte boundary, else 1 in workgroups of 512 threads (W <= 512: a thread still owns one position).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"

namespace {

constexpr int LDS_WORDS = 4096;                 // the staged obs rows of a workgroup: 16 KB
constexpr int MAX_PASSES = 8;
constexpr int JOINT_MAX_N = 4;

struct JoinArgs {
    const uint32_t* obs; uint32_t* x; int64_t R;
    int n, Do, AD, W;                           // AD = A Do words per obs row, W = A n Do words per x row
    int P, RP, S;                               // vectors per x row, rows per pass, rows per workgroup
};

template <int VEC> struct Words;
template <> struct Words<1> { typedef uint32_t type; };
template <> struct Words<2> { typedef uint2 type; };
template <> struct Words<4> { typedef uint4 type; };

// Word o of an x row -> the word of the obs row it copies.  o = (i, s, c): plane i = team n + k, slot s, column c; slot 0 is plane i
// itself, slot s >= 1 the s-th other plane of the team's n adjacent columns in ascending order.
__device__ inline int source_word(int o, int n, int Do) {
    const int nd = n * Do;
    const int i = o / nd, rem = o - i * nd;
    const int s = rem / Do, c = rem - s * Do;
    const int team = i / n, k = i - team * n;
    const int m = s == 0 ? k : (s <= k ? s - 1 : s);
    return (team * n + m) * Do + c;
}

template <int VEC, int TPB>
__global__ __launch_bounds__(TPB) void bsx_ppo_joint_obs_kernel(const JoinArgs a) {
    __shared__ uint32_t s_obs[LDS_WORDS];
    typedef typename Words<VEC>::type V;
    const int tid = threadIdx.x;
    const int64_t r0 = int64_t(blockIdx.x) * a.S;
    const int rows = int(a.R - r0 < a.S ? a.R - r0 : int64_t(a.S));
    const uint32_t* __restrict__ src = a.obs + r0 * a.AD;
    for (int j = tid; j < rows * a.AD; j += TPB) s_obs[j] = src[j];
    const int rr = tid / a.P, p = tid - rr * a.P;
    int off[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) off[k] = source_word(p * VEC + k, a.n, a.Do);
    __syncthreads();
    if (rr >= a.RP) return;
    for (int row = rr; row < rows; row += a.RP) {
        const uint32_t* s = s_obs + row * a.AD;
        uint32_t w[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) w[k] = s[off[k]];
        V* dst = reinterpret_cast<V*>(a.x + (r0 + row) * a.W + p * VEC);
        if constexpr (VEC == 4) *dst = make_uint4(w[0], w[1], w[2], w[3]);
        else if constexpr (VEC == 2) *dst = make_uint2(w[0], w[1]);
        else *dst = w[0];
    }
}

template <int VEC, int TPB>
int launch(JoinArgs a, hipStream_t stream) {
    a.P = a.W / VEC;
    a.RP = TPB / a.P;
    const int passes = LDS_WORDS / (a.RP * a.AD) < MAX_PASSES ? LDS_WORDS / (a.RP * a.AD) : MAX_PASSES;     // >= 1: RP AD <= TPB VEC / n <= 1024
    a.S = a.RP * passes;
    hipLaunchKernelGGL((bsx_ppo_joint_obs_kernel<VEC, TPB>), dim3(unsigned((a.R + a.S - 1) / a.S)), dim3(TPB), 0, stream, a);
    return int(hipGetLastError());
}

}  // namespace

extern "C" {

int bsx_ppo_joint_obs(const float* obs, int64_t R, int A, int Do, float* x, void* stream) {
    if (!obs || !x) return BSX_E_ARG;
    if (R < 0 || R > BSX_MAX_E || A < 2 || A % 2 || A / 2 > JOINT_MAX_N || Do < 1 || (A / 2) * Do > BSX_MLP_MAX_D) return BSX_E_ARG;
    if (!aligned(obs, 4) || !aligned(x, 4)) return BSX_E_ALIGN;
    if (R == 0) return 0;
    const int n = A / 2;
    JoinArgs a{reinterpret_cast<const uint32_t*>(obs), reinterpret_cast<uint32_t*>(x), R, n, Do, A * Do, A * n * Do, 0, 0, 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.W % 4 == 0 && aligned(x, 16)) return launch<4, 256>(a, s);
    if (aligned(x, 8)) return launch<2, 256>(a, s);
    return launch<1, 512>(a, s);
}

}  // extern "C"
