// bsx_explore.hip -- the annealing schedule of the epsilon-greedy behaviour policy (BsxActorNoise.epsilon, bsx_actor_core.h), on device:
// one small launch that advances a device counter and rewrites the per-plane exploration rates, so that a captured rollout graph anneals
// from replay to replay with no host work.  binary64, every operation rounded on its own (built with -ffp-contract=off), one rounding to
// float32 at the end: the linear kind is restated bit for bit by tests/epsilon_util.py, the exponential kind is held to numpy's exp.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_args.h"

namespace {

constexpr int TPB = 64;

struct EpsArgs { float* epsilon; int A; int64_t* count; int64_t by; double start, end; int64_t steps; int kind; };

// One workgroup: every lane reads the old count, lane 0 stores the new one behind the barrier, the lanes share the A entries.
__global__ __launch_bounds__(TPB) void bsx_epsilon_advance_kernel(const EpsArgs p) {
    const int64_t c = *p.count + p.by;
    __syncthreads();
    if (threadIdx.x == 0) *p.count = c;
    const double x = double(c) / double(p.steps);
    const double f = p.kind == BSX_EPS_LINEAR ? fmax(0.0, 1.0 - x) : exp(-x);
    const float eps = float(p.end + (p.start - p.end) * f);
    for (int i = threadIdx.x; i < p.A; i += TPB) p.epsilon[i] = eps;
}

}  // namespace

extern "C" int bsx_epsilon_advance(float* epsilon, int A, int64_t* count, int64_t by, double start, double end, int64_t steps, int kind,
                                   void* stream) {
    if (!epsilon || !count || A < 1 || steps < 1 || (kind != BSX_EPS_LINEAR && kind != BSX_EPS_EXP)) return BSX_E_ARG;
    if (!(start >= 0.0 && start <= 1.0) || !(end >= 0.0 && end <= 1.0)) return BSX_E_ARG;
    if (!aligned(epsilon, 4) || !aligned(count, 8)) return BSX_E_ALIGN;
    const EpsArgs a{epsilon, A, count, by, start, end, steps, kind};
    hipLaunchKernelGGL(bsx_epsilon_advance_kernel, dim3(1), dim3(TPB), 0, static_cast<hipStream_t>(stream), a);
    return int(hipGetLastError());
}
