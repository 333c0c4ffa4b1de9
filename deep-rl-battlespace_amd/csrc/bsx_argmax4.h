// bsx_argmax4.h -- the discrete game's choice among four scores, stated ONCE: the step kernels (bsx_step_kernel.h and its split forms) play
// it, the DQN head (bsx_dqn_head.hip) learns from it.  namespace bsxk.
#pragma once

namespace bsxk {

// np.argmax over four scores (battle_env.py:327-328): the first maximum; a NaN compares as the maximum.  The running maximum is a
// register, not v[arg]: a dynamically indexed local array lives in scratch memory.
__device__ inline int argmax4(float a, float b, float c, float d) {
    int am = 0;
    float best = a;
    const float v[3] = {b, c, d};
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (!(best != best) && (v[i] > best || v[i] != v[i])) { am = i + 1; best = v[i]; }
    return am;
}

}  // namespace bsxk
