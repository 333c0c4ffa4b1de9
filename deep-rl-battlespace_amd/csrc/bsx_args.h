// bsx_args.h -- the argument check every C entry point that takes games starts with (bsx_kernels.hip, bsx_actor.hip).  Host code only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "battlespace_hip.h"

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// `p` -- the state block (256-byte aligned), or the first array of a call that takes none -- with the game count and the team size:
// BSX_E_ARG for a null `p` or a size out of range, then BSX_E_ALIGN for a `p` off its `align`-byte boundary; 0 = go on.  An entry point
// checks its other arguments for BSX_E_ARG before this and for BSX_E_ALIGN after it, which keeps the code a call that breaks several
// rules at once gets.
inline int check_games(const void* p, int64_t E, int n, size_t align = 256, int n_max = BSX_MAX_N) {
    if (!p || E <= 0 || E > BSX_MAX_E || n < 1 || n > n_max) return BSX_E_ARG;
    return aligned(p, align) ? 0 : BSX_E_ALIGN;
}

// the ranges of the bsx_mlp_* entry points: any agent count up to 2 * BSX_MAX_N (odd ones too) and any input width up to BSX_MLP_MAX_D
inline bool mlp_shape(int64_t R, int A, int D) {
    return R >= 1 && R <= BSX_MAX_E && A >= 1 && A <= 2 * BSX_MAX_N && D >= 1 && D <= BSX_MLP_MAX_D;
}
