// bsx_step_lds.inl -- the LDS layout of the step kernels (bsx_step_kernel.h and bsx_step_split.h include it in the kernel body): the arrays, this
// wave's pointers into them, the bullet pass's rectangle form (make_rect / hits_rect) and the owner-flag and overlap-field constants.  Sized by
// the includer's WAVES, N, ACTOR and CONT, and by the two-wave kernel's form: MANY (0 per call, 1 / 2 multi-tick; -1 in the one-wave kernel)
// and DRAW.  Arrays a kernel never touches are dropped by the compiler.
// LDS is private to this wavefront: accesses are volatile (program order) and the hardware runs one wave's LDS
// operations in order, so cross-lane hand-offs need no s_barrier -- only a compiler scheduling fence.
    constexpr int NE = (N > 0) ? N : 1;                  // compile-time enemy count (runtime-n build reads LDS in loops)
    constexpr int DROW = (N > 0) ? 3 * N + 2 : 3 * BSX_MAX_N + 2;
    __shared__ volatile int s_x_all[WAVES * SPB], s_y_all[WAVES * SPB], s_hp_all[WAVES * SPB];
    __shared__ volatile int s_bhit_all[WAVES * SPB];     // base hits, index gl + shooter team
    __shared__ __attribute__((aligned(16))) float s_obs_all[WAVES * SPB * DROW];   // observation rows, [wave][lane][D]
    __shared__ __attribute__((aligned(16))) float s_small[ACTOR ? (N == 1 ? 4 : 2 * N) * bsx_actor::SMALL : 4];   // per-neuron vectors + heads of the actors (1v1: + the two value heads')
    __shared__ int s_act_all[(ACTOR && !CONT && WAVES > 1) ? WAVES * SPB : 1];       // arg-max per row, ACTOR with several waves
    __shared__ float s_actf_all[(ACTOR && CONT && WAVES > 1) ? WAVES * SPB * 3 : 1];  // continuous: [speed, turn, shoot] per row
    __shared__ double s_actd_all[(ACTOR && CONT && WAVES > 1) ? WAVES * SPB * 3 : 1]; // ... of a scripted team's rows, binary64
    __shared__ int s_gdone_all[(ACTOR && WAVES > 1) ? 32 : 1];                       // game-over flag per game of the workgroup
    // n >= 2: every plane-to-plane pair is computed ONCE, by one of its two planes, and handed to the other through these
    __shared__ float s_pd_all[(N >= 2) ? WAVES * SPB * N : 1];      // range (symmetric)
    __shared__ double s_pr_all[(N >= 2) ? WAVES * SPB * N : 1];     // the owner's bearing in radians, [0, 2 pi)
    // wave-packed bullet pass: the wave's pool entries (and this call's shots behind them) are WORK SLOTS, one per lane and round
    __shared__ __attribute__((aligned(8))) u32x2 s_new_all[WAVES * SPB];   // this call's shots as pool entries (age 0, the PRE-move pose), by shot rank
    __shared__ uint32_t s_agg_all[WAVES * SPB];          // per owner: misses << 16 | base hits << 24
    // The rectangles a bullet is tested against (enemy base, enemy planes' sprites), staged per owner / per plane for the work slots.
    // 1v1: as (lower corner, upper corner) pairs of packed (x, y) halves BIASED by +64, so that no half is ever negative and the
    // corners are plain 32-bit adds of packed literals: a bullet at b overlaps <=> no half of (b - lower) | (upper - b) is negative
    // (C2 7.33 -> 7.20 us against the centre form: ~15 instructions fewer per round where the instruction count is the bound).
    // 4v4 and the runtime-n kernel: the centre (x | alive << 15 | y << 16) and the margins as constants in the slot -- measured faster there
    // (round 3: 4v4 23.1 us against 24.7 with corners; round 4, with the table shot: 20.5 against 20.8).  2v2 / 3v3 take the corner form
    // since round 4 (with the table shot 10.22 -> 9.67 and 17.97 -> 17.05 us; profiles/r04_experiments.json).
    constexpr bool CORNERS = N >= 1 && N <= 3;
    typedef typename std::conditional<CORNERS, u32x2, uint32_t>::type rect_t;
    __shared__ __attribute__((aligned(8))) rect_t s_eb_all[WAVES * SPB];        // per owner: the enemy base, dx in [-33, 33], dy in [-32, 31]
    __shared__ __attribute__((aligned(8))) rect_t s_pq_all[WAVES * SPB];        // per plane: its post-move sprite, dx in [-27, 27], dy in [-25, 24]; dead: never hit
    // rect(centre, alive, margins below / above): what the owner side stages
    auto make_rect = [](uint32_t c, bool alive, int xl, int yl, int xh, int yh) {
        if constexpr (CORNERS) return alive ? u32x2{c + pk_const(PK_BIAS - xl, PK_BIAS - yl), c + pk_const(PK_BIAS + xh, PK_BIAS + yh)} : u32x2{0x7F007F00u, 0u};
        else return c | (alive ? 0x8000u : 0u);
    };
    // 0 / -1: does the bullet at b (CORNERS: biased) overlap the rectangle?  (r is a generic rect_t: the form not taken is then never compiled,
    // also where CORNERS does not depend on a template parameter)
    auto hits_rect = [](s16x2 b, auto r, int xl, int yl, int xh, int yh) {
        if constexpr (CORNERS) return ~pk_any_negative(pk_bits(b - as_pk(r.x)) | pk_bits(as_pk(r.y) - b));
        else {
            const s16x2 d = b - as_pk(r & ENT_XY);
            return ~pk_any_negative(pk_bits(d + as_pk(pk_const(xl, yl))) | pk_bits(as_pk(pk_const(xh, yh)) - d)) & (int(r << 16) >> 31);
        }
    };
    // per owner: what a work slot must know about its bullet's owner: the owner's tick % 12 (the exact-path ring) | 16: the owner's game
    // is in its physics call (its bullets fly) | 32: the game is being re-spawned by this call (its bullets are dropped)
    constexpr uint32_t OWN_PHYS = 16u, OWN_DROP = 32u;
    __shared__ uint32_t s_fl_all[WAVES * SPB];
    __shared__ __attribute__((aligned(16))) double s_nd_all[WAVES * SPB * 2];   // per owner: this call's shot's float64 step (written and read on the exact path only)
    // plane-overlap candidates per owner, by AGE (rare): FW bits per age (which enemy planes the bullet of that age overlaps), and where
    // that bullet's entry now sits in the pool (for the tombstone of a consumed bullet)
    constexpr int FW = (N > 0 && N <= 4) ? 4 : 16;       // bits per overlap field
    constexpr int OW = (FW == 4) ? 1 : 3;                // 64-bit words holding the 12 fields
    __shared__ unsigned long long s_ov_all[WAVES * SPB * OW];
    __shared__ uint16_t s_pp_all[WAVES * SPB * K];
    // the two-wave kernel's hand-offs between its waves (bsx_step_split.h; one element where the kernel's form never touches them)
    __shared__ uint32_t s_npl_all[MANY == 1 ? 2 * SPB : 1];                            // MANY = 1: the bullets' counts per shooter (misses | base hits << 8 | plane hits << 16), by tick parity
    __shared__ __attribute__((aligned(16))) v4u_t s_t0_all[MANY == 0 ? SPB : 1];      // per call: the post-move poses (position, heading, enemy base), wave 0 -> geometry wave
    __shared__ __attribute__((aligned(16))) v4f_t s_gm_all[MANY == 0 ? SPB : 1];      // per call: the four observation values, geometry wave -> storing wave
    __shared__ __attribute__((aligned(16))) v4u_t s_pub_all[MANY == 2 ? 2 * SPB : 1]; // MANY = 2: what a tick's outputs need, game wave -> outputs wave, by tick parity
    __shared__ __attribute__((aligned(16))) v4u_t s_rw_all[DRAW ? SPB : 1];           // per call, DRAW: the call's Philox block per lane (jitter or re-spawn), geometry wave -> first wave
    auto* const s_new = BSX_LDS(u32x2, s_new_all) + wave * SPB;
    auto* const s_agg = BSX_LDS(uint32_t, s_agg_all) + wave * SPB;
    auto* const s_eb = BSX_LDS(rect_t, s_eb_all) + wave * SPB;
    auto* const s_pq = BSX_LDS(rect_t, s_pq_all) + wave * SPB;
    auto* const s_fl = BSX_LDS(uint32_t, s_fl_all) + wave * SPB;
    auto* const s_nd = BSX_LDS(double, s_nd_all) + wave * SPB * 2;
    auto* const s_ov = BSX_LDS(unsigned long long, s_ov_all) + wave * SPB * OW;
    auto* const s_pp = BSX_LDS(uint16_t, s_pp_all) + wave * SPB * K;
    if constexpr (MANY < 0) {                            // (the two-wave kernel clears them in the role branch of the wave that runs the bullets)
#pragma unroll
        for (int q = 0; q < OW; ++q) s_ov[tid * OW + q] = 0ull;   // cleared again by whoever finds them set
    }
    float* const s_pd = s_pd_all + ((N >= 2) ? wave * SPB * N : 0);
    double* const s_pr = s_pr_all + ((N >= 2) ? wave * SPB * N : 0);
    // (explicit LDS address space: a volatile access through a generic pointer compiles to flat_load / flat_store)
    typedef __attribute__((address_space(3))) volatile int lds_vint;
    lds_vint* const s_x = (lds_vint*)(uintptr_t)(s_x_all) + wave * SPB;
    lds_vint* const s_y = (lds_vint*)(uintptr_t)(s_y_all) + wave * SPB;
    lds_vint* const s_hp = (lds_vint*)(uintptr_t)(s_hp_all) + wave * SPB;
    lds_vint* const s_bhit = (lds_vint*)(uintptr_t)(s_bhit_all) + wave * SPB;
    float* const s_obs = s_obs_all + wave * SPB * DROW;
    auto* const s_npl = BSX_LDS(uint32_t, s_npl_all);
    auto* const s_t0 = (__attribute__((address_space(3))) volatile v4u_t*)(uintptr_t)(s_t0_all);
    auto* const s_gm = (__attribute__((address_space(3))) volatile v4f_t*)(uintptr_t)(s_gm_all);
    auto* const s_pub = (__attribute__((address_space(3))) volatile v4u_t*)(uintptr_t)(s_pub_all);
    auto* const s_rw = (__attribute__((address_space(3))) volatile v4u_t*)(uintptr_t)(s_rw_all);
