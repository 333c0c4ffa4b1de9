// bsx_actor_body.inl -- the body of the stand-alone actor kernels (bsx_actor.hip includes it inside bsx_actor_kernel<PREC> and
// bsx_actor_gaussian_kernel<PREC>; it shares their locals, so this is a textual unit, not a function).  Names it expects: PREC, GAUSS
// (constexpr: finish the rows with the Gaussian policy head), p (ActorArgs), gh (BsxGaussianHead, read only when GAUSS).
// (A textual unit and not an inlined function: as a function taking the arguments by reference, the plain kernels' instruction
//  schedule moved.)
    const int D = p.D, Dp = dpad(D);
    const int a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, c = lane & 31;
    const float* __restrict__ W = p.weights + size_t(a) * blob_floats(D);

    // per-neuron vectors (6 x 64), head weights (256) and head bias (4): once per workgroup into LDS
    __shared__ __attribute__((aligned(16))) float s_small[SMALL];
    for (int i = tid; i < SMALL / 4; i += TPB)
        reinterpret_cast<float4*>(s_small)[i] = reinterpret_cast<const float4*>(W + off_small(D))[i];

    const int64_t row0 = (int64_t(blockIdx.x) * (TPB / 64) + wave) * ROWS_PER_WAVE;   // first env of this wave
    // the replay counter is a device word behind a kernel argument: requested here, with the first weight loads, not where the noise
    // needs it (the compiler's choice -- a scalar miss with nothing left to hide it at the end of the kernel)
    uint64_t seq_add = p.seq_base ? *p.seq_base : 0ull;
    float4 o[2];
    if constexpr (PREC != BSX_ACTOR_F32) {
        __syncthreads();
        o[0] = make_float4(0.f, 0.f, 0.f, 0.f); o[1] = o[0];
#pragma nounroll
        for (int nt = 0; nt < 2; ++nt) {                 // rolled: one tile's registers at a time
            const int64_t en = row0 + 32 * nt + c;
            const float* xr = p.obs + (size_t(en < p.E ? en : p.E - 1) * p.A + a) * D;
            const float* Wn = W;
            asm volatile("" : "+s"(Wn));                 // keeps the weight loads inside the loop (hoisted, they double the registers)
            const float4 t = tile_forward<PREC>(Wn, s_small, D, lane, [&](int k) { return k < D ? xr[k] : 0.f; });
            if (nt == 0) o[0] = t; else o[1] = t;
        }
    } else {
        __syncthreads();
        const float* sm = s_small + hh * 32;      // this lane half's [mo][v] slice of each 64-float vector ([hh][mo][v])

        // ---- layer 1: acc1[mo][nt] = b1 + W1^T * X^T
        f32x16 acc1[2][2];
    #pragma unroll
        for (int mo = 0; mo < 2; ++mo)
    #pragma unroll
            for (int v = 0; v < 16; ++v) { acc1[mo][0][v] = sm[0 * H + mo * 16 + v]; acc1[mo][1][v] = acc1[mo][0][v]; }
        const float* xrow[2];
    #pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t en = row0 + 32 * nt + c;
            xrow[nt] = p.obs + (size_t(en < p.E ? en : p.E - 1) * p.A + a) * D;
        }
        for (int s = 0; s < Dp / 2; ++s) {
            const int k = 2 * s + hh;
            const float a0 = W[(0 * (Dp / 2) + s) * 64 + lane], a1 = W[(1 * (Dp / 2) + s) * 64 + lane];
            const float b0 = k < D ? xrow[0][k] : 0.f, b1 = k < D ? xrow[1][k] : 0.f;
            acc1[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc1[0][0], 0, 0, 0);
            acc1[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc1[0][1], 0, 0, 0);
            acc1[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc1[1][0], 0, 0, 0);
            acc1[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc1[1][1], 0, 0, 0);
        }
        // the 64 x 64 layer's A operands: 64 VGPRs, coalesced 16-byte loads, issued behind layer 1's own loads (vmcnt is in-order), in flight under the LayerNorm
        float4 w2[2][2][4];
    #pragma unroll
        for (int mo = 0; mo < 2; ++mo)
    #pragma unroll
            for (int mt = 0; mt < 2; ++mt)
    #pragma unroll
                for (int vq = 0; vq < 4; ++vq)
                    w2[mo][mt][vq] = reinterpret_cast<const float4*>(W + off_w2(D))[((mo * 2 + mt) * 4 + vq) * 64 + lane];

        asm volatile("" : "+s"(seq_add));                // (waited for here, under the 64 x 64 layer's weight loads)
        ln_relu_tile(acc1[0][0], acc1[1][0], sm + 1 * H, sm + 2 * H);
        ln_relu_tile(acc1[0][1], acc1[1][1], sm + 1 * H, sm + 2 * H);

        // ---- layer 2: acc2[mo][nt] = b2 + W2^T * H1^T, the K index running over layer 1's accumulator registers
        f32x16 acc2[2][2];
    #pragma unroll
        for (int mo = 0; mo < 2; ++mo)
    #pragma unroll
            for (int v = 0; v < 16; ++v) { acc2[mo][0][v] = sm[3 * H + mo * 16 + v]; acc2[mo][1][v] = acc2[mo][0][v]; }
    #pragma unroll
        for (int mt = 0; mt < 2; ++mt)
    #pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float4 q0 = w2[0][mt][v >> 2], q1 = w2[1][mt][v >> 2];
                const float wa0 = (v & 3) == 0 ? q0.x : ((v & 3) == 1 ? q0.y : ((v & 3) == 2 ? q0.z : q0.w));
                const float wa1 = (v & 3) == 0 ? q1.x : ((v & 3) == 1 ? q1.y : ((v & 3) == 2 ? q1.z : q1.w));
                acc2[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa0, acc1[mt][0][v], acc2[0][0], 0, 0, 0);
                acc2[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa0, acc1[mt][1][v], acc2[0][1], 0, 0, 0);
                acc2[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa1, acc1[mt][0][v], acc2[1][0], 0, 0, 0);
                acc2[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa1, acc1[mt][1][v], acc2[1][1], 0, 0, 0);
            }
        ln_relu_tile(acc2[0][0], acc2[1][0], sm + 4 * H, sm + 5 * H);
        ln_relu_tile(acc2[0][1], acc2[1][1], sm + 4 * H, sm + 5 * H);

        // ---- head: 64 -> 4 on the vector pipe; each lane sums its 32 neurons, the partner lane l^32 has the other 32
        const float4* w3 = reinterpret_cast<const float4*>(s_small + 6 * H) + hh * 32;   // [hh][mt][v] float4
        o[0] = make_float4(0.f, 0.f, 0.f, 0.f); o[1] = o[0];
    #pragma unroll
        for (int mt = 0; mt < 2; ++mt)
    #pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float4 ww = w3[mt * 16 + v];
    #pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float hv = acc2[mt][nt][v];
                    o[nt].x = fmaf(hv, ww.x, o[nt].x); o[nt].y = fmaf(hv, ww.y, o[nt].y);
                    o[nt].z = fmaf(hv, ww.z, o[nt].z); o[nt].w = fmaf(hv, ww.w, o[nt].w);
                }
            }
    #pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            o[nt].x += __shfl_xor(o[nt].x, 32); o[nt].y += __shfl_xor(o[nt].y, 32);
            o[nt].z += __shfl_xor(o[nt].z, 32); o[nt].w += __shfl_xor(o[nt].w, 32);
        }
}
    // lower half finishes the rows of tile 0, upper half those of tile 1: every lane writes one row
    float4 r4 = hh ? o[1] : o[0];
    const float4 b3 = *reinterpret_cast<const float4*>(s_small + 6 * H + H * NA);
    const int64_t e = row0 + 32 * hh + c;
    const size_t row = size_t(e < p.E ? e : p.E - 1) * p.A + a;
    const uint64_t seq = p.seq + seq_add;                // seq_base: device word, so graph replays re-key
    const bool game_over = p.nz.ou_scale > 0.f && p.nz.env_done && p.nz.env_done[e < p.E ? e : p.E - 1];
    if constexpr (GAUSS)
        r4 = finish_row<true>(r4, b3, p.nz, p.seed, seq, row, uint64_t(p.env_offset) * uint64_t(p.A) + row, false, e < p.E, row,
                              gh.log_std + 3 * a, gh.logp);
    else
        r4 = finish_row(r4, b3, p.nz, p.seed, seq, row, uint64_t(p.env_offset) * uint64_t(p.A) + row, game_over, e < p.E, row, nullptr, nullptr, a);
    if (e < p.E) reinterpret_cast<float4*>(p.scores)[row] = r4;
    if (p.nz.value_weights) {
        // ---- the value head: a second MLP of the same shape on the same rows, in the same precision mode (per-tile code of
        //      bsx_actor_core.h, which the fused rollout runs as well: same bits), one 32-row tile at a time; its
        //      per-neuron vectors and head take the place of the actor's in LDS (every lane is done with them)
        const float* __restrict__ Wv = p.nz.value_weights + size_t(a) * blob_floats(D);
        __syncthreads();
        for (int i = tid; i < SMALL / 4; i += TPB)
            reinterpret_cast<float4*>(s_small)[i] = reinterpret_cast<const float4*>(Wv + off_small(D))[i];
        __syncthreads();
        float4 v[2];
#pragma nounroll
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t en = row0 + 32 * nt + c;
            const float* xr = p.obs + (size_t(en < p.E ? en : p.E - 1) * p.A + a) * D;
            const float* Wn = Wv;
            asm volatile("" : "+s"(Wn));
            const float4 t = tile_forward<PREC>(Wn, s_small, D, lane, [&](int k) { return k < D ? xr[k] : 0.f; });
            if (nt == 0) v[0] = t; else v[1] = t;
        }
        const float vh = hh ? v[1].x : v[0].x;
        if (e < p.E) p.nz.value[row] = vh + s_small[6 * H + H * NA];
    }
