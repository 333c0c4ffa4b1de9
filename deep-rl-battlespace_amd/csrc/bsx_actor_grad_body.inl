// bsx_actor_grad_body.inl -- the body of the training-pass kernels (bsx_actor_grad.hip includes it inside bsx_actor_grad_kernel<MT1> and
// bsx_mlp_grad_kernel<MT1>; it shares their locals, so this is a textual unit, not a function, as bsx_actor_body.inl is for the forward).
// Names it expects: MT1, DX (constexpr: also write the input gradient), p (GradArgs), gx (float*, [R][A][D]; read only when DX).
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
        if constexpr (DX) {
            // ---- dx^T = W1 da1^T: the da1 registers are the B operand as they stand; A = W1[k = 32 m + c][j = nid(mt, v, hh)], the four
            //      j of a register quad as one 16-byte load from the blob's W1A section (bsx_actor_grad.hip's header says why from there).
            //      A lane whose k is beyond the section's Dp rows reads row Dp - 1 instead: its products are never stored
#pragma unroll
            for (int m = 0; m < MT1; ++m) {
                // (the lane's indices derived again and made opaque, as at the end of the kernel: the address is loop-invariant and would
                //  otherwise be kept in registers across the whole round loop)
                const int dl = here(int(threadIdx.x)) & 63, kr = 32 * m + (dl & 31), kk = kr < Dp ? kr : Dp - 1;
                const float4* wa = reinterpret_cast<const float4*>(W + ((kk >> 1) * 64 + (kk & 1) * 32 + 4 * (dl >> 5)));
                f32x16 dx;
#pragma unroll
                for (int v = 0; v < 16; ++v) dx[v] = 0.f;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int vq = 0; vq < 4; ++vq) {
                        const float4 q = wa[mt * (Dp / 2) * 16 + 2 * vq];
                        dx = __builtin_amdgcn_mfma_f32_32x32x2f32(q.x, mt == 0 ? t0[4 * vq + 0] : t1[4 * vq + 0], dx, 0, 0, 0);
                        dx = __builtin_amdgcn_mfma_f32_32x32x2f32(q.y, mt == 0 ? t0[4 * vq + 1] : t1[4 * vq + 1], dx, 0, 0, 0);
                        dx = __builtin_amdgcn_mfma_f32_32x32x2f32(q.z, mt == 0 ? t0[4 * vq + 2] : t1[4 * vq + 2], dx, 0, 0, 0);
                        dx = __builtin_amdgcn_mfma_f32_32x32x2f32(q.w, mt == 0 ? t0[4 * vq + 3] : t1[4 * vq + 3], dx, 0, 0, 0);
                    }
                // lane (c, hh) holds dx[row c][k = nid(m, v, hh)]: rows beyond R and columns beyond D are not written
                if (valid) {
                    int Dl = D;                                   // (opaque: sixteen loop-invariant k < D lane masks would be kept in scalar
                    asm volatile("" : "+s"(Dl));                  //  registers across the round loop)
                    int64_t xo = xr - p.obs;                      // this row of grad_x: x's own offset (opaque here: formed at the top
                    asm volatile("" : "+v"(xo));                  //  of the round, the address would be live across all of it)
                    float* gr = gx + xo;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int k = nid(m, v, hh);
                        if (k < Dl) gr[k] = dx[v];
                    }
                }
            }
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
