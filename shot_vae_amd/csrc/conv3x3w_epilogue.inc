// Epilogue of the wide 3x3 convolution kernels (conv3x3w.hip, conv3x3x.hip), included INSIDE the kernel body after the K
// loop.  In scope: smem, ssum, tid, lane, wave, r, h, n0, gr0, g, a, acc[2][NF] (32x32 accumulator tiles: pixel half f,
// 32-channel group i), the constants BN, NF, W and a configuration type C with SCR, OFF_SSUM.  EPD = groups of residual
// rows in flight.
    // ---- epilogue: per 32-channel group through a wave-private LDS transpose ------------------------------------------
    // (every wave is past the last barrier: the halo and weight buffers are free)
    // SV_EPI_NSCR scratch sets per wave (1 or 2): with two, consecutive groups use different LDS.  SV_EPI_BASE = byte offset
    // of the scratch in LDS (0: over the dead halo / weight buffers; a persistent kernel keeps it apart).  SV_EPI_ALIAS:
    // the per-wave reduction buffer lies over the (by then consumed) transpose scratch of the same wave.
    constexpr int NSCR = SV_EPI_NSCR, EBASE = SV_EPI_BASE;
    constexpr bool EALIAS = SV_EPI_ALIAS != 0;
    constexpr int ERED = EALIAS ? 0 : 4 * NSCR * 4096;
    float* const scr0 = reinterpret_cast<float*>(smem + EBASE + wave * NSCR * C::SCR);                 // [64 pixels][36]
    float* const red0 = EALIAS ? scr0 : reinterpret_cast<float*>(smem + EBASE + 4 * NSCR * C::SCR + wave * NSCR * 4096);
    static_assert(EBASE + 4 * NSCR * C::SCR + ERED <= C::OFF_SSUM, "epilogue scratch");
    bf16* const O = reinterpret_cast<bf16*>(a.out);
    // SV_EPI_MODE (compile time): 0 = the fusion flags are read from the arguments (one binary for every call);
    // 1 = statistics only, 2 = residual + statistics, 3 = activation-backward (ex) -- no bias in 1..3.  With the flags known
    // the group loop is straight-line code: its LDS reads are batched instead of one exposed round trip per basic block.
    constexpr int EMODE = SV_EPI_MODE;
    const bf16* const R_ = reinterpret_cast<const bf16*>(a.residual);
    const bf16* const EX_ = reinterpret_cast<const bf16*>(a.ex);
    const bool has_R = EMODE == 0 ? R_ != nullptr : EMODE == 2;
    const bool has_EX = EMODE == 0 ? EX_ != nullptr : EMODE == 3;
    const bf16* const R = has_R ? R_ : nullptr;
    const bf16* const EX = has_EX ? EX_ : nullptr;
    const bool want_stats = EMODE == 0 ? (a.stats != nullptr && !has_EX) : (EMODE == 1 || EMODE == 2);
    const bool has_bias = EMODE == 0 ? a.bias != nullptr : false;
    // (read ONCE: `a` lives in the kernel-argument segment and the K loops' inline assembly clobbers memory, so every use of
    //  a.ex_slope was a scalar load -- and `cond ? v : v * a.ex_slope` a branch per element around that load + its wait:
    //  64 exposed round trips per 32-channel group of the data gradient)
    const float ex_slope = has_EX ? a.ex_slope : 1.f;
    const int ipix = lane >> 2, cg = lane & 3;
    const int64_t gp0 = (int64_t)gr0 * W + 64 * wave;
    // residual / raw-tensor operand of the epilogue: the rows of group i+1 are requested while group i is processed
    // (one exposed HBM round trip per block instead of one per 32-channel group)
    // per-channel constants of the block's channels: one cooperative copy into LDS instead of a dependent global
    // round trip per 32-channel group
    float* const cst = reinterpret_cast<float*>(smem + EBASE + 4 * NSCR * C::SCR + ERED);      // [5][BN]
    static_assert(EBASE + 4 * NSCR * C::SCR + ERED + 5 * BN * 4 <= C::OFF_SSUM, "epilogue scratch (halo, weight and coefficient buffers are free after the loop)");
    if (has_bias || has_EX) {
        for (int c = tid; c < BN; c += 256) {
            if (has_bias) cst[c] = a.bias[n0 + c];
            if (has_EX) {
                const float rs = a.ex_rstd[n0 + c];
                cst[BN + c] = a.ex_scale[n0 + c];
                cst[2 * BN + c] = a.ex_shift[n0 + c];
                cst[3 * BN + c] = -a.ex_mean[n0 + c] * rs;                         // xhat = x * rstd - mean * rstd
                cst[4 * BN + c] = rs;
            }
        }
        __syncthreads();
    }
    const bf16* const esrc = has_R ? R_ : EX_;
    const bool has_esrc = has_R || has_EX;
    // EPD groups of residual / raw-tensor rows in flight: one group of work (~1.2 k cycles) does not cover an HBM round trip
    constexpr int EPD = SV_EPD;
    bf16x8 eopn[EPD][4];
    if (has_esrc) {
#pragma unroll
        for (int d = 0; d < EPD; ++d)
            if (d < NF) {
#pragma unroll
                for (int it = 0; it < 4; ++it)
                    eopn[d][it] = *reinterpret_cast<const bf16x8*>(esrc + (gp0 + 16 * it + ipix) * g.ldo + n0 + 8 * cg + 32 * d);
            }
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const int nl = 32 * i + 8 * cg, n = n0 + nl;
        float* const scr = scr0 + (i % NSCR) * (C::SCR / 4);
        float* const red = red0 + (i % NSCR) * 1024;
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f32x4 v = {acc[f][i][4 * gq], acc[f][i][4 * gq + 1], acc[f][i][4 * gq + 2], acc[f][i][4 * gq + 3]};
                *reinterpret_cast<f32x4*>(scr + (32 * f + r) * 36 + 8 * gq + 4 * h) = v;
            }
        float bias[8], esc[8], esh[8], ers[8], emr[8];
        auto load8 = [&](const float* p, float (&d)[8]) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(p + nl), hi = *reinterpret_cast<const f32x4*>(p + nl + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { d[e] = lo[e]; d[e + 4] = hi[e]; }
        };
        if (has_bias) load8(cst, bias);
        if (has_EX) {
            load8(cst + BN, esc);
            load8(cst + 2 * BN, esh);
            load8(cst + 3 * BN, emr);
            load8(cst + 4 * BN, ers);
        }
        float s1[8], s2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
        bf16x8 eop[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) eop[it] = eopn[i % EPD][it];
        if (has_esrc && i + EPD < NF) {
#pragma unroll
            for (int it = 0; it < 4; ++it)
                eopn[i % EPD][it] = *reinterpret_cast<const bf16x8*>(esrc + (gp0 + 16 * it + ipix) * g.ldo + n + 32 * EPD);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int pix = 16 * it + ipix;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(scr + pix * 36 + 8 * cg);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(scr + pix * 36 + 8 * cg + 4);
            float vv[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vv[e] = v0[e];
                vv[e + 4] = v1[e];
            }
            if (has_bias) {
#pragma unroll
                for (int e = 0; e < 8; ++e) vv[e] += bias[e];
            }
            if (has_R) {
#pragma unroll
                for (int e = 0; e < 8; ++e) vv[e] += (float)eop[it][e];
            }
            if (has_EX) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xf = (float)eop[it][e];
                    const float gv = vv[e] * ((xf * esc[e] + esh[e] > 0.f) ? 1.f : ex_slope);
                    vv[e] = gv;
                    s1[e] += gv;
                    s2[e] += gv * (xf * ers[e] + emr[e]);
                }
            } else if (want_stats) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    s1[e] += vv[e];
                    s2[e] += vv[e] * vv[e];
                }
            }
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)vv[e];
            *reinterpret_cast<bf16x8*>(O + (gp0 + pix) * g.ldo + n) = o;
        }
        // (compiler fence: the reduction buffer below may lie over this wave's transpose scratch -- SV_EPI_ALIAS -- and is
        //  accessed through float lvalues while the scratch is accessed through f32x4: nothing of the read-back above may
        //  move below, nothing of the reduction above the next group's dump)
        asm volatile("" ::: "memory");
        if (want_stats || has_EX) {
            // 16 partial sums per lane, 16 lanes (pixel rows) per channel group cg = lane & 3.  First across the four lanes of a DPP row
            // that share cg (two row_shr steps: lanes 12..15 of a row then hold the row's sums), only those lanes go through LDS:
            // a quarter of the scratch traffic of an all-through-LDS form and 4 instead of 16 dependent reads per lane
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s1[e] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s1[e]), 0x114, 0xf, 0xf, true));
                s2[e] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s2[e]), 0x114, 0xf, 0xf, true));
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s1[e] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s1[e]), 0x118, 0xf, 0xf, true));
                s2[e] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s2[e]), 0x118, 0xf, 0xf, true));
            }
            if ((lane & 12) == 12) {
                float* mine = red + (cg * 4 + (lane >> 4)) * 16;
#pragma unroll
                for (int q4 = 0; q4 < 2; ++q4) {
                    *reinterpret_cast<f32x4*>(mine + 4 * q4) = f32x4{s1[4 * q4], s1[4 * q4 + 1], s1[4 * q4 + 2], s1[4 * q4 + 3]};
                    *reinterpret_cast<f32x4*>(mine + 8 + 4 * q4) = f32x4{s2[4 * q4], s2[4 * q4 + 1], s2[4 * q4 + 2], s2[4 * q4 + 3]};
                }
            }
            const float* col = red + (lane >> 4) * 64 + (lane & 15);
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) t += col[16 * q];
            const int e2 = lane & 15;
            // SV_EPI_WAVE_SUMS: every wave owns a copy of the sums (each address is written once per item and wave: a plain
            // store, nothing to clear, no LDS float atomics); otherwise the four waves meet in one copy
            if (SV_EPI_WAVE_SUMS) ssum[wave * 2 * BN + (e2 >> 3) * BN + 32 * i + 8 * (lane >> 4) + (e2 & 7)] = t;
            else atomicAdd(&ssum[(e2 >> 3) * BN + 32 * i + 8 * (lane >> 4) + (e2 & 7)], t);
        }
        asm volatile("" ::: "memory");
    }
    if (want_stats || has_EX) {
        __syncthreads();
        double* dst = (has_EX ? a.bsums : a.stats) + (size_t)(blockIdx.x & (a.replicas - 1)) * 2 * g.N;
        for (int i = tid; i < 2 * BN; i += 256) {
            const int which = i / BN, nl = i - which * BN;
            float v = ssum[i];
            if (SV_EPI_WAVE_SUMS) v += ssum[2 * BN + i] + ssum[4 * BN + i] + ssum[6 * BN + i];
            atomicAdd(dst + which * g.N + n0 + nl, (double)v);
        }
    }
