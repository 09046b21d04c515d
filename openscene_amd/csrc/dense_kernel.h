// The text of the 1x1-convolution kernel (dense.hip includes it once per kernel template: the three-piece kernel under the name and
// template parameters it always had, and the reduced-precision template with a leading piece count).  Not a header of its own: it needs
// the includes and constants of dense.hip and the three macros below.
//   OSN_DN_TEMPLATE  the template header     OSN_DN_NAME  the kernel's name     OSN_DN_NP  its piece count (a constant expression)
// NP (split.h): pieces per operand -- planes staged, fragment planes held (planes 0 .. NP - 1 of the one weight image), products kept.
OSN_DN_TEMPLATE
__global__ __launch_bounds__(256, 2) void OSN_DN_NAME(const float* __restrict__ in, const bf16x8* __restrict__ Wp,
                                                    float* __restrict__ out, int64_t n, int cin, int cout, int ns, int ncb,
                                                    int64_t per_plane /* 1 KB blocks per weight plane */, const Epi epi) {
    constexpr int NP = OSN_DN_NP;                   // pieces per operand (split.h)
    constexpr int NT = 256;
    constexpr int CK = 32 * KS;
    constexpr int LDA = CK + 8;                     // bf16 row stride of a staged plane (16-byte aligned rows)
    constexpr int QPR = CK / 4;                     // 4-channel quads per staged row
    constexpr int NQ = DN_BM * QPR / NT;            // quads per thread per chunk (2 KS)
    __shared__ __attribute__((aligned(16))) __bf16 stage[NP][DN_BM][LDA];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t r0 = int64_t(blockIdx.x) * DN_BM;
    const int ncg = (cout + 127) / 128;
    const bool single = ns <= KS;                   // the contraction is one chunk: the staged rows serve every column group

    int q_row[NQ], q_col[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int idx = tid + NT * j;
        q_row[j] = idx / QPR;
        q_col[j] = (idx % QPR) * 4;
    }
    float4 P[NQ];
    auto fetch = [&](int s0) {                      // unconditional, clamped addresses; masked at conversion time
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int64_t row = r0 + q_row[j] < n ? r0 + q_row[j] : n - 1;
            const int ch = 32 * s0 + q_col[j];
            P[j] = *reinterpret_cast<const float4*>(in + row * cin + (ch < cin ? ch : 0));
        }
    };
    auto stage_rows = [&](int s0) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const bool ok = 32 * s0 + q_col[j] < cin && r0 + q_row[j] < n;
            bf16x4 p[NP];
            tl_split4<NP>(ok ? P[j] : make_float4(0.f, 0.f, 0.f, 0.f), p);      // split.h: two elements per conversion
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<bf16x4*>(&stage[pl][q_row[j]][q_col[j]]) = p[pl];
        }
    };

    // column groups of this workgroup: all of them (single chunk), else the one blockIdx.y names
    const int cg_first = single ? 0 : int(blockIdx.y);
    const int cg_end = single ? ncg : int(blockIdx.y) + 1;
    fetch(0);
    for (int cg = cg_first; cg < cg_end; ++cg) {
        const int cb0 = cg * 8 + 2 * wave;          // this wave's first 16-column block
        f32x4 acc[4][2];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[rb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bool wave_on = cg * 128 + 32 * wave < cout;      // (a 96-column layer leaves the fourth wave staging only)
        for (int s0 = 0; s0 < ns; s0 += KS) {
            // ---- the chunk's weight fragments of this wave's columns: one coalesced 1 KB load each
            bf16x8 B[KS][2][NP];
            if (wave_on)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const bool on = s0 + ks < ns && cb0 + nb < ncb;
                    const int64_t blk = on ? int64_t(s0 + ks) * ncb + cb0 + nb : 0;
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) B[ks][nb][pl] = (Wp + ((pl * per_plane + blk) << 6))[lane];
                }
            if (!(single && cg > cg_first)) {       // (single chunk: the rows staged for the first column group stay)
                stage_rows(s0);
                if (s0 + KS < ns) fetch(s0 + KS);   // the next chunk's rows: in flight during the MFMAs below
                __syncthreads();
            }
            const int akq = 8 * (lane >> 4);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (wave_on && s0 + ks < ns) {
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) {
                        bf16x8 af[NP];
#pragma unroll
                        for (int pl = 0; pl < NP; ++pl)
                            af[pl] = *reinterpret_cast<const bf16x8*>(&stage[pl][16 * rb + (lane & 15)][ks * 32 + akq]);
                        split_products<NP>([&](auto ap, auto bp) {
#pragma unroll
                            for (int nb = 0; nb < 2; ++nb)
                                acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(B[ks][nb][bp], af[ap], acc[rb][nb], 0, 0, 0);
                        });
                    }
                }
            }
            if (!single && s0 + KS < ns) __syncthreads();   // every wave is done reading the stage before the next chunk lands
        }
        // ---- accumulators -> output rows.  The weight fragment is the MFMA's FIRST operand (the staged rows the second), so a
        // block comes out transposed: lane l holds columns 4 (l >> 4) .. + 3 of row l & 15 -- one 16-byte store per block
        if (wave_on) {
            EpiCols ec[2];
            if constexpr (EPI) {                 // the lane's two column quads: constants once for the four row blocks
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const int col = cg * 128 + 32 * wave + 16 * nb + 4 * (lane >> 4);
                    ec[nb] = epi_cols(epi, col < cout ? col : 0);
                }
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const int64_t row = r0 + 16 * rb + (lane & 15);
                if (row < n) {
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        const int col = cg * 128 + 32 * wave + 16 * nb + 4 * (lane >> 4);
                        if (col < cout) {        // (cout % 4 == 0: a quad is inside or outside as a whole)
                            float4 v = make_float4(acc[rb][nb][0], acc[rb][nb][1], acc[rb][nb][2], acc[rb][nb][3]);
                            if constexpr (EPI) v = epi_apply(epi, ec[nb], v, row, col, cout);  // evaluation-mode batch norm (epilogue.h)
                            *reinterpret_cast<float4*>(out + row * cout + col) = v;
                        }
                    }
                }
            }
        }
    }
}
