// The text of the weight-stationary convolution kernel (spconv_ws.hip includes it once per kernel template: the three-piece kernel
// under the name and template parameters it always had, and the reduced-precision template with a leading piece count).  Not a header
// of its own: it needs the includes and constants of spconv_ws.hip and the three macros below.
//   OSN_WS_TEMPLATE  the template header     OSN_WS_NAME  the kernel's name     OSN_WS_NP  its piece count (a constant expression)
// NP (split.h): pieces per operand -- planes staged, fragment planes held (planes 0 .. NP - 1 of the one weight image), products kept.
OSN_WS_TEMPLATE
__global__ __launch_bounds__(256) void OSN_WS_NAME(const float* __restrict__ in, const bf16x8* __restrict__ Wp,
                                                        const int32_t* __restrict__ gsrc, const int32_t* __restrict__ gdst,
                                                        const int32_t* __restrict__ poff, float* __restrict__ partial,
                                                        float* __restrict__ zeros, int n_dst, int K, int cin, int cout, int ns, int ncb, int chunk,
                                                        int direct, const Epi epi) {
    constexpr int NP = OSN_WS_NP;             // pieces per operand (split.h)
    constexpr int NT = 256;
    constexpr int CK = 32 * KS;               // input channels per chunk
    constexpr int LDA = CK + 8;               // bf16 row stride of a staged plane (16-byte aligned rows)
    constexpr int QPR = CK / 4;               // 4-channel quads per staged row
    constexpr int NQ = (32 * QPR + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) __bf16 stage[2][NP][32][LDA];
    __shared__ int sidx[WS_CH], didx[WS_CH];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.y;
    // the line of zeros the reduction reads for the offsets a row does not have
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid < 64) zeros[tid] = 0.f;
    const int pk0 = poff[k], pk1 = poff[k + 1];
    const int p0 = pk0 + blockIdx.x * chunk;
    if (p0 >= pk1) return;                                             // this offset has fewer chunks
    const int np = min(chunk, pk1 - p0);
    const int nsteps = (np + 31) >> 5;
    const int col0 = blockIdx.z * (32 * NW);
    const int cb0 = blockIdx.z * (2 * NW) + 2 * wave;                  // this wave's first 16-column block

    for (int e = tid; e < WS_CH; e += NT) {
        sidx[e] = e < np ? gsrc[p0 + e] : 0;                           // padded pair: input row 0 (valid address)
        didx[e] = e < np ? gdst[p0 + e] : -1;
    }
    int q_row[NQ], q_col[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int idx = tid + NT * j;
        q_row[j] = (idx / QPR) & 31;
        q_col[j] = (idx % QPR) * 4;
    }
    __syncthreads();

    f32x4 acc[WS_NG][2][2];
#pragma unroll
    for (int g = 0; g < WS_NG; ++g)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[g][h][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 P[NQ];
    auto fetch = [&](int g, int s0) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const unsigned row = unsigned(sidx[32 * g + q_row[j]]);
            const int ch = 32 * s0 + q_col[j];
            const unsigned cu = ch < cin ? unsigned(ch) : 0u;
            P[j] = *reinterpret_cast<const float4*>(in + (uint64_t(row) * unsigned(cin) + cu));
        }
    };
    int buf = 0;
    for (int s0 = 0; s0 < ns; s0 += KS) {
        // ---- the chunk's weight fragments: one coalesced 1 KB load each, consumed after the first barrier
        bf16x8 B[KS][2][NP];
        if (wave < NW) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const bool on = s0 + ks < ns && cb0 + nb < ncb;
                    const unsigned sb = on ? unsigned(s0 + ks) : 0u, cb = on ? unsigned(cb0 + nb) : 0u;
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) {
                        const unsigned blk = (unsigned(pl * K + k) * unsigned(ns) + sb) * unsigned(ncb) + cb;
                        B[ks][nb][pl] = (Wp + (size_t(blk) << 6))[lane];
                    }
                }
        }
        fetch(0, s0);
#pragma unroll
        for (int g = 0; g < WS_NG; ++g) {
            if (g < nsteps) {
                // ---- split the fetched quads into three bf16 pieces, stage them
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    const bool ok = 32 * s0 + q_col[j] < cin;
                    bf16x4 p[NP];
                    tl_split4<NP>(ok ? P[j] : make_float4(0.f, 0.f, 0.f, 0.f), p);      // split.h: two elements per conversion
                    if (NT * NQ == 32 * QPR || tid + NT * j < 32 * QPR) {
#pragma unroll
                        for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<bf16x4*>(&stage[buf][pl][q_row[j]][q_col[j]]) = p[pl];
                    }
                }
                if (g + 1 < nsteps) fetch(g + 1, s0);      // the next step's rows: in flight during the MFMAs below
                // one barrier per step: the other stage buffer was last read in the step before this barrier's
                __syncthreads();
                if (wave < NW) {
                    const bool half1 = np - 32 * g > 16;               // the second 16-pair half holds real pairs
                    const int akq = 8 * (lane >> 4);
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        if (s0 + ks < ns) {
                            bf16x8 af[2][NP];
#pragma unroll
                            for (int h = 0; h < 2; ++h)
#pragma unroll
                                for (int pl = 0; pl < NP; ++pl)
                                    af[h][pl] = *reinterpret_cast<const bf16x8*>(
                                        &stage[buf][pl][(half1 ? h : 0) * 16 + (lane & 15)][ks * 32 + akq]);
                            // split_products' order per accumulator (split.h), consecutive MFMAs on different accumulators
                            auto mfma_half = [&](int h, auto ap, auto bp) {
#pragma unroll
                                for (int nb = 0; nb < 2; ++nb)
                                    acc[g][h][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(B[ks][nb][bp], af[h][ap], acc[g][h][nb], 0, 0, 0);
                            };
                            if (half1) split_products<NP>([&](auto ap, auto bp) { mfma_half(0, ap, bp); mfma_half(1, ap, bp); });
                            else split_products<NP>([&](auto ap, auto bp) { mfma_half(0, ap, bp); });
                        }
                    }
                }
                buf ^= 1;
            }
        }
    }
    if (wave >= NW) return;
    EpiCols ec[2];
    if constexpr (EPI) {                         // (direct launches: the lane's two column quads, constants once)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int col = col0 + 32 * wave + 16 * nb + 4 * (lane >> 4);
            ec[nb] = epi_cols(epi, col < cout ? col : 0);
        }
    }
    // ---- result rows -> partial[k][dst].  The weight fragment is the MFMA's FIRST operand (the staged rows the second), so a
    // block comes out transposed: lane l holds columns 4 (l >> 4) .. + 3 of pair l & 15 -- one 16-byte store per block
#pragma unroll
    for (int g = 0; g < WS_NG; ++g) {
        if (g < nsteps) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int d = didx[32 * g + 16 * h + (lane & 15)];
                if (d >= 0) {
                    // direct: every destination row has exactly one pair in the whole map -- `partial` IS the output
                    float* row = partial + ((direct ? int64_t(0) : int64_t(k) * n_dst) + d) * cout;
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        const int col = col0 + 32 * wave + 16 * nb + 4 * (lane >> 4);
                        if (col < cout) {
                            float4 v = make_float4(acc[g][h][nb][0], acc[g][h][nb][1], acc[g][h][nb][2], acc[g][h][nb][3]);
                            if constexpr (EPI) v = epi_apply(epi, ec[nb], v, d, col, cout);
                            *reinterpret_cast<float4*>(row + col) = v;
                        }
                    }
                }
            }
        }
    }
}
