// The text of the register-gather convolution kernel (spconv_rg.hip includes it once per kernel template: the three-piece kernel
// under the name and template parameters it always had, and the reduced-precision template with a leading piece count).  Not a header
// of its own: it needs the includes and constants of spconv_rg.hip and the three macros below.
//   OSN_RG_TEMPLATE  the template header     OSN_RG_NAME  the kernel's name     OSN_RG_NP  its piece count (a constant expression)
// NP (split.h): pieces per operand -- pieces formed of a gathered row, fragment planes held (planes 0 .. NP - 1 of the one weight
// image), products kept.
OSN_RG_TEMPLATE
__global__ __launch_bounds__(256, OCC) void OSN_RG_NAME(const float* __restrict__ in, const bf16x8* __restrict__ Wp,
                                                        const int32_t* __restrict__ nbr, const int32_t* __restrict__ out_rows,
                                                        float* __restrict__ out, int n_out, int K, int cin, int cout,
                                                        unsigned in_bytes, const Epi epi) {
    constexpr int NP = OSN_RG_NP;                                 // pieces per operand (split.h)
    constexpr int ROWS = 64 * HALVES;
    constexpr int LDR = 32 + 4;                                   // fp32 row pitch of a partial tile in LDS (32 columns per pass)
    __shared__ __attribute__((aligned(16))) float red[4][64][LDR];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int row0 = blockIdx.x * ROWS;
    const __amdgpu_buffer_rsrc_t insrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, int(in_bytes), 0x00020000);
    const unsigned cin4 = unsigned(cin) * 4u;
    const unsigned ns = unsigned(KS), ncb = unsigned(NCB);
    const uint32_t plane_blocks = unsigned(K) * ns * ncb;        // 1 KB blocks per bf16 piece of the whole weight

    f32x4 acc[HALVES][RG_RB][NCB];
#pragma unroll
    for (int h = 0; h < HALVES; ++h)
#pragma unroll
        for (int rb = 0; rb < RG_RB; ++rb)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[h][rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    // table entries of offset k for this lane's A rows: row (h, rb, l15); rows past the table: -1
    auto load_idx = [&](int k, int (&idx)[HALVES][RG_RB]) {
#pragma unroll
        for (int h = 0; h < HALVES; ++h)
#pragma unroll
            for (int rb = 0; rb < RG_RB; ++rb) {
                const int r = row0 + 64 * h + 16 * rb + l15;
                const bool on = k < K && r < n_out;
                const int v = nbr[on ? int64_t(k) * n_out + r : 0];
                idx[h][rb] = on ? v : -1;
            }
    };
    // the lane's 32 bytes of every gathered row (absent neighbour: offset past the matrix -> zeros, no memory access)
    auto gather = [&](const int (&idx)[HALVES][RG_RB], float4 (&P)[HALVES][RG_RB][KS][2]) {
#pragma unroll
        for (int h = 0; h < HALVES; ++h)
#pragma unroll
            for (int rb = 0; rb < RG_RB; ++rb) {
                const unsigned base = idx[h][rb] >= 0 ? __umul24(unsigned(idx[h][rb]), cin4) + 32u * unsigned(lg) : 0xFFFFFF00u;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const unsigned o = idx[h][rb] >= 0 ? base + 128u * unsigned(ks) : base;
                    P[h][rb][ks][0] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(insrc, o, 0, 0));
                    P[h][rb][ks][1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(insrc, o + 16u, 0, 0));
                }
            }
    };

    int idxA[HALVES][RG_RB], idxB[HALVES][RG_RB];
    float4 PA[HALVES][RG_RB][KS][2], PB[HALVES][RG_RB][KS][2];
    // software pipeline over this wave's offsets k = wave, wave + 4, ...: table entries two offsets ahead, gathered rows one ahead
    load_idx(wave, idxA);
    load_idx(wave + 4, idxB);
    gather(idxA, PA);

    auto load_b = [&](int k, bf16x8 (&B)[KS][NCB][NP]) {
        const unsigned kk = k < K ? unsigned(k) : 0u;            // (past the last offset: any valid block, never multiplied)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
                    const uint32_t blk = uint32_t(pl) * plane_blocks + (kk * ns + unsigned(ks)) * ncb + unsigned(cb);
                    B[ks][cb][pl] = (Wp + (size_t(blk) << 6))[lane];
                }
    };
    bf16x8 BA[KS][NCB][NP], BB[BD ? KS : 1][BD ? NCB : 1][NP];
    if (BD) load_b(wave, BA);

    auto body = [&](int k, int (&idx_cur)[HALVES][RG_RB], float4 (&P_cur)[HALVES][RG_RB][KS][2], int (&idx_nxt)[HALVES][RG_RB],
                    float4 (&P_nxt)[HALVES][RG_RB][KS][2], bf16x8 (&B)[KS][NCB][NP], bf16x8 (&B_nxt)[BD ? KS : 1][BD ? NCB : 1][NP]) {
        // which (half, block) groups have any pair at this offset (wave-uniform masks), before idx_cur is recycled
        bool any[HALVES][RG_RB];
#pragma unroll
        for (int h = 0; h < HALVES; ++h)
#pragma unroll
            for (int rb = 0; rb < RG_RB; ++rb) any[h][rb] = __ballot(idx_cur[h][rb] >= 0) != 0ull;
        // weight fragments: one coalesced 1 KB load each -- this offset's now, or (BD) the next offset's into the other set
        if constexpr (BD) {
            load_b(k + 4, reinterpret_cast<bf16x8(&)[KS][NCB][NP]>(B_nxt));
        } else {
            load_b(k, B);
        }
        // next offset's rows in flight during this offset's MFMAs; the offset after that: its table entries
        gather(idx_nxt, P_nxt);
        load_idx(k + 8, idx_cur);
#pragma unroll
        for (int h = 0; h < HALVES; ++h)
#pragma unroll
            for (int rb = 0; rb < RG_RB; ++rb) {
                if (any[h][rb]) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        bf16x8 A[NP];
                        split8<NP>(P_cur[h][rb][ks][0], P_cur[h][rb][ks][1], A);
                        // split_products' order per accumulator (split.h); consecutive MFMAs on different accumulators
                        split_products<NP>([&](auto ap, auto bp) {
#pragma unroll
                            for (int cb = 0; cb < NCB; ++cb)
                                acc[h][rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(B[ks][cb][bp], A[ap], acc[h][rb][cb], 0, 0, 0);
                        });
                    }
                }
            }
    };
    for (int k = wave; k < K; k += 8) {
        if constexpr (BD) {
            body(k, idxA, PA, idxB, PB, BA, BB);
            if (k + 4 < K) body(k + 4, idxB, PB, idxA, PA, reinterpret_cast<bf16x8(&)[KS][NCB][NP]>(BB), reinterpret_cast<bf16x8(&)[BD ? KS : 1][BD ? NCB : 1][NP]>(BA));
        } else {
            body(k, idxA, PA, idxB, PB, BA, BB);
            if (k + 4 < K) body(k + 4, idxB, PB, idxA, PA, BA, BB);
        }
    }

    // ---- the four waves' partial tiles -> out, summed in wave order (64 rows x 32 columns at a time through LDS)
#pragma unroll
    for (int h = 0; h < HALVES; ++h) {
#pragma unroll
        for (int cp = 0; cp < NCB / 2; ++cp) {
            if (h > 0 || cp > 0) __syncthreads();                // the previous pass has been read
#pragma unroll
            for (int rb = 0; rb < RG_RB; ++rb)
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2)
                    *reinterpret_cast<f32x4*>(&red[wave][16 * rb + l15][16 * c2 + 4 * lg]) = acc[h][rb][2 * cp + c2];
            __syncthreads();
            EpiCols ec;
            if constexpr (EPI) ec = epi_cols(epi, 32 * cp + 4 * (tid & 7));       // (256 % 8 == 0: a thread keeps its column quad)
            for (int e = tid; e < 64 * 8; e += 256) {
                const int j = e >> 3, c4 = e & 7;
                const int r = row0 + 64 * h + j;
                if (r < n_out) {
                    float4 s = *reinterpret_cast<const float4*>(&red[0][j][4 * c4]);
#pragma unroll
                    for (int w = 1; w < 4; ++w) {
                        const float4 v = *reinterpret_cast<const float4*>(&red[w][j][4 * c4]);
                        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
                    }
                    const int64_t orow = out_rows ? out_rows[r] : r;
                    if constexpr (EPI) s = epi_apply(epi, ec, s, orow, 32 * cp + 4 * c4, cout);
                    *reinterpret_cast<float4*>(out + orow * cout + 32 * cp + 4 * c4) = s;
                }
            }
        }
    }
}
