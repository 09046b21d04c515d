// The text of the tile-list convolution kernel (spconv_tl.hip includes it once per kernel template: the three-piece kernel under the
// name and template parameters it always had, and the reduced-precision template with a leading piece count).  Not a header of its own:
// it needs the includes, constants and TL_TICK of spconv_tl.hip and the three macros below.
//   OSN_TL_TEMPLATE  the template header     OSN_TL_NAME  the kernel's name     OSN_TL_NP  its piece count (a constant expression)
// NP (split.h): pieces per operand -- planes staged to LDS (stage[NP]), fragment planes held in registers (B[KS][2][NP], planes
// 0 .. NP - 1 of the one weight image), MFMAs issued per block (6 / 3 / 1).
OSN_TL_TEMPLATE
__global__ __launch_bounds__(256, OCC) void OSN_TL_NAME(const float* __restrict__ in, const bf16x8* __restrict__ Wp,
                                                               const int32_t* __restrict__ cnt, const int2* __restrict__ lst,
                                                               const int32_t* __restrict__ out_rows, float* __restrict__ out,
                                                               double* __restrict__ bn_partial, int32_t* __restrict__ counter,
                                                               float* __restrict__ partial, int nz, int n_out, int K, int cin,
                                                               int cout, int bm, int n_tiles, int ns, int ncb,
                                                               int self_reset, long long* __restrict__ prof, unsigned in_bytes,
                                                               const Epi epi) {
    constexpr int NP = OSN_TL_NP;             // pieces per operand (split.h)
    static_assert(!(BUFG && RAGGED), "the buffer gather is for full channel chunks");
    constexpr int NT = 256;
    constexpr int CW = 32 * NW;               // output columns of the workgroup
    constexpr int S = CW + 4;                 // fp32 row stride of the output tile
    constexpr int CK = 32 * KS;               // input channels per chunk
    constexpr int LDA = CK + 8;               // bf16 row stride of a staged plane (16-byte aligned rows)
    constexpr int QPR = CK / 4;                           // 4-channel quads per staged row
    constexpr int NQ = (32 * QPR + NT - 1) / NT;          // quads per thread per step
    constexpr int NL = (TL_LCAP + NT - 1) / NT;           // list entries per thread per batch
    // the fp32 output tile: bm rows + one dump row for padded pairs.  Dynamic LDS (sized by the launch from the map's tile height):
    // a 64-row tile leaves room for a third workgroup per CU (the OCC = 3 instances)
    extern __shared__ __attribute__((aligned(16))) float otile[];
    __shared__ __attribute__((aligned(16))) __bf16 stage[NP][32][LDA];
    __shared__ uint32_t plist[TL_LCAP];       // (local output row << 24) | input row, 32-padded per offset
    __shared__ int klist[TL_KMAX];
    __shared__ int kcnt[TL_KMAX];
    __shared__ int lstart[TL_KMAX + 1];       // first plist slot of each offset of the current batch
    __shared__ unsigned char gowner[TL_LCAP / 32];
    // Round 4: the batch's (offset, chunk, step) sequence as a TABLE, written once per batch by one thread per offset:
    //   x = first plist slot of the step   y = pairs of the step (1 .. 32) | first step of its (offset, chunk) << 8 | first
    //   k-step of the chunk << 16          z = 1 KB weight block of (offset, chunk): (k ns + s0) ncb
    // Round 3's loop advanced three iterators per step through LDS look-ups (pairs, list start and offset of the current
    // list entry, each a dependent read + readfirstlane) and rebuilt every weight-fragment address from scalars: 220 scalar
    // and 35 wait instructions per 72 MFMAs.  The kernel is bound by instruction issue (with every byte of memory traffic
    // removed it runs 149 instead of 173 us, profiles/r04_s2_*), so the control path is what there is to cut.
    __shared__ uint4 stab[TL_STEPS];
    __shared__ int nact_s, bend_s, tile_s;

    long long tacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long tlast = PROF ? __builtin_amdgcn_s_memtime() : 0;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);         // wave-uniform => scalar registers
    const int col0 = blockIdx.y * CW;
    // (Rotating which wave of a workgroup is the staging-only one -- so that the staging waves of co-resident workgroups do not
    // all sit on one SIMD -- was measured: 1 - 7 % SLOWER, profiles/r04_s6_ab_wave_role_rotation.txt.  Waves keep their columns.)
    const int cw = wave;                                               // column-owner index of this wave (>= NW: staging only)
    const int cb0 = blockIdx.y * (2 * NW) + 2 * cw;                    // this wave's first 16-column block

    // loop-invariant staging coordinates of this thread's quads (full 128-channel rows; narrower chunks mask)
    int q_row[NQ], q_col[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int idx = tid + NT * j;
        q_row[j] = (idx / QPR) & 31;
        q_col[j] = (idx % QPR) * 4;
    }
    // BUFG: resource over the feature matrix (raw buffer, 32-bit byte offsets; in_bytes < 2^31 is the launch's condition)
    const __amdgpu_buffer_rsrc_t insrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, int(BUFG ? in_bytes : 0u), 0x00020000);
    const unsigned cin4 = unsigned(cin) * 4u;

    bf16x8 B[KS][2][NP];
    float4 P0[NQ], P1[NQ];
    // RAGGED = false: every channel chunk is full (every MinkUNet width) -- no channel masks, no fragment selects in the loop
    constexpr bool ragged = RAGGED;
    // a fragment load is ONE instruction: scalar base of (offset, chunk, k-step, plane) + this lane's byte offset inside the
    // column block (two registers: one per column block of the wave).  Column blocks past the weight are never stored: they
    // read block 0 instead (valid memory).
    uint32_t boff[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) boff[nb] = (cb0 + nb < ncb ? unsigned(cb0 + nb) : 0u) * 1024u + 16u * unsigned(lane);
    const uint32_t plane_bytes = unsigned(K) * unsigned(ns) * unsigned(ncb) * 1024u;      // one bf16 piece of the whole weight
    const uint32_t kstep_bytes = unsigned(ncb) * 1024u;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8*>(Wp), 0, int(3u * plane_bytes), 0x00020000);   // raw buffer, 32-bit offsets

    for (;;) {
        // ---- draw the next tile (densest first: a tile-ordered table has the rows with most neighbours last)
        if (tid == 0) tile_s = atomicAdd(&counter[blockIdx.y], 1);
        __syncthreads();
        // A unit of work = (tile, part z of nz): small tables cut the tile's active offsets into nz contiguous
        // parts handled by different workgroups (a tile's offsets are a serial chain: weights, then its steps);
        // part z writes its own partial tile, summed in part order by reduce_partial_rows_kernel.
        const int draw = __builtin_amdgcn_readfirstlane(tile_s);
        if (draw >= n_tiles * nz) break;
        const int tile = n_tiles - 1 - draw / nz;
        const int zpart = draw - (draw / nz) * nz;
        const int row0 = tile * bm;
        const int rows = min(bm, n_out - row0);
        // The tile's output row ids: loaded at the draw, parked before the epilogue in the unused tail of kcnt[] (K <= 40 offsets),
        // so that no load sits between the last MFMA and the stores: 96 -> 96 -1 %, 128 -> 96 -2 % (profiles/r04_s11_*).  NO new LDS
        // for it: 352 more bytes cross an allocation granule, the third workgroup per CU is gone and the kernel runs 138 instead
        // of 125 us (measured).  Also measured there: the next draw issued at the start of the epilogue (-1 % / 0), and a whole
        // tile of look-ahead -- draw and offset counts in flight across the steps -- 30 % SLOWER: the compiler's waitcnt pass sees
        // loads pending across the step loop and gives up its counted waits, and a reserved tile is lost to the dynamic balance.
        const bool park = K <= TL_KMAX - TL_BMAX;
        int* const orow_s = kcnt + (TL_KMAX - TL_BMAX);
        const int orow_pre = (park && tid < rows) ? (out_rows ? out_rows[row0 + tid] : row0 + tid) : 0;

        {
            // the zeros are materialised HERE (opaque to the optimiser): hoisted out of the persistent loop they stayed live across
            // every step, were spilled, had their registers borrowed as an MFMA temporary and were reloaded from scratch memory in
            // each step of the 96 -> 96 instance (ISA: one scratch_load_dwordx4 per step in the in-order vmcnt queue of the gathers)
            float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            asm volatile("" : "+v"(z.x), "+v"(z.y), "+v"(z.z), "+v"(z.w));
            for (int i = tid; i < (bm + 1) * S / 4; i += NT) reinterpret_cast<float4*>(otile)[i] = z;
        }

        // ---- active offsets of the tile, ascending (=> fixed summation order)
        if (cnt) {
            if (wave == 0) {
                int n = 0;
                for (int k0 = 0; k0 < K; k0 += 64) {
                    const int k = k0 + lane;
                    const int c = k < K ? cnt[int64_t(tile) * K + k] : 0;
                    const unsigned long long m = __ballot(c > 0);
                    if (c > 0) {
                        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
                        klist[pos] = k;
                        kcnt[pos] = c;
                    }
                    n += __popcll(m);
                }
                if (lane == 0) nact_s = n;
            }
        } else if (tid == 0) {              // identity map (K == 1): the tile's own rows, in order
            klist[0] = 0;
            kcnt[0] = rows;
            nact_s = 1;
        }
        __syncthreads();
        const int nact_all = __builtin_amdgcn_readfirstlane(nact_s);
        const int nact = nact_all * (zpart + 1) / nz;      // this part: active offsets [nact_all z / nz, nact_all (z + 1) / nz)
        TL_TICK(0)                                         // 0: tile draw, zeroing, active offsets

        int a0 = nact_all * zpart / nz;
        while (a0 < nact) {
            // ---- batch [a0, a1): as many consecutive offsets as fit the LDS list buffer
            if (tid == 0) {
                int tot = 0, a = a0;
                while (a < nact) {
                    const int np = (kcnt[a] + 31) & ~31;
                    if (tot + np > TL_LCAP) break;         // a single offset (<= 96 entries) always fits
                    lstart[a] = tot;
                    tot += np;
                    ++a;
                }
                lstart[a] = tot;
                bend_s = a;
            }
            __syncthreads();                               // (also: the previous batch is done with plist / lstart)
            const int a1 = __builtin_amdgcn_readfirstlane(bend_s);
            const int E = __builtin_amdgcn_readfirstlane(lstart[a1]);
            for (int a = a0 + tid; a < a1; a += NT)
                for (int g = lstart[a] >> 5; g < (lstart[a + 1] >> 5); ++g) gowner[g] = (unsigned char)a;
            __syncthreads();
            if (cnt) {
                // all loads first (unconditional, clamped addresses), then the selects and the LDS writes: one
                // exposed memory latency per batch instead of one per entry
                int2 x[NL];
                bool okv[NL];
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                    const int e = tid + NT * j;
                    const int ec = e < E ? e : 0;
                    const int a = gowner[ec >> 5];
                    const int p = ec - lstart[a];
                    okv[j] = e < E && p < kcnt[a];
                    x[j] = lst[(int64_t(tile) * K + klist[a]) * bm + (okv[j] ? p : 0)];
                }
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                    // padded pair: input row 0 (valid address), dump row
                    const uint32_t v = okv[j] ? ((uint32_t(x[j].y) << 24) | uint32_t(x[j].x)) : (uint32_t(bm) << 24);
                    if (tid + NT * j < E) plist[tid + NT * j] = v;
                }
            } else {
                for (int e = tid; e < E; e += NT)
                    plist[e] = e < rows ? ((uint32_t(e) << 24) | uint32_t(row0 + e)) : (uint32_t(bm) << 24);
            }
            // step table of the batch: offset a owns entries [nchunk (lstart[a] / 32), + nchunk niter(a)), chunk-major
            const int nchunk = (ns + KS - 1) / KS;
            for (int a = a0 + tid; a < a1; a += NT) {
                const int np = kcnt[a], niter = (np + 31) >> 5, l0 = lstart[a];
                const int kk = cnt ? klist[a] : 0;
                int t = nchunk * (l0 >> 5);
                for (int c = 0; c < nchunk; ++c)
                    for (int g = 0; g < niter; ++g, ++t)
                        stab[t] = make_uint4(uint32_t(l0 + 32 * g), uint32_t(min(32, np - 32 * g)) | (g == 0 ? 0x100u : 0u) | (uint32_t(c * KS) << 16),
                                             uint32_t((kk * ns + c * KS) * ncb), 0u);
            }
            const int T = nchunk * (E >> 5);
            __syncthreads();
            TL_TICK(1)                                     // 1: batch list load

            // ---- flat pipeline over the step table of the batch
            struct Step {
                int base, fl, blk0;           // stab entry (scalars); base < 0: past the end
                __device__ bool valid() const { return base >= 0; }
                __device__ int np() const { return fl & 0xFF; }
                __device__ bool first() const { return (fl & 0x100) != 0; }
                __device__ int s0() const { return fl >> 16; }
            };
            auto entry = [&](int t) {
                Step e;
                if (t < T) {
                    const uint4 v = stab[t];
                    e.base = __builtin_amdgcn_readfirstlane(int(v.x));
                    e.fl = __builtin_amdgcn_readfirstlane(int(v.y));
                    e.blk0 = __builtin_amdgcn_readfirstlane(int(v.z));
                } else {
                    e.base = -1; e.fl = 0; e.blk0 = 0;
                }
                return e;
            };
            // gather of one step: 32 list entries x up to 128 channels, one 16-byte load per quad (unconditional,
            // clamped address; masked at conversion time)
            auto fetch = [&](const Step& it, float4 (&P)[NQ]) {
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    const unsigned row = plist[it.base + q_row[j]] & 0xFFFFFFu;
                    if constexpr (BUFG) {
                        const unsigned voff = __umul24(row, cin4) + 4u * unsigned(q_col[j]);      // < in_bytes < 2^31 for every listed row
                        P[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(insrc, voff, 128u * unsigned(it.s0()), 0));
                    } else {
                        const int ch = 32 * it.s0() + q_col[j];
                        const unsigned cu = ch < cin ? unsigned(ch) : 0u;
                        P[j] = *reinterpret_cast<const float4*>(in + (uint64_t(row) * unsigned(cin) + cu));
                    }
                }
            };
            // fragments of k-step ks of the (offset, chunk) that step `u` belongs to: buffer loads -- resource = the whole weight
            // image, scalar offset = (offset, chunk, k-step, plane), vector offset = the lane's two precomputed registers
            auto load_b = [&](int ks, const Step& u) {
                const uint32_t ub = uint32_t(u.blk0) << 10;                                           // wave-uniform
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
                    // k-steps past the last chunk (ragged only) are never multiplied: any valid block will do (ks 0's)
                    const int kk = (!ragged || u.s0() + ks < ns) ? ks : 0;
                    const uint32_t so = ub + uint32_t(pl) * plane_bytes + uint32_t(kk) * kstep_bytes;  // scalar
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
                        B[ks][nb][pl] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, boff[nb], so, 0));
                }
            };
            bool b_ahead = false;          // this step's fragments were loaded during the previous step
            auto step = [&](const Step& it, float4 (&P)[NQ], const Step& n1s, const Step& nf) {
                // ---- split the fetched quads into three bf16 pieces (registers), two elements per conversion; channels past
                // the input (only when cin is not a multiple of the chunk) are zeroed first
                bf16x4 pc[NQ][NP];
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    float4 v = P[j];
                    if (ragged && !(32 * it.s0() + q_col[j] < cin)) v = make_float4(0.f, 0.f, 0.f, 0.f);
                    tl_split4<NP>(v, pc[j]);
                }
                TL_TICK(2)                                 // 2: wait for the gathered rows + split
                // ---- new (offset, chunk): B fragments of this wave's 32 columns, one coalesced 1 KB load each -- unless the
                // previous step already fetched them behind its own MFMAs (see the end of the k-step loop)
                if (it.first() && !b_ahead && cw < NW) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) load_b(ks, it);
                }
                // the NEXT step opens a new (offset, chunk): its fragments are loaded into the registers of k-step ks as soon as
                // this step's MFMAs of ks are issued (the last use of the current ones), i.e. beside the remaining MFMAs, the tile
                // write-back and the two barriers -- no second register set
                const bool ahead = n1s.valid() && n1s.first() && cw < NW;
                TL_TICK(8)                                 // 8: B-load issue
                __syncthreads();                           // every wave is done reading the previous stage
                TL_TICK(3)                                 // 3: barrier A
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    if (NT * NQ == 32 * QPR || tid + NT * j < 32 * QPR) {
#pragma unroll
                        for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<bf16x4*>(&stage[pl][q_row[j]][q_col[j]]) = pc[j][pl];
                    }
                }
                if (nf.valid()) fetch(nf, P);              // ahead of time; in flight during the MFMAs below
                TL_TICK(9)                                 // 9: stage write + next gather issue
                __syncthreads();                           // stage ready
                TL_TICK(4)                                 // 4: barrier B
                if (cw >= NW) { b_ahead = false; return; }     // staging-only wave
                // ---- 32 pairs x 32 columns per wave: accumulator blocks [pair half][column block]
                // (the last step of an offset may hold at most 16 pairs -- the average (tile, offset) of a 100 k-row map
                // has 36 -- : its second 16-pair half is all padding and is skipped: MFMAs, fragment reads, tile update)
                const bool half1 = it.np() > 16;                    // wave-uniform
                // Round 4: the accumulators START from the output tile's cells and are stored back after the last MFMA.  The
                // MFMAs take the WEIGHT fragment as their first operand and the staged rows as the second (same registers either
                // way round: both fragment layouts are [16 rows or columns][8 k per lane group]), i.e. they produce the block
                // TRANSPOSED: lane l holds columns 4 (l >> 4) .. + 3 of pair l & 15 -- four consecutive floats of one output row,
                // one 16-byte LDS access.  Round 3 added the finished block in a separate read-add-write phase, which the
                // compiler turned into a chain of eight dependent 8-byte LDS round trips (it could not prove the 16-byte
                // alignment): 920 of a step's 7 100 clocks.  Now the tile cells are read while the fragments are, and written
                // once.  (Within one offset an output row occurs at most once and a wave owns its columns: no other access to
                // these cells between the read and the write.)
                const int pbase = it.base + (lane & 15);
                int ocell[2];
                f32x4 acc[2][2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 0 || half1) {
                        ocell[h] = int(plist[pbase + 16 * h] >> 24) * S + 32 * cw + 4 * (lane >> 4);
                        const f32x4* cell = reinterpret_cast<const f32x4*>(__builtin_assume_aligned(&otile[ocell[h]], 16));
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) acc[h][nb] = cell[4 * nb];
                    }
                }
                const int akq = 8 * (lane >> 4);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (!ragged || it.s0() + ks < ns) {
                        bf16x8 af[2][NP];
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int pl = 0; pl < NP; ++pl)
                                af[h][pl] = *reinterpret_cast<const bf16x8*>(&stage[pl][(half1 ? h : 0) * 16 + (lane & 15)][ks * 32 + akq]);
                        // product-major order: consecutive MFMAs go to DIFFERENT accumulators (a dependent chain per
                        // accumulator would stall the in-order issue on every MFMA's result); per accumulator the
                        // order is that of split_products (split.h)
                        auto mfma_half = [&](int h, auto ap, auto bp) {
#pragma unroll
                            for (int nb = 0; nb < 2; ++nb)
                                acc[h][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(B[ks][nb][bp], af[h][ap], acc[h][nb], 0, 0, 0);
                        };
                        if (half1) split_products<NP>([&](auto ap, auto bp) { mfma_half(0, ap, bp); mfma_half(1, ap, bp); });
                        else split_products<NP>([&](auto ap, auto bp) { mfma_half(0, ap, bp); });
                    }
                    if (ahead) load_b(ks, n1s);
                }
                b_ahead = ahead;
                if (PROF) {                                // force the MFMA results (and thus the B loads) before the tick
                    float sink = 0.f;
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb)
                            if (h == 0 || half1) sink += acc[h][nb][0];
                    asm volatile("" ::"v"(sink));
                }
                TL_TICK(5)                                 // 5: B-load wait + tile / fragment reads + MFMAs
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 0 || half1) {
                        f32x4* cell = reinterpret_cast<f32x4*>(__builtin_assume_aligned(&otile[ocell[h]], 16));
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) cell[4 * nb] = acc[h][nb];
                    }
                }
                TL_TICK(6)                                 // 6: output-tile write-back
            };

            Step cur = entry(0), n1 = entry(1), n2 = entry(2);
            int tn = 3;
            if (cur.valid()) fetch(cur, P0);
            if (n1.valid()) fetch(n1, P1);
            while (cur.valid()) {
                step(cur, P0, n1, n2);
                cur = n1; n1 = n2; n2 = entry(tn++);
                if (!cur.valid()) break;
                step(cur, P1, n1, n2);
                cur = n1; n1 = n2; n2 = entry(tn++);
            }
            a0 = a1;
        }
        if (park && tid < rows) orow_s[tid] = orow_pre;
        __syncthreads();

        // ---- epilogue: tile rows -> out[out_rows[row]] (16-byte stores), optional batch-norm partial sums
        constexpr int V = CW / 4;
        if constexpr (EPI) {
            // a thread keeps ONE column quad and walks the rows (NT / V rows per pass): the stage's per-column constants -- four loads and
            // four reciprocal square roots -- once per tile and thread instead of once per stored quad
            constexpr int RPP = NT / V;
            const int c4 = tid % V, col = col0 + 4 * c4;
            if (tid < RPP * V && col < cout) {
                const EpiCols ec = epi_cols(epi, col);
                for (int j = tid / V; j < rows; j += RPP) {
                    const float4 v = *reinterpret_cast<const float4*>(&otile[j * S + 4 * c4]);
                    const int64_t orow = park ? orow_s[j] : (out_rows ? out_rows[row0 + j] : row0 + j);
                    *reinterpret_cast<float4*>(out + orow * cout + col) = epi_apply(epi, ec, v, orow, col, cout);
                }
            }
        } else
        for (int idx = tid; idx < rows * V; idx += NT) {
            const int j = idx / V, c4 = idx - j * V;
            const int col = col0 + 4 * c4;
            if (col < cout) {
                const float4 v = *reinterpret_cast<const float4*>(&otile[j * S + 4 * c4]);
                if (nz > 1) {                              // partial tile of part z, table row order
                    *reinterpret_cast<float4*>(partial + (int64_t(zpart) * n_out + row0 + j) * cout + col) = v;
                } else {
                    const int64_t orow = park ? orow_s[j] : (out_rows ? out_rows[row0 + j] : row0 + j);
                    // (inference: evaluation-mode batch norm + residual + ReLU on the finished row, epilogue.h)
                    *reinterpret_cast<float4*>(out + orow * cout + col) = v;
                }
            }
        }
        if (bn_partial) {
            for (int c = tid; c < CW; c += NT) {
                if (col0 + c < cout) {
                    double s1 = 0, s2 = 0;
                    for (int j = 0; j < rows; ++j) {
                        const double v = otile[j * S + c];
                        s1 += v;
                        s2 += v * v;
                    }
                    bn_partial[(int64_t(tile) * 2 + 0) * cout + col0 + c] = s1;
                    bn_partial[(int64_t(tile) * 2 + 1) * cout + col0 + c] = s2;
                }
            }
        }
        __syncthreads();                                   // the tile buffer is free for the next draw
        TL_TICK(7)                                         // 7: epilogue
    }
    if (PROF && tid == 0 && blockIdx.y == 0)
        for (int i = 0; i < 10; ++i) prof[int64_t(blockIdx.x) * 10 + i] = tacc[i];
    // caller-owned persistent counters: the last workgroup of a column group to leave (every other one has made its final
    // draw before it took its exit ticket) puts both counters back to zero for the next launch -- no memset per call
    if ((self_reset & 1) && tid == 0) {
        const int done = atomicAdd(&counter[64 + blockIdx.y], 1);
        if (done == int(gridDim.x) - 1) {
            counter[blockIdx.y] = 0;
            counter[64 + blockIdx.y] = 0;
        }
    }
}
