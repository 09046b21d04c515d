// The pair-array weight-gradient kernel's text (wgrad_tl.hip), included once per kernel template.  The including file defines
//   OSN_WG_TEMPLATE  the template header     OSN_WG_NAME  the kernel's name     OSN_WG_NP  its piece count (a constant expression)
// NP pieces per operand (split.h): NP planes of each operand are split, staged in LDS and read back transposed, and the products of
// split_products<NP> are accumulated -- 6 / 3 / 1 MFMAs per 16 x 16 block and 32-pair step.  No include guard: that is the point.
OSN_WG_TEMPLATE
__global__ __launch_bounds__(256, 2) void OSN_WG_NAME(const float* __restrict__ rows_a, const float* __restrict__ rows_g,
                                                      const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_g,
                                                      const int32_t* __restrict__ poff, const int4* __restrict__ items,
                                                      float* __restrict__ partial, int ca, int cg, int n_cgb,
                                                      int ident_rows, int ident_quota, unsigned a_bytes, unsigned g_bytes) {
    constexpr int NP = OSN_WG_NP;                        // pieces per operand (split.h)
    constexpr int CA_T = 32 * MB, CG_T = 32 * NB;
    constexpr int LDA = CA_T + 8, LDG = CG_T + 8;        // bf16 row pitch (16-byte aligned rows)
    constexpr int QA = CA_T / 4, QG = CG_T / 4;          // quads per staged row
    __shared__ __attribute__((aligned(16))) __bf16 Ap[NP][32][LDA];
    __shared__ __attribute__((aligned(16))) __bf16 Gp[NP][32][LDG];
    __shared__ int idxbuf[2][32];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    const int a0 = (blockIdx.x / n_cgb) * CA_T;          // first input channel of the workgroup's block
    const int g0 = (blockIdx.x % n_cgb) * CG_T;
    int k, p0, p1, base;
    int pstep = 32;                                      // pairs between this item's consecutive 32-pair steps
    if (idx_a) {
        const int4 it = items[blockIdx.y];
        k = it.x; p0 = it.y; p1 = it.z;
        if (k < 0) return;
        base = poff[k];
        // item.w = j | n << 16 (0 = the whole range): the item takes the steps j, j + n, ... of [p0, p1) -- strided items of one row
        // region walk its rows together (round 6: Z-ordered pair arrays, tools/micro_crowd.py)
        const int n_it = it.w >> 16;
        if (n_it > 1) { p0 += 32 * (it.w & 0xFFFF); pstep = 32 * n_it; }
        if (p0 >= p1) p1 = p0;                           // (an item past the range's last step: nothing to add, zeros are stored)
    } else {
        k = 0; base = 0;
        p0 = blockIdx.y * ident_quota;
        p1 = min(p0 + ident_quota, ident_rows);
        if (p0 >= p1) return;
    }
    (void)k;

    f32x4 acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging coordinates of this thread's quads (MB of the A rows, NB of the G rows)
    int ar[MB], ac[MB], gr[NB], gc[NB];
#pragma unroll
    for (int j = 0; j < MB; ++j) { const int idx = tid + 256 * j; ar[j] = idx / QA; ac[j] = (idx - ar[j] * QA) * 4; }
#pragma unroll
    for (int j = 0; j < NB; ++j) { const int idx = tid + 256 * j; gr[j] = idx / QG; gc[j] = (idx - gr[j] * QG) * 4; }

    const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rows_a), 0, int(BUFG ? a_bytes : 0u), 0x00020000);
    const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rows_g), 0, int(BUFG ? g_bytes : 0u), 0x00020000);
    const unsigned ca4 = unsigned(ca) * 4u, cg4 = unsigned(cg) * 4u;
    float4 pa[MB], pg[NB];
    // the (input row, output row) of pair p0 + s * 32 + (tid & 31): threads 0..31 hold the A index, 32..63 the G index
    auto load_idx = [&](int p) -> int {
        const int q = p + (tid & 31);
        if (tid >= 64) return -1;
        if (q >= p1) return -1;
        if (!idx_a) return q;
        return tid < 32 ? idx_a[base + q] : idx_g[base + q];
    };
    auto fetch = [&](int par) {
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            const int r = idxbuf[0][ar[j]];
            const int ch = a0 + ac[j];
            if constexpr (BUFG) {       // (channels past the operand: inside the matrix or past its end, where the resource returns zeros)
                pa[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                       arsrc, __umul24(unsigned(max(r, 0)), ca4) + 4u * unsigned(ch), 0, 0));
                continue;
            }
            const bool ok = r >= 0 && ch < ca;
            const unsigned ru = ok ? unsigned(r) : 0u, cu = ok ? unsigned(ch) : 0u;
            pa[j] = *reinterpret_cast<const float4*>(rows_a + (uint64_t(ru) * unsigned(ca) + cu));
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int r = idxbuf[1][gr[j]];
            const int ch = g0 + gc[j];
            if constexpr (BUFG) {
                pg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                       grsrc, __umul24(unsigned(max(r, 0)), cg4) + 4u * unsigned(ch), 0, 0));
                continue;
            }
            const bool ok = r >= 0 && ch < cg;
            const unsigned ru = ok ? unsigned(r) : 0u, cu = ok ? unsigned(ch) : 0u;
            pg[j] = *reinterpret_cast<const float4*>(rows_g + (uint64_t(ru) * unsigned(cg) + cu));
        }
        (void)par;
    };
    // NP bf16 pieces per element, two elements per conversion (split.h); rows of padded pairs and channels past the
    // operand are zeroed first
    // (three named pieces and `if constexpr`, not arrays indexed by the piece: with arrays six of the three-piece instances were
    //  allocated two registers fewer than before, and the pre-existing symbols keep their figures)
    auto split4 = [&](const float4& v, bool ok, bf16x4& h1, bf16x4& h2, bf16x4& h3) {
        bf16x4 h[NP];
        tl_split4<NP>(ok ? v : make_float4(0.f, 0.f, 0.f, 0.f), h);
        h1 = h[0];
        if constexpr (NP > 1) h2 = h[1];
        if constexpr (NP > 2) h3 = h[2];
    };

    // prologue: indices of step 0 -> LDS -> rows of step 0 in flight, indices of step 1 in registers
    int ireg = load_idx(p0);
    if (tid < 64) idxbuf[tid >> 5][tid & 31] = ireg;
    __syncthreads();
    bool ok_a[MB], ok_g[NB];
    auto valid_now = [&]() {
#pragma unroll
        for (int j = 0; j < MB; ++j) ok_a[j] = idxbuf[0][ar[j]] >= 0 && a0 + ac[j] < ca;
#pragma unroll
        for (int j = 0; j < NB; ++j) ok_g[j] = idxbuf[1][gr[j]] >= 0 && g0 + gc[j] < cg;
    };
    valid_now();
    fetch(0);
    ireg = load_idx(p0 + pstep);

    for (int p = p0; p < p1; p += pstep) {
        // ---- split the rows of this step (registers)
        bf16x4 a1[MB], a2[MB], a3[MB], g1[NB], g2[NB], g3[NB];   // (pieces past NP: never written, never read)
#pragma unroll
        for (int j = 0; j < MB; ++j) split4(pa[j], ok_a[j], a1[j], a2[j], a3[j]);
#pragma unroll
        for (int j = 0; j < NB; ++j) split4(pg[j], ok_g[j], g1[j], g2[j], g3[j]);
        __syncthreads();                                   // the previous step's fragments have been read
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            *reinterpret_cast<bf16x4*>(&Ap[0][ar[j]][ac[j]]) = a1[j];
            if constexpr (NP > 1) *reinterpret_cast<bf16x4*>(&Ap[1][ar[j]][ac[j]]) = a2[j];
            if constexpr (NP > 2) *reinterpret_cast<bf16x4*>(&Ap[2][ar[j]][ac[j]]) = a3[j];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            *reinterpret_cast<bf16x4*>(&Gp[0][gr[j]][gc[j]]) = g1[j];
            if constexpr (NP > 1) *reinterpret_cast<bf16x4*>(&Gp[1][gr[j]][gc[j]]) = g2[j];
            if constexpr (NP > 2) *reinterpret_cast<bf16x4*>(&Gp[2][gr[j]][gc[j]]) = g3[j];
        }
        if (tid < 64) idxbuf[tid >> 5][tid & 31] = ireg;  // indices of the next step
        __syncthreads();
        if (p + pstep < p1) {
            valid_now();
            fetch(0);                                      // rows of the next step: in flight during the MFMAs
            ireg = load_idx(p + 2 * pstep);
        }
        // ---- fragments by transpose reads: lane i of a 16-lane group points at (pair 8 g + (i >> 2), channels
        // 4 (i & 3) .. + 3) of a 16-channel block and receives channel i of pairs 8 g .. 8 g + 3 (then + 4)
        const int li = lane & 15, lg = lane >> 4;
        auto frag = [&](const __bf16* plane, int pitch, int c16) -> bf16x8 {
            const __bf16* q = plane + (8 * lg + (li >> 2)) * pitch + c16 + 4 * (li & 3);
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4*)(q));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4*)(q + 4 * pitch));
            union { s16x4 h[2]; bf16x8 v; } u;
            u.h[0] = lo; u.h[1] = hi;
            return u.v;
        };
        bf16x8 fa[MB][NP], fg[NB][NP];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) fa[i][pl] = frag(&Ap[pl][0][0], LDA, (wi * MB + i) * 16);
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) fg[j][pl] = frag(&Gp[pl][0][0], LDG, (wj * NB + j) * 16);
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                f32x4 t = acc[i][j];
                split_products<NP>([&](auto ap, auto gp) {
                    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][ap], fg[j][gp], t, 0, 0, 0);
                });
                acc[i][j] = t;
            }
    }

    // ---- partial[item][ca][cg]: C row = 4 (lane >> 4) + r (input channel), col = lane & 15 (output channel)
    float* d = partial + int64_t(blockIdx.y) * ca * cg;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int co = g0 + (wj * NB + j) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = a0 + (wi * MB + i) * 16 + 4 * (lane >> 4) + r;
                if (ci < ca && co < cg) d[int64_t(ci) * cg + co] = acc[i][j][r];
            }
        }
}
