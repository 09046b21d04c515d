// Text search over a bank of scenes on gfx950: per-point heat-maps for arbitrary queries and the k best points of every
// scene, for a bank of per-point fp16 features (the files run/evaluate.py:232-235,328-330 writes).
//
//   osn_bank_append   bank[row0 + i] = X[gather[i]].half()            (run/evaluate.py:290, the rows the query reads)
//   osn_bank_search   score(p, q) = run/evaluate.py:305,310 (normalize) or :291 (raw) on the stored fp16 row,
//                     heat [N, Q], and per (scene, query) the k best points / the points over a threshold.
//
// Pass 1 (heat_kernel) is the streaming pass: 128 bank rows per workgroup, fp16 rows go HBM -> registers -> LDS with no
// conversion, v_mfma_f32_32x32x16_f16 against the query chunk, fp32 accumulate.  The sum of squares of a row is taken
// from the very chunks that feed the MFMA (the bank is read once), the accumulator is divided by (norm + 1e-5) in fp32
// and rounded to fp16 once.  The scores leave through an LDS tile twice: row-major into the caller's `heat` (optional)
// and column-major into the workspace (`heatT` [Q][ldT]): a (scene, query) pair is then one contiguous fp16 array.
//
// What a score is held to (tests/search_bounds.py; on the device tests/test_gpu_search_bounds.py).  v = the stored row (fp16, or
// code * 2^e), S = sum v_k t_k, A = sum |v_k| |t_k|, N = sqrt(sum v_k^2) in float64; c = 2e-6, this project's bound for an
// fp32-accumulating MFMA contraction; DELTA = 1.4e-5, four times the measured error of fp32 sqrtf(sum v^2) + 1e-5f:
//   raw          fp16_rne(S - c A) <= score <= fp16_rne(S + c A)
//   normalize    fp16_rne(L) <= score <= fp16_rne(U): L, U = min, max of (S -+ c A) / ((N + 1e-5) (1 -+ DELTA)) over the signs
// ends rounded from float64 once.  A zero row scores +0.0 bit for bit; a NaN in a row makes every score of it NaN; an inf
// makes them NaN too (normalize, and any fp8 row: its codes are all NaN) or S itself (raw, fp16 rows).  fp16 subnormals count.
//
// Pass 2 selects on heatT with integer arithmetic only.  The fp16 score becomes a monotone 16-bit key (NaN -> 0, below
// -inf; -0 -> +0).  A two-round 8-bit radix select over per-(scene, query) 256-bin histograms (LDS per workgroup, integer
// atomics into the global one) finds the k-th key K exactly.  Everything above K is selected; of the points equal to K the
// lowest indices are: per-chunk counts of key == K give every chunk its rank offset, a block scan orders the chunk's own.
// A final rank-by-counting sort of the <= 128 candidates writes (score desc, index asc).  No floating-point atomics:
// results are bitwise repeatable.
//
// The fp8 bank (osn_bank_append_fp8 / osn_bank_search_fp8) stores a row as d OCP e4m3fn codes and one exponent byte e:
// value = code * 2^e, e the smallest integer >= -120 with max|x| * 2^-e <= 448.  The append is one wave per row (the
// row stays in registers between the max and the conversion); the heat pass streams 16 codes per 16-byte load, widens
// them to fp16 (exact) on the way into LDS (heat_fp8_kernel); 2^e enters where the scores leave: raw scores are acc * 2^e,
// normalised ones acc / (||c|| + 1e-5 / 2^e), which never forms a number of the row's own size (e goes up to 120).  The two
// heat kernels call one set of __device__ templates for the query staging, the MFMA loop, the row norms and the score
// output; each has its own row fetch, stash and stage loop.  Pass 2 and the entries' argument checks are shared too.
//
// Negative queries (osn_bank_search_contrast / _fp8): the heat kernels' CONTRAST instances walk the negatives' column groups
// first -- same loop, each score rounded to fp16, only the row's maximum kept (rneg, LDS) -- and then write, for the queries,
// fp16(1 / (1 + expf(-(s - rneg) / temperature))) in place of the fp16 score s.  Pass 2 selects on that relevancy unchanged.
#include <type_traits>

#include "bank.h"

namespace osn {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int S_BM = 128;          // bank rows per workgroup (4 waves x 32)
constexpr int S_DK = 128;          // feature chunk (halfs): 256 bytes of a row, 32 KB per workgroup in flight
constexpr int S_LD = S_DK + 8;     // padded LDS row (272 B: 16-byte aligned, conflict-free 16-byte reads)
static_assert(S_LD >= S_BM + 8, "the score tile [column][row] reuses the row tile");
enum { ENS_NONE = 0, ENS_VOCABULARY = 1, ENS_QUERY = 2 };  // two banks searched as one (osn_bank_search_ensemble): mode + 1

constexpr int SEL_T = 256;         // threads of a select workgroup
constexpr int SEL_IT = 2;          // 8 scores per thread and iteration
constexpr int SEL_R = SEL_T * 8 * SEL_IT;   // rows of a chunk (4096)
constexpr int SEL_ST = 16;         // uint32 words of per-(scene, query) select state
constexpr uint32_t SEL_NONE = 0x10000u;     // K of an empty selection (above every key)
enum { ST_KK = 0, ST_B1, ST_ABOVE, ST_K, ST_GT, ST_NEED_EQ, ST_EQ_TOTAL, ST_SLOT_GT, ST_SLOT_EQ };

// ------------------------------------------------------------------------------------------------------ append
__global__ __launch_bounds__(256) void bank_append_kernel(const float* __restrict__ X, int64_t n_rows, const int64_t* __restrict__ g,
                                                          int64_t n, int d4, _Float16* __restrict__ out, int32_t* __restrict__ err) {
    const int64_t total = n * d4;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int64_t p = e / d4;
        const int c = int(e - p * d4);
        const int64_t r = g ? g[p] : p;
        if (r < 0 || r >= n_rows) {                          // nothing is read or written for this row
            if (c == 0) atomicOr(err, BANK_E_GATHER);
            continue;
        }
        const float4 v = *reinterpret_cast<const float4*>(X + (r * d4 + c) * 4);
        half4 h;
        h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
        *reinterpret_cast<half4*>(out + (p * d4 + c) * 4) = h;
    }
}

// ------------------------------------------------------------------------------------------------------ pass 1
// What heat_kernel and heat_fp8_kernel share: the query chunk's way into registers and LDS, the MFMAs of one chunk, the
// row norms and the way the scores leave.  Each kernel keeps its own row fetch and stash, lane-to-row mapping and stage loop.

// query chunk [d0, d0 + S_DK) of the column group at cg0 -> registers.  All loads unconditional from clamped addresses
// (query.hip: a conditional fetch makes the compiler drain the memory counter before every stash)
template <int CT>
__device__ __forceinline__ void fetch_queries(uint4 (&pt)[2 * CT], const _Float16* __restrict__ T, int cg0, int d0, int d, int q,
                                              int tid) {
#pragma unroll
    for (int j = 0; j < 2 * CT; ++j) {
        const int f = tid + 256 * j;
        const int trow = f >> 4, ch = f & 15;
        const int col = cg0 + trow;
        const bool ok = col < q && d0 + ch * 8 < d;
        pt[j] = *reinterpret_cast<const uint4*>(ok ? T + int64_t(col) * d + d0 + ch * 8 : T);
    }
}

template <int CT>
__device__ __forceinline__ void stash_queries(_Float16 (*Ts)[S_LD], const uint4 (&pt)[2 * CT], int cg0, int d0, int d, int q,
                                              int tid) {
#pragma unroll
    for (int j = 0; j < 2 * CT; ++j) {
        const int f = tid + 256 * j;
        const int trow = f >> 4, ch = f & 15;
        const bool ok = cg0 + trow < q && d0 + ch * 8 < d;
        uint4 v = pt[j];
        if (!ok) v = make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4*>(&Ts[trow][ch * 8]) = v;
    }
}

// the MFMAs of one chunk: fragments of k-step ks + 1 are read from LDS while the MFMAs of k-step ks run (two register sets,
// as query.hip)
template <int CT>
__device__ __forceinline__ void mfma_chunk(f32x16 (&acc)[CT], const _Float16 (*Xs)[S_LD], const _Float16 (*Ts)[S_LD], int wave,
                                           int lane) {
    const int arow = wave * 32 + (lane & 31);
    const int kh = 8 * (lane >> 5);
    half8 fa[2], fb[2][CT];
    auto frags = [&](int ks, int w) {
        fa[w] = *reinterpret_cast<const half8*>(&Xs[arow][ks * 16 + kh]);
#pragma unroll
        for (int t = 0; t < CT; ++t)
            fb[w][t] = *reinterpret_cast<const half8*>(&Ts[t * 32 + (lane & 31)][ks * 16 + kh]);
    };
    frags(0, 0);
#pragma unroll
    for (int ks = 0; ks < S_DK / 16; ++ks) {
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 1 < S_DK / 16) frags(ks + 1, (ks + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < CT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks & 1], fb[ks & 1][t], acc[t], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// rden[row] = ||row|| + 1e-5 [/ rscale[row]] (run/evaluate.py:305) from the partial sums of squares of the LANES lanes that
// share a row (lane tid % LANES of row ps * (256 / LANES) + tid / LANES).  SCALED (code rows, value = code * 2^e): the
// denominator ||c|| 2^e + 1e-5 with 2^e divided out, so that nothing of the size of the row's values is ever formed in fp32:
// ||c|| 2^e passes 2^128 from e = 115 on at d = 768.  1e-5 / 2^e is exact (a subnormal from e = 110 on, next to ||c|| >= 224).
// rscale[row] becomes 1 on the way: the normalised scores leave as acc * 1 / rden through the very code the raw ones take
template <int LANES, bool SCALED>
__device__ __forceinline__ void row_norms(float* rden, const float (&ss)[S_BM * LANES / 256], float* rscale, int tid) {
    constexpr int SWEEP = 256 / LANES;
#pragma unroll
    for (int ps = 0; ps < S_BM / SWEEP; ++ps) {
        float s = ss[ps];
#pragma unroll
        for (int m = 1; m < LANES; m <<= 1) s += __shfl_xor(s, m, 64);
        const int row = ps * SWEEP + tid / LANES;
        if (tid % LANES == 0) {
            if constexpr (SCALED) {
                rden[row] = sqrtf(s) + 1e-5f / rscale[row];
                rscale[row] = 1.f;
            } else {
                rden[row] = sqrtf(s) + 1e-5f;
            }
        }
    }
    __syncthreads();
}

// the scores of one column group leave: accumulator [* rscale, exact: 2^e for raw scores, 1 for normalised ones (row_norms)],
// divided by rden in fp32, rounded to fp16 once into the LDS tile Sc[column][row] (CT * 32 <= 128 rows of the row tile); from
// there column-major into heatT and, where the caller wants it, row-major into heat.
// CONTRAST (osn_bank_search_contrast): a group of negatives (`neg`, q = their number) is stored nowhere -- the largest fp16
// score of a row, NaN if one of them is, is kept in rneg[row]; a group of queries writes, in place of the fp16 score s,
// fp16(1 / (1 + expf(-(s - rneg[row]) / temperature))), the relevancy against the best negative.
// ENS_VOCABULARY: the pick's two walks over the queries are such maxima groups (neg, rneg = the source's row maxima), with or
// without CONTRAST.  ENS_QUERY: a group of queries runs twice; side 0 (source A) keeps its fp16 values in `held` and writes
// nothing, side 1 (source B) writes the larger of the two where A < B (IEEE), A's otherwise, and the choice into `source`
// (nullable, [n, q] bytes).
template <int CT, bool SCALED, bool CONTRAST, int ENS = ENS_NONE>
__device__ __forceinline__ void scores_out(const f32x16 (&acc)[CT], _Float16 (*Sc)[S_LD], const float* rden, const float* rscale,
                                           float* rneg, bool neg, float temperature, _Float16* __restrict__ heat,
                                           _Float16* __restrict__ heatT, int64_t ldT, int64_t row0, int64_t n, int q, int cg0,
                                           int normalize, int tid, int side = 0, half2 (*held)[8] = nullptr,
                                           uint8_t* __restrict__ source = nullptr) {
    const int lane = tid & 63, wave = tid >> 6;
    constexpr bool MAXIMA = CONTRAST || ENS == ENS_VOCABULARY;      // groups that leave a row maximum and nothing else exist
#pragma unroll
    for (int t = 0; t < CT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            float v = acc[t][r];
            if (SCALED) v *= rscale[lrow];
            if (normalize) v /= rden[lrow];
            _Float16 h = (_Float16)v;
            if (CONTRAST && !neg) {
                const float z = ((float)h - rneg[lrow]) / temperature;
                h = (_Float16)(1.0f / (1.0f + expf(-z)));
            }
            if constexpr (ENS == ENS_QUERY) {
                if (!neg) {
                    if (side == 0) {                        // (uniform) A's value waits in registers for B's
                        held[t][r >> 1][r & 1] = h;
                        continue;
                    }
                    const _Float16 a = held[t][r >> 1][r & 1];
                    const bool from_b = (float)a < (float)h;        // IEEE: a tie, -0 against +0, a NaN on either side -> A
                    h = from_b ? h : a;
                    const int64_t row = row0 + lrow;
                    const int col = cg0 + t * 32 + (lane & 31);
                    if (source && row < n && col < q) source[row * q + col] = from_b ? 1 : 0;
                }
            }
            Sc[t * 32 + (lane & 31)][lrow] = h;
        }
    }
    if constexpr (ENS == ENS_QUERY) {
        if (!neg && side == 0) return;                      // nothing was written to the tile
    }
    __syncthreads();
    if (MAXIMA && neg) {                                    // (uniform over the workgroup)
        if (tid < S_BM) {
            const int qn = (q - cg0) < 32 * CT ? (q - cg0) : 32 * CT;
            float nm = rneg[tid];
            for (int c = 0; c < qn; ++c) {
                const float v = (float)Sc[c][tid];
                nm = (v > nm || v != v) ? v : nm;           // a NaN stays
            }
            rneg[tid] = nm;
        }
        __syncthreads();                                    // the tile is the next column group's row buffer
        return;
    }
    for (int e = tid; e < CT * 32 * (S_BM / 8); e += 256) {       // column-major: 16-byte pieces of a column's 128 rows
        const int col = e >> 4, v8 = e & 15;
        const int gc = cg0 + col;
        if (gc >= q) continue;
        const int64_t r = row0 + 8 * v8;
        _Float16* dst = heatT + int64_t(gc) * ldT + r;
        if (r + 8 <= n) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&Sc[col][8 * v8]);
        } else {
            for (int j = 0; j < 8; ++j)
                if (r + j < n) dst[j] = Sc[col][8 * v8 + j];
        }
    }
    if (heat) {
        const int qn = (q - cg0) < 32 * CT ? (q - cg0) : 32 * CT;
        for (int e = tid; e < S_BM * qn; e += 256) {
            const int r = e / qn, c = e - r * qn;
            if (row0 + r < n) heat[(row0 + r) * q + cg0 + c] = Sc[c][r];
        }
    }
    __syncthreads();                                        // the tile is the next column group's row buffer
}

// The column groups in the order a heat kernel walks them: the queries' groups from cg = 0; with CONTRAST the negatives'
// groups (Tn [m, d]) come first, from cg < 0.  The row norms are taken during the first group walked, whichever that is.
template <int CT, bool CONTRAST>
struct ColumnGroups {
    int first;             // cg of the first group: -(groups of negatives) * 32 * CT, or 0
    __device__ __forceinline__ explicit ColumnGroups(int m) : first(CONTRAST ? -((m + 32 * CT - 1) / (32 * CT)) * (32 * CT) : 0) {}
    __device__ __forceinline__ bool neg(int cg) const { return CONTRAST && cg < 0; }
    __device__ __forceinline__ int col0(int cg) const { return neg(cg) ? cg - first : cg; }       // first column inside its matrix
};

// Two banks as one (ENS, osn_bank_search_ensemble): B2 holds the second source's rows; bit ps of `from2` sends the fetch of this
// thread's row ps of a sweep to B2.  A walk is one column group over the workgroup's rows, the plain kernel's loop body.
//   ENS_VOCABULARY  the queries' groups over A, then over B, normalised, each keeping only the row maxima (rneg, rneg2), as the
//                   negatives of CONTRAST do; source(row) = max A < max B goes to LDS (over rneg2) and to `source`; then the plain
//                   kernel's walks, every row fetched from its chosen source, the sum of squares taken again on the way (the same
//                   chunks in the same order: the chosen source's denominator, bit for bit).  LDS: 512 bytes more than CONTRAST.
//   ENS_QUERY       A's negatives (rneg) and first group of queries, then B's (rneg2), then every further group over A and over B;
//                   A's fp16 values of a group wait in registers for B's (scores_out), across B's negatives for the first group.
//                   Denominators of both sources stay in LDS (rden, rden2).
template <int CT, int WGS, bool CONTRAST, int ENS = ENS_NONE>
__global__ __launch_bounds__(256, WGS) void heat_kernel(const _Float16* __restrict__ B, const _Float16* __restrict__ T,
                                                        _Float16* __restrict__ heat, _Float16* __restrict__ heatT, int64_t ldT,
                                                        int64_t n, int d, int q, int normalize, const _Float16* __restrict__ Tn,
                                                        int m, float temperature, const _Float16* __restrict__ B2,
                                                        uint8_t* __restrict__ source) {
    __shared__ __attribute__((aligned(16))) _Float16 Xs[S_BM][S_LD];
    __shared__ __attribute__((aligned(16))) _Float16 Ts[CT * 32][S_LD];
    __shared__ float rden[S_BM];
    __shared__ float rneg[S_BM];                            // CONTRAST: the row's best negative score
    __shared__ float rden2[S_BM];                           // ENS_QUERY: B's denominators
    __shared__ float rneg2[S_BM];                           // ENS: B's row maxima, then the pick | B's best negative score

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = int64_t(blockIdx.x) * S_BM;
    const int xq = tid & 15, xr = tid >> 4;                 // 16 lanes x 16 bytes = one row's 256-byte chunk; 16 rows per sweep
    float ss[S_BM / 16];
#pragma unroll
    for (int ps = 0; ps < S_BM / 16; ++ps) ss[ps] = 0.f;
    if (CONTRAST && tid < S_BM) rneg[tid] = -INFINITY;      // (read after the barriers of the first group)
    uint32_t from2 = 0;
    half2 held[ENS == ENS_QUERY ? CT : 1][8];

    // one column group: columns cg0 .. of Tg [qg, d]; sumsq: the row norms are taken on the way, into den
    auto walk = [&](const _Float16* __restrict__ Tg, int qg, int cg0, bool neg, bool sumsq, int nrm, float* den, float* rn,
                    int side) {
        f32x16 acc[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        if constexpr (ENS != ENS_NONE) {
            if (sumsq) {
#pragma unroll
                for (int ps = 0; ps < S_BM / 16; ++ps) ss[ps] = 0.f;
            }
        }
        // one chunk in flight in registers while the MFMAs of the previous one run from LDS (rows fetched as the queries are)
        uint4 px[S_BM / 16];
        uint4 pt[2 * CT];
        auto fetch = [&](int d0) {
            fetch_queries<CT>(pt, Tg, cg0, d0, d, qg, tid);
#pragma unroll
            for (int ps = 0; ps < S_BM / 16; ++ps) {
                const int64_t row = row0 + ps * 16 + xr;
                const bool ok = row < n && d0 + xq * 8 < d;
                const _Float16* __restrict__ Bs = B;
                if constexpr (ENS != ENS_NONE) Bs = (from2 >> ps) & 1u ? B2 : B;
                px[ps] = *reinterpret_cast<const uint4*>(ok ? Bs + row * d + d0 + xq * 8 : B);
            }
        };
        auto stash = [&](int d0) {
#pragma unroll
            for (int ps = 0; ps < S_BM / 16; ++ps) {
                const int row = ps * 16 + xr;
                const bool ok = row0 + row < n && d0 + xq * 8 < d;
                uint4 v = px[ps];
                if (!ok) v = make_uint4(0, 0, 0, 0);
                if (sumsq) {
                    const half8 h = __builtin_bit_cast(half8, v);
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) s += (float)h[k] * (float)h[k];
                    ss[ps] += s;
                }
                *reinterpret_cast<uint4*>(&Xs[row][xq * 8]) = v;
            }
            stash_queries<CT>(Ts, pt, cg0, d0, d, qg, tid);
        };
        fetch(0);
        stash(0);
        __syncthreads();
        for (int d0 = 0; d0 < d; d0 += S_DK) {
            __builtin_amdgcn_sched_barrier(0);
            fetch(d0 + S_DK);                               // (past the end: the first 16 bytes of B / T, never staged)
            __builtin_amdgcn_sched_barrier(0);
            mfma_chunk<CT>(acc, Xs, Ts, wave, lane);
            __syncthreads();
            if (d0 + S_DK < d) stash(d0 + S_DK);
            __syncthreads();
        }
        if (sumsq) row_norms<16, false>(den, ss, nullptr, tid);
        scores_out<CT, false, CONTRAST, ENS>(acc, Xs, den, nullptr, rn, neg, temperature, heat, heatT, ldT, row0, n, qg, cg0, nrm,
                                             tid, side, held, source);
    };

    const ColumnGroups<CT, CONTRAST> groups(m);
    if constexpr (ENS == ENS_VOCABULARY) {
        for (int side = 0; side < 2; ++side) {
            float* rmax = side ? rneg2 : rneg;
            from2 = side ? ~0u : 0u;
            if (tid < S_BM) rmax[tid] = -INFINITY;          // (read after the barriers of the first group)
            for (int cg = 0; cg < q; cg += 32 * CT) walk(T, q, cg, true, cg == 0, 1, rden, rmax, 0);
        }
        if (tid < S_BM) {                                   // (the last walk ended with a barrier)
            const bool from_b = rneg[tid] < rneg2[tid];     // IEEE: a tie or a NaN on either side -> A
            if (row0 + tid < n) source[row0 + tid] = from_b ? 1 : 0;
            rneg2[tid] = from_b ? 1.f : 0.f;
            if (CONTRAST) rneg[tid] = -INFINITY;
        }
        __syncthreads();
        from2 = 0;
#pragma unroll
        for (int ps = 0; ps < S_BM / 16; ++ps) from2 |= (rneg2[ps * 16 + xr] != 0.f ? 1u : 0u) << ps;
    }
    if constexpr (ENS == ENS_QUERY) {
        if (CONTRAST && tid < S_BM) rneg2[tid] = -INFINITY;
        // a source's negatives and its first group of queries back to back (its rows are still in cache), then the further groups
        for (int side = 0; side < 2; ++side) {
            from2 = side ? ~0u : 0u;
            for (int cg = groups.first; cg <= 0; cg += 32 * CT) {
                const bool neg = groups.neg(cg);
                walk(neg ? Tn : T, neg ? m : q, groups.col0(cg), neg, normalize && cg == groups.first, normalize,
                     side ? rden2 : rden, side ? rneg2 : rneg, side);
            }
        }
        for (int cg = 32 * CT; cg < q; cg += 32 * CT) {
            for (int side = 0; side < 2; ++side) {
                from2 = side ? ~0u : 0u;
                walk(T, q, cg, false, false, normalize, side ? rden2 : rden, side ? rneg2 : rneg, side);
            }
        }
    } else {
        for (int cg = groups.first; cg < q; cg += 32 * CT) {
            const bool neg = groups.neg(cg);
            walk(neg ? Tn : T, neg ? m : q, groups.col0(cg), neg, normalize && cg == groups.first, normalize, rden, rneg, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ fp8 bank
constexpr int Q8_RG = 2;           // 16-element groups of a row a lane keeps in registers: rows up to 64 * 16 * Q8_RG = 2048
                                   // wide are read from HBM once, wider rows read their tail twice (max, then conversion)

template <bool F16>
__device__ inline void q8_load(const void* __restrict__ X, int64_t at, float (&v)[16]) {
    if (F16) {
        const uint4* p = reinterpret_cast<const uint4*>(static_cast<const _Float16*>(X) + at);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const half8 h = __builtin_bit_cast(half8, p[j]);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[8 * j + k] = (float)h[k];
        }
    } else {
        const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(X) + at);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 f = p[j];
            v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w;
        }
    }
}

__device__ inline uint32_t q8_absmax(const float (&v)[16], uint32_t m) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {                          // |x| as bits: orders as the value does, inf and NaN on top
        const uint32_t b = __float_as_uint(v[k]) & 0x7FFFFFFFu;
        m = b > m ? b : m;
    }
    return m;
}

// 16 values * 2^-e -> 16 e4m3fn codes (v_cvt_pk_fp8_f32: round to nearest even, never saturating here: |v * s| <= 448)
__device__ inline uint4 q8_codes(const float (&v)[16], float s, bool bad) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c = 0;
        c = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j] * s, v[4 * j + 1] * s, c, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j + 2] * s, v[4 * j + 3] * s, c, true);
        w[j] = bad ? 0x7F7F7F7Fu : uint32_t(c);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// one wave per row: lane l holds the 16-element groups l, l + 64, ... of the row; ng = d / 16 groups
template <bool F16>
__global__ __launch_bounds__(256) void bank_append_fp8_kernel(const void* __restrict__ X, int64_t n_rows, const int64_t* __restrict__ g,
                                                              int64_t n, int ng, uint8_t* __restrict__ codes, int8_t* __restrict__ exps,
                                                              int32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t d = int64_t(ng) * 16;
    for (int64_t p = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); p < n; p += int64_t(gridDim.x) * 4) {
        const int64_t r = g ? g[p] : p;
        if (r < 0 || r >= n_rows) {                          // (the whole wave) nothing is read or written for this row
            if (lane == 0) atomicOr(err, BANK_E_GATHER);
            continue;
        }
        float v[Q8_RG][16];
        uint32_t amax = 0;
#pragma unroll
        for (int j = 0; j < Q8_RG; ++j) {
            const int grp = lane + 64 * j;
            if (grp < ng) {
                q8_load<F16>(X, r * d + grp * 16, v[j]);
                amax = q8_absmax(v[j], amax);
            }
        }
        for (int grp = lane + 64 * Q8_RG; grp < ng; grp += 64) {
            float t[16];
            q8_load<F16>(X, r * d + grp * 16, t);
            amax = q8_absmax(t, amax);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t o = __shfl_xor(amax, m, 64);
            amax = o > amax ? o : amax;
        }
        // amax = 1.M * 2^(E - 127) = m * 2^x with m = 1.M / 2 in [0.5, 1), x = E - 126: e = x - 9 if m <= 0.875, else x - 8
        const bool bad = amax >= 0x7F800000u;
        const int E = int(amax >> 23);
        int e = E - 135 + ((amax & 0x7FFFFFu) > 0x600000u ? 1 : 0);
        if (E == 0 || e < -120) e = -120;                    // (a float32 subnormal maximum lies below 448 * 2^-120)
        if (amax == 0 || bad) e = 0;
        const float s = __uint_as_float(uint32_t(127 - e) << 23);          // 2^-e, exact: 7 <= 127 - e <= 247
#pragma unroll
        for (int j = 0; j < Q8_RG; ++j) {
            const int grp = lane + 64 * j;
            if (grp < ng) *reinterpret_cast<uint4*>(codes + p * d + grp * 16) = q8_codes(v[j], s, bad);
        }
        for (int grp = lane + 64 * Q8_RG; grp < ng; grp += 64) {
            float t[16];
            q8_load<F16>(X, r * d + grp * 16, t);
            *reinterpret_cast<uint4*>(codes + p * d + grp * 16) = q8_codes(t, s, bad);
        }
        if (lane == 0) exps[p] = int8_t(e);
    }
}

// pass 1 over code rows.  A chunk is 128 features = 128 bytes of a row (8 lanes x 16 bytes, 32 rows per sweep); TWO code
// chunks are in flight in registers, so a workgroup has the 32 KB outstanding that heat_kernel has with its one 256-byte
// chunk (the query chunk, an L2 hit, stays one ahead).
// Two workgroups per CU: the second register stage and the conversion need 194 / 250 VGPRs (one / two column tiles); held to
// the 168 of three workgroups the kernel spills inside the loop and measured 0.81x of the fp16 pass at 8 x 150 k x 768 x 32
// where this shape measured 0.67x.
// ENS: as heat_kernel; the second source is (B2, E2).  ENS_VOCABULARY loads rscale anew for each of its three parts (row_norms
// leaves 1 there), the last from the exponent of each row's chosen source; ENS_QUERY keeps rscale2 / rden2 for B.
template <int CT, int WGS, bool CONTRAST, int ENS = ENS_NONE>
__global__ __launch_bounds__(256, WGS) void heat_fp8_kernel(const uint8_t* __restrict__ B, const int8_t* __restrict__ E,
                                                            const _Float16* __restrict__ T, _Float16* __restrict__ heat,
                                                            _Float16* __restrict__ heatT, int64_t ldT, int64_t n, int d, int q,
                                                            int normalize, const _Float16* __restrict__ Tn, int m,
                                                            float temperature, const uint8_t* __restrict__ B2,
                                                            const int8_t* __restrict__ E2, uint8_t* __restrict__ source) {
    __shared__ __attribute__((aligned(16))) _Float16 Xs[S_BM][S_LD];
    __shared__ __attribute__((aligned(16))) _Float16 Ts[CT * 32][S_LD];
    __shared__ float rden[S_BM];
    __shared__ float rscale[S_BM];                          // 2^e of the row
    __shared__ float rneg[S_BM];                            // CONTRAST: the row's best negative score
    __shared__ float rden2[S_BM];                           // ENS_QUERY: B's denominators
    __shared__ float rscale2[S_BM];                         // ENS_QUERY: B's 2^e
    __shared__ float rneg2[S_BM];                           // ENS: B's row maxima, then the pick | B's best negative score

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = int64_t(blockIdx.x) * S_BM;
    const int xq = tid & 7, xr = tid >> 3;                  // 8 lanes x 16 codes = one row's 128-byte chunk; 32 rows per sweep
    constexpr int NPS = S_BM / 32;
    float ss[NPS];
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) ss[ps] = 0.f;
    if (tid < S_BM) {
        const int64_t row = row0 + tid < n ? row0 + tid : n - 1;
        rscale[tid] = __uint_as_float(uint32_t(127 + int(E[row])) << 23);
        if (ENS == ENS_QUERY) rscale2[tid] = __uint_as_float(uint32_t(127 + int(E2[row])) << 23);
        if (CONTRAST) rneg[tid] = -INFINITY;
    }
    uint32_t from2 = 0;
    half2 held[ENS == ENS_QUERY ? CT : 1][8];

    // one column group: columns cg0 .. of Tg [qg, d]; sumsq: the row norms are taken on the way, into den (and rs becomes 1)
    auto walk = [&](const _Float16* __restrict__ Tg, int qg, int cg0, bool neg, bool sumsq, int nrm, float* den, float* rs,
                    float* rn, int side) {
        f32x16 acc[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        if constexpr (ENS != ENS_NONE) {
            if (sumsq) {
#pragma unroll
                for (int ps = 0; ps < NPS; ++ps) ss[ps] = 0.f;
            }
        }
        uint4 pxa[NPS], pxb[NPS];                           // code chunks c + 1 and c + 2 while the MFMAs of chunk c run
        uint4 pt[2 * CT];                                   // the query chunk c + 1 (from L2)
        auto fetch_x = [&](uint4(&px)[NPS], int d0) {       // (unconditional from clamped addresses, as the queries)
#pragma unroll
            for (int ps = 0; ps < NPS; ++ps) {
                const int64_t row = row0 + ps * 32 + xr;
                const bool ok = row < n && d0 + xq * 16 < d;
                const uint8_t* __restrict__ Bs = B;
                if constexpr (ENS != ENS_NONE) Bs = (from2 >> ps) & 1u ? B2 : B;
                px[ps] = *reinterpret_cast<const uint4*>(ok ? Bs + row * d + d0 + xq * 16 : B);
            }
        };
        auto stash = [&](const uint4(&px)[NPS], int d0) {
#pragma unroll
            for (int ps = 0; ps < NPS; ++ps) {
                const int row = ps * 32 + xr;
                const bool ok = row0 + row < n && d0 + xq * 16 < d;
                uint4 v = px[ps];
                if (!ok) v = make_uint4(0, 0, 0, 0);
                half2 h[8];
                q8_widen(v, h);                             // e4m3 -> fp16, exact (bank.h)
                if (sumsq) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) s = __builtin_amdgcn_fdot2(h[j], h[j], s, false);
                    ss[ps] += s;
                }
                uint4 lo, hi;
                lo.x = __builtin_bit_cast(uint32_t, h[0]); lo.y = __builtin_bit_cast(uint32_t, h[1]);
                lo.z = __builtin_bit_cast(uint32_t, h[2]); lo.w = __builtin_bit_cast(uint32_t, h[3]);
                hi.x = __builtin_bit_cast(uint32_t, h[4]); hi.y = __builtin_bit_cast(uint32_t, h[5]);
                hi.z = __builtin_bit_cast(uint32_t, h[6]); hi.w = __builtin_bit_cast(uint32_t, h[7]);
                *reinterpret_cast<uint4*>(&Xs[row][xq * 16]) = lo;
                *reinterpret_cast<uint4*>(&Xs[row][xq * 16 + 8]) = hi;
            }
            stash_queries<CT>(Ts, pt, cg0, d0, d, qg, tid);
        };
        fetch_queries<CT>(pt, Tg, cg0, 0, d, qg, tid);
        fetch_x(pxa, 0);
        fetch_x(pxb, S_DK);                                 // (past the end: the first 16 bytes of B / T, never staged)
        stash(pxa, 0);
        __syncthreads();
        for (int d0 = 0; d0 < d; d0 += 2 * S_DK) {
            __builtin_amdgcn_sched_barrier(0);
            fetch_queries<CT>(pt, Tg, cg0, d0 + S_DK, d, qg, tid);
            fetch_x(pxa, d0 + 2 * S_DK);
            __builtin_amdgcn_sched_barrier(0);
            mfma_chunk<CT>(acc, Xs, Ts, wave, lane);
            __syncthreads();
            if (d0 + S_DK >= d) break;
            stash(pxb, d0 + S_DK);
            __syncthreads();
            __builtin_amdgcn_sched_barrier(0);
            fetch_queries<CT>(pt, Tg, cg0, d0 + 2 * S_DK, d, qg, tid);
            fetch_x(pxb, d0 + 3 * S_DK);
            __builtin_amdgcn_sched_barrier(0);
            mfma_chunk<CT>(acc, Xs, Ts, wave, lane);
            __syncthreads();
            if (d0 + 2 * S_DK < d) stash(pxa, d0 + 2 * S_DK);
            __syncthreads();
        }
        if (sumsq) row_norms<8, true>(den, ss, rs, tid);            // ||c|| + 1e-5 / 2^e
        scores_out<CT, true, CONTRAST, ENS>(acc, Xs, den, rs, rn, neg, temperature, heat, heatT, ldT, row0, n, qg, cg0, nrm, tid,
                                            side, held, source);
    };

    const ColumnGroups<CT, CONTRAST> groups(m);
    if constexpr (ENS == ENS_VOCABULARY) {
        const int64_t erow = row0 + tid < n ? row0 + tid : n - 1;          // (tid < S_BM)
        for (int side = 0; side < 2; ++side) {
            float* rmax = side ? rneg2 : rneg;
            from2 = side ? ~0u : 0u;
            if (tid < S_BM) {                               // (read after the barriers of the first group)
                rmax[tid] = -INFINITY;
                if (side) rscale[tid] = __uint_as_float(uint32_t(127 + int(E2[erow])) << 23);
            }
            for (int cg = 0; cg < q; cg += 32 * CT) walk(T, q, cg, true, cg == 0, 1, rden, rscale, rmax, 0);
        }
        if (tid < S_BM) {                                   // (the last walk ended with a barrier)
            const bool from_b = rneg[tid] < rneg2[tid];     // IEEE: a tie or a NaN on either side -> A
            if (row0 + tid < n) source[row0 + tid] = from_b ? 1 : 0;
            rneg2[tid] = from_b ? 1.f : 0.f;
            rscale[tid] = __uint_as_float(uint32_t(127 + int(from_b ? E2[erow] : E[erow])) << 23);
            if (CONTRAST) rneg[tid] = -INFINITY;
        }
        __syncthreads();
        from2 = 0;
#pragma unroll
        for (int ps = 0; ps < NPS; ++ps) from2 |= (rneg2[ps * 32 + xr] != 0.f ? 1u : 0u) << ps;
    }
    if constexpr (ENS == ENS_QUERY) {
        if (CONTRAST && tid < S_BM) rneg2[tid] = -INFINITY;
        // a source's negatives and its first group of queries back to back (its rows are still in cache), then the further groups
        for (int side = 0; side < 2; ++side) {
            from2 = side ? ~0u : 0u;
            for (int cg = groups.first; cg <= 0; cg += 32 * CT) {
                const bool neg = groups.neg(cg);
                walk(neg ? Tn : T, neg ? m : q, groups.col0(cg), neg, normalize && cg == groups.first, normalize,
                     side ? rden2 : rden, side ? rscale2 : rscale, side ? rneg2 : rneg, side);
            }
        }
        for (int cg = 32 * CT; cg < q; cg += 32 * CT) {
            for (int side = 0; side < 2; ++side) {
                from2 = side ? ~0u : 0u;
                walk(T, q, cg, false, false, normalize, side ? rden2 : rden, side ? rscale2 : rscale, side ? rneg2 : rneg, side);
            }
        }
    } else {
        for (int cg = groups.first; cg < q; cg += 32 * CT) {
            const bool neg = groups.neg(cg);
            walk(neg ? Tn : T, neg ? m : q, groups.col0(cg), neg, normalize && cg == groups.first, normalize, rden, rscale, rneg, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ pass 2
// monotone key of an fp16 score: NaN -> 0 (below -inf = 0x03FF), -0 -> +0 (equal values tie on the index, as a sort does)
__device__ inline uint32_t sel_key(uint16_t hb) {
    if ((hb & 0x7FFFu) > 0x7C00u) return 0u;
    if (hb == 0x8000u) hb = 0;
    return (hb & 0x8000u) ? (~uint32_t(hb) & 0xFFFFu) : (uint32_t(hb) | 0x8000u);
}

// element j of eight packed halfs, as bits (taken with shifts: a bit cast of a vector ELEMENT read element 0 for every j)
__device__ inline uint16_t half_bits(const uint4& v, int j) {
    const uint32_t w = j < 2 ? v.x : j < 4 ? v.y : j < 6 ? v.z : v.w;
    return uint16_t(w >> (16 * (j & 1)));
}

// rows of a scene, clamped so that nothing is read out of bounds whatever the offsets hold (search_check_kernel reports them)
struct SceneRange {
    int64_t o_s, o_e;      // global rows [o_s, o_e)
    int64_t g0, g1;        // this chunk's 8-aligned global rows [g0, g1)
};
__device__ inline SceneRange scene_range(const int64_t* __restrict__ off, int s, int64_t n, int64_t max_rows, int chunk) {
    SceneRange r;
    int64_t a = off[s], b = off[s + 1];
    a = a < 0 ? 0 : (a > n ? n : a);
    b = b < a ? a : (b > n ? n : b);
    if (b - a > max_rows) b = a + max_rows;
    r.o_s = a;
    r.o_e = b;
    const int64_t end8 = (b + 7) & ~int64_t(7);
    r.g0 = (a & ~int64_t(7)) + int64_t(chunk) * SEL_R;
    r.g1 = r.g0 + SEL_R < end8 ? r.g0 + SEL_R : end8;
    return r;
}

__global__ void search_check_kernel(const int64_t* __restrict__ off, int S, int64_t n, int64_t max_rows, int32_t* __restrict__ err) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int64_t a = off[s], b = off[s + 1];
    int e = 0;
    if (a < 0 || b < a || b > n || (s == 0 && a != 0)) e |= BANK_E_OFFSETS;
    else if (b - a > max_rows) e |= BANK_E_LONG;
    if (e) atomicOr(err, e);
}

__device__ inline uint32_t block_sum(uint32_t v, uint32_t* sh4) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}

// PASS 0: histogram of the key's high byte (and the threshold count); PASS 1: of the low byte among keys whose high byte is b1;
// PASS 2: the chunk's number of keys == K (only where the ties have to be ordered)
template <int PASS>
__global__ __launch_bounds__(SEL_T) void select_hist_kernel(const _Float16* __restrict__ heatT, int64_t ldT, const int64_t* __restrict__ off,
                                                            int64_t n, int64_t max_rows, int Q, int max_chunks,
                                                            const float* __restrict__ thr, unsigned long long* __restrict__ counts,
                                                            uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                            uint32_t* __restrict__ chunk_eq) {
    __shared__ uint32_t h[256];
    __shared__ uint32_t sh4[4];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x, s = blockIdx.y, q = blockIdx.z;
    const int64_t item = int64_t(s) * Q + q;
    const uint32_t* st = state + item * SEL_ST;
    uint32_t want = 0;
    if (PASS == 1) {
        if (st[ST_K] == SEL_NONE) return;
        want = st[ST_B1];
    }
    if (PASS == 2) {
        if (st[ST_K] == SEL_NONE || st[ST_EQ_TOTAL] == st[ST_NEED_EQ]) return;
        want = st[ST_K];
    }
    const SceneRange R = scene_range(off, s, n, max_rows, chunk);
    if (PASS != 2) {
        if (R.g0 >= R.g1) return;
        h[tid] = 0;
        __syncthreads();
    }
    const bool do_thr = PASS == 0 && thr != nullptr;
    const float th = do_thr ? thr[q] : 0.f;
    uint32_t cnt = 0;
    const _Float16* col = heatT + int64_t(q) * ldT;
    for (int it = 0; it < SEL_IT; ++it) {
        const int64_t g = R.g0 + (int64_t(it) * SEL_T + tid) * 8;
        if (g >= R.g1) continue;
        const uint4 v = *reinterpret_cast<const uint4*>(col + g);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t gi = g + j;
            if (gi < R.o_s || gi >= R.o_e) continue;
            const uint16_t hb = half_bits(v, j);
            const uint32_t key = sel_key(hb);
            if (PASS == 0) {
                atomicAdd(&h[key >> 8], 1u);
                if (do_thr && (float)__builtin_bit_cast(_Float16, hb) >= th) ++cnt;
            } else if (PASS == 1) {
                if ((key >> 8) == want) atomicAdd(&h[key & 255u], 1u);
            } else {
                if (key == want) ++cnt;
            }
        }
    }
    if (PASS != 2) {
        __syncthreads();
        if (h[tid]) atomicAdd(&hist[item * 256 + tid], h[tid]);
    }
    if (do_thr || PASS == 2) {
        const uint32_t tot = block_sum(cnt, sh4);
        if (tid == 0) {
            if (PASS == 2) chunk_eq[(int64_t(s) * max_chunks + chunk) * Q + q] = tot;
            else if (tot) atomicAdd(&counts[item], (unsigned long long)tot);
        }
    }
}

// one workgroup per (scene, query): the bin in which the kk-th largest key lies; the bins are zeroed for the next round
template <int PASS>
__global__ __launch_bounds__(256) void select_pick_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state, int k) {
    __shared__ uint32_t a[256];
    const int tid = threadIdx.x;
    const int64_t item = blockIdx.x;
    uint32_t* st = state + item * SEL_ST;
    if (PASS == 1 && st[ST_K] == SEL_NONE) return;
    const uint32_t own = hist[item * 256 + tid];
    hist[item * 256 + tid] = 0;
    a[tid] = own;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                     // suffix sums: a[t] = sum of the bins >= t
        const uint32_t v = a[tid] + (tid + o < 256 ? a[tid + o] : 0u);
        __syncthreads();
        a[tid] = v;
        __syncthreads();
    }
    const uint32_t total = a[0];
    if (PASS == 0) {
        const uint32_t kk = total < uint32_t(k) ? total : uint32_t(k);
        if (tid < SEL_ST) st[tid] = 0;
        __syncthreads();
        if (tid == 0) { st[ST_KK] = kk; if (kk == 0) st[ST_K] = SEL_NONE; }
        const uint32_t above = tid + 1 < 256 ? a[tid + 1] : 0u;
        if (kk > 0 && above < kk && kk <= a[tid]) { st[ST_B1] = uint32_t(tid); st[ST_ABOVE] = above; }
    } else {
        const uint32_t kk2 = st[ST_KK] - st[ST_ABOVE];      // 1 <= kk2 <= count of bin b1 = total
        const uint32_t above = tid + 1 < 256 ? a[tid + 1] : 0u;
        if (above < kk2 && kk2 <= a[tid]) {
            const uint32_t gt = st[ST_ABOVE] + above;
            st[ST_K] = (st[ST_B1] << 8) | uint32_t(tid);
            st[ST_GT] = gt;
            st[ST_NEED_EQ] = st[ST_KK] - gt;
            st[ST_EQ_TOTAL] = own;
        }
    }
}

// candidates: keys > K take the next free slot below count_gt (their order is settled by the final sort); keys == K take slot
// count_gt + rank, rank = their place among the scene's equal keys in index order, as long as rank < need_eq
__global__ __launch_bounds__(SEL_T) void select_collect_kernel(const _Float16* __restrict__ heatT, int64_t ldT, const int64_t* __restrict__ off,
                                                               int64_t n, int64_t max_rows, int Q, int max_chunks, int k,
                                                               uint32_t* __restrict__ state, const uint32_t* __restrict__ chunk_eq,
                                                               uint2* __restrict__ cand) {
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, s = blockIdx.y, q = blockIdx.z;
    const int64_t item = int64_t(s) * Q + q;
    uint32_t* st = state + item * SEL_ST;
    const uint32_t K = st[ST_K];
    if (K == SEL_NONE) return;
    const uint32_t count_gt = st[ST_GT], need_eq = st[ST_NEED_EQ];
    const bool ordered = st[ST_EQ_TOTAL] != need_eq;
    const SceneRange R = scene_range(off, s, n, max_rows, chunk);
    if (R.g0 >= R.g1) return;
    uint32_t run = 0;                                       // equal keys of the scene before this chunk / this sweep
    if (ordered)
        for (int c = 0; c < chunk; ++c) run += chunk_eq[(int64_t(s) * max_chunks + c) * Q + q];
    uint2* out = cand + item * k;
    const _Float16* col = heatT + int64_t(q) * ldT;
    for (int it = 0; it < SEL_IT; ++it) {
        const int64_t g = R.g0 + (int64_t(it) * SEL_T + tid) * 8;
        uint32_t keys[8];
        uint16_t bits[8];
        uint32_t neq = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { keys[j] = 0xFFFFFFFFu; bits[j] = 0; }
        if (g < R.g1) {
            const uint4 v = *reinterpret_cast<const uint4*>(col + g);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t gi = g + j;
                bits[j] = half_bits(v, j);
                const bool in = gi >= R.o_s && gi < R.o_e;
                keys[j] = in ? sel_key(bits[j]) : 0xFFFFFFFFu;               // (outside the scene: neither > K nor == K below)
                if (in && keys[j] > K) {
                    const uint32_t slot = atomicAdd(&st[ST_SLOT_GT], 1u);
                    if (slot < uint32_t(k)) out[slot] = make_uint2(bits[j], uint32_t(gi - R.o_s));
                }
                if (in && keys[j] == K) ++neq;
            }
        }
        if (!ordered) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (keys[j] == K) {
                    const uint32_t slot = count_gt + atomicAdd(&st[ST_SLOT_EQ], 1u);
                    if (slot < uint32_t(k)) out[slot] = make_uint2(bits[j], uint32_t(g + j - R.o_s));
                }
            continue;
        }
        if (run >= need_eq) continue;                       // (uniform over the workgroup; later sweeps still hold keys > K)
        // exclusive scan of neq over the workgroup's threads (thread order = row order)
        uint32_t inc = neq;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t o = __shfl_up(inc, m, 64);
            if (lane >= m) inc += o;
        }
        __syncthreads();
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t before = run;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        uint32_t rank = before + inc - neq;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (keys[j] == K) {
                if (rank < need_eq) out[count_gt + rank] = make_uint2(bits[j], uint32_t(g + j - R.o_s));
                ++rank;
            }
        run += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// one workgroup per (scene, query): rank the kk candidates by (key desc, index asc), pad with (-inf, -1)
__global__ __launch_bounds__(128) void select_sort_kernel(const uint32_t* __restrict__ state, const uint2* __restrict__ cand, int k,
                                                          _Float16* __restrict__ topk_scores, int64_t* __restrict__ topk_points) {
    __shared__ uint32_t skey[128], sidx[128];
    const int tid = threadIdx.x;
    const int64_t item = blockIdx.x;
    const uint32_t kk = state[item * SEL_ST + ST_KK];
    uint2 c = make_uint2(0, 0);
    if (uint32_t(tid) < kk) c = cand[item * k + tid];
    const uint32_t key = sel_key(uint16_t(c.x));
    skey[tid] = key;
    sidx[tid] = c.y;
    __syncthreads();
    if (uint32_t(tid) < kk) {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < kk; ++j) rank += (skey[j] > key || (skey[j] == key && sidx[j] < c.y)) ? 1u : 0u;
        topk_scores[item * k + rank] = __builtin_bit_cast(_Float16, uint16_t(c.x));
        topk_points[item * k + rank] = int64_t(c.y);
    } else if (tid < k) {
        topk_scores[item * k + tid] = __builtin_bit_cast(_Float16, uint16_t(0xFC00));
        topk_points[item * k + tid] = -1;
    }
}

static int sel_max_chunks(int64_t max_scene_rows) { return int(cdiv(max_scene_rows + 7, SEL_R)); }

struct SearchWs {
    size_t heatT, hist, state, chunk_eq, cand, total;
    int64_t ldT;
};
static SearchWs search_ws(int64_t n, int S, int Q, int k, int64_t max_scene_rows) {
    SearchWs w;
    const size_t items = size_t(S > 0 ? S : 0) * size_t(Q > 0 ? Q : 1);
    w.ldT = int64_t(align_up(size_t(n > 0 ? n : 1), 8));
    size_t o = 0;
    w.heatT = o; o += align_up(size_t(Q > 0 ? Q : 1) * size_t(w.ldT) * 2, 256);
    w.hist = o; o += align_up(items * 256 * 4, 256);
    w.state = o; o += align_up(items * SEL_ST * 4, 256);
    w.chunk_eq = o; o += align_up(items * size_t(sel_max_chunks(max_scene_rows > 0 ? max_scene_rows : 0)) * 4, 256);
    w.cand = o; o += align_up(items * size_t(k > 0 ? k : 1) * 8, 256);
    w.total = o;
    return w;
}

// pass 2 on the workspace's heatT (written by either heat kernel): the k best rows of every (scene, query), counts
static int select_pass(const SearchWs& w, char* p, int64_t n, const int64_t* scene_offsets, int n_scenes, int64_t max_scene_rows,
                       int q, int k, const float* thresholds, void* topk_scores_f16, int64_t* topk_points, int64_t* counts,
                       int32_t* err, hipStream_t st) {
    const _Float16* heatT = reinterpret_cast<const _Float16*>(p + w.heatT);
    uint32_t* hist = reinterpret_cast<uint32_t*>(p + w.hist);
    uint32_t* state = reinterpret_cast<uint32_t*>(p + w.state);
    uint32_t* chunk_eq = reinterpret_cast<uint32_t*>(p + w.chunk_eq);
    uint2* cand = reinterpret_cast<uint2*>(p + w.cand);
    const size_t items = size_t(n_scenes) * size_t(q);
    OSN_HIP(hipMemsetAsync(hist, 0, items * 256 * 4, st));
    if (counts) OSN_HIP(hipMemsetAsync(counts, 0, items * 8, st));
    hipLaunchKernelGGL(search_check_kernel, dim3(unsigned(cdiv(n_scenes, 256))), dim3(256), 0, st, scene_offsets, n_scenes, n,
                       max_scene_rows, err);
    const int mc = sel_max_chunks(max_scene_rows);
    const dim3 cgrid(unsigned(mc > 0 ? mc : 1), unsigned(n_scenes), unsigned(q));
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    _Float16* ts = static_cast<_Float16*>(topk_scores_f16);
    hipLaunchKernelGGL(select_hist_kernel<0>, cgrid, dim3(SEL_T), 0, st, heatT, w.ldT, scene_offsets, n, max_scene_rows, q, mc,
                       counts ? thresholds : nullptr, cnt, hist, state, chunk_eq);
    hipLaunchKernelGGL(select_pick_kernel<0>, dim3(unsigned(items)), dim3(256), 0, st, hist, state, k);
    hipLaunchKernelGGL(select_hist_kernel<1>, cgrid, dim3(SEL_T), 0, st, heatT, w.ldT, scene_offsets, n, max_scene_rows, q, mc,
                       nullptr, cnt, hist, state, chunk_eq);
    hipLaunchKernelGGL(select_pick_kernel<1>, dim3(unsigned(items)), dim3(256), 0, st, hist, state, k);
    hipLaunchKernelGGL(select_hist_kernel<2>, cgrid, dim3(SEL_T), 0, st, heatT, w.ldT, scene_offsets, n, max_scene_rows, q, mc,
                       nullptr, cnt, hist, state, chunk_eq);
    hipLaunchKernelGGL(select_collect_kernel, cgrid, dim3(SEL_T), 0, st, heatT, w.ldT, scene_offsets, n, max_scene_rows, q, mc, k,
                       state, chunk_eq, cand);
    hipLaunchKernelGGL(select_sort_kernel, dim3(unsigned(items)), dim3(128), 0, st, state, cand, k, ts, topk_points);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

}  // namespace osn

using namespace osn;
// the checks osn_bank_append and osn_bank_append_fp8 share: `who` names the entry in the messages, a row holds a multiple of
// `dm` features, `out` is the matrix the rows go to.  n == 0 passes without a look at the pointers: nothing to append.
static int append_args(const char* who, int dm, const void* X, int64_t n_rows, const int64_t* gather, int64_t n, int d,
                       const void* out, int64_t row0, const int32_t* err) {
    OSN_REQUIRE(n >= 0 && n_rows >= 0 && row0 >= 0 && d >= dm && d % dm == 0, OSN_E_ARG,
                "%s: need n, n_rows, row0 >= 0 and d %% %d == 0 (n=%lld n_rows=%lld row0=%lld d=%d)", who, dm, (long long)n,
                (long long)n_rows, (long long)row0, d);
    OSN_REQUIRE(err, OSN_E_ARG, "%s: null err word", who);
    OSN_REQUIRE(gather || n <= n_rows, OSN_E_ARG, "%s: %lld rows wanted of %lld", who, (long long)n, (long long)n_rows);
    if (n == 0) return OSN_OK;
    OSN_REQUIRE(X && out, OSN_E_ARG, "%s: null pointer", who);
    OSN_REQUIRE(aligned16(X) && aligned16(out), OSN_E_ARG, "%s: X and the bank's rows must be 16-byte aligned", who);
    return OSN_OK;
}

extern "C" int osn_bank_append(const float* X, int64_t n_rows, const int64_t* gather, int64_t n, int d, void* bank_f16,
                               int64_t row0, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = append_args("osn_bank_append", 8, X, n_rows, gather, n, d, bank_f16, row0, err);
    if (rc != OSN_OK || n == 0) return rc;
    _Float16* out = static_cast<_Float16*>(bank_f16) + row0 * int64_t(d);
    const int64_t blocks = cdiv(n * (d / 4), 256);
    const unsigned grid = unsigned(blocks < (int64_t(1) << 20) ? blocks : (int64_t(1) << 20));
    hipLaunchKernelGGL(bank_append_kernel, dim3(grid), dim3(256), 0, st, X, n_rows, gather, n, d / 4, out, err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_bank_append_fp8(const void* X, int x_is_f16, int64_t n_rows, const int64_t* gather, int64_t n, int d,
                                   uint8_t* codes, int8_t* exps, int64_t row0, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(x_is_f16 == 0 || x_is_f16 == 1, OSN_E_ARG, "osn_bank_append_fp8: x_is_f16=%d (0 or 1)", x_is_f16);
    const int rc = append_args("osn_bank_append_fp8", 16, X, n_rows, gather, n, d, codes, row0, err);
    if (rc != OSN_OK || n == 0) return rc;
    OSN_REQUIRE(exps, OSN_E_ARG, "osn_bank_append_fp8: null pointer");
    uint8_t* out = codes + row0 * int64_t(d);
    const int64_t blocks = cdiv(n, 4);
    const dim3 grid(unsigned(blocks < (int64_t(1) << 20) ? blocks : (int64_t(1) << 20)));
    if (x_is_f16) hipLaunchKernelGGL(bank_append_fp8_kernel<true>, grid, dim3(256), 0, st, X, n_rows, gather, n, d / 16, out, exps + row0, err);
    else hipLaunchKernelGGL(bank_append_fp8_kernel<false>, grid, dim3(256), 0, st, X, n_rows, gather, n, d / 16, out, exps + row0, err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

// 0 = fine, else OSN_E_ARG with the error bits spelled out (synchronises the stream)
extern "C" int osn_bank_check(const int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_bank_check: null pointer");
    int32_t h = 0;
    OSN_HIP(hipMemcpyAsync(&h, err, 4, hipMemcpyDeviceToHost, st));
    OSN_HIP(hipStreamSynchronize(st));
    OSN_REQUIRE(!(h & BANK_E_GATHER), OSN_E_ARG, "osn_bank_append: a gather index outside [0, n_rows) (X[gather] raises in the reference)");
    OSN_REQUIRE(!(h & BANK_E_OFFSETS), OSN_E_ARG, "osn_bank_search: scene_offsets must start at 0, ascend and end within the bank");
    OSN_REQUIRE(!(h & BANK_E_LONG), OSN_E_ARG, "osn_bank_search: a scene is longer than max_scene_rows");
    OSN_REQUIRE(!(h & BANK_E_POOL_ROW), OSN_E_ARG, "osn_bank_pool: a row index outside [0, n) (the entry was skipped)");
    OSN_REQUIRE(!(h & BANK_E_POOL_WEIGHT), OSN_E_ARG, "osn_bank_pool: a negative or non-finite weight (the entry was skipped)");
    OSN_REQUIRE(!(h & BANK_E_POOL_STARTS), OSN_E_ARG, "osn_bank_pool: starts must ascend from 0 to the number of entries");
    return OSN_OK;
}

extern "C" size_t osn_bank_search_ws_bytes(int64_t n, int n_scenes, int q, int k, int64_t max_scene_rows) {
    return search_ws(n, n_scenes, q, k, max_scene_rows).total;
}

// the second source of an ensemble search (osn_bank_search_ensemble): null for every other entry
struct Ensemble {
    const void* rows;      // fp16 rows, or codes
    const int8_t* exps;    // the codes' row exponents
    int mode;              // 0 vocabulary, 1 query
    uint8_t* source;       // [n] (mode 0) | [n, q], nullable (mode 1)
};

// pass 1 of every search: one or two column tiles (32 or 64 columns a group); three workgroups per CU over fp16 rows, two over
// codes (heat_fp8_kernel).  The CONTRAST instances keep these bounds: the relevancy adds no register that lives across the
// chunk loop and 512 bytes of LDS (3 x 53248 B with two column tiles, of 160 KB).
// The ensemble instances over fp16 rows run TWO workgroups per CU.  Their LDS fits three (ENS_VOCABULARY adds 512 bytes to
// CONTRAST's, 3 x 53760 B; ENS_QUERY 1024, 3 x 54272 B = 162816 of 163840), but held to the 168 VGPRs
// of three they spill 64 .. 436 bytes a lane inside the walk; measured at 8 x 150 k x 768 x 32 (heat pass, us, three | two per CU):
// vocabulary 1042 | 997, with 4 negatives 1158 | 1183; query 864 | 805, with 4 negatives 1727 | 1318 (the last pair with both
// sources' negatives ahead of the queries; a source's negatives next to its first group of queries: 1180 at two per CU).
constexpr int ENS_WGS16 = 2;
template <bool CONTRAST, int ENS>
static void heat_launch(bool fp8, const void* rows, const int8_t* exps, const _Float16* T, _Float16* heat, _Float16* heatT,
                        int64_t ldT, int64_t n, int d, int q, int normalize, const _Float16* Tn, int m, float temperature,
                        const void* rows2, const int8_t* exps2, uint8_t* source, hipStream_t st) {
    const dim3 grid(unsigned(cdiv(n, S_BM))), block(256);
    const bool one = q <= 32 && m <= 32;                    // (m = 0 without negatives)
    if (fp8) {
        const uint8_t* B = static_cast<const uint8_t*>(rows);
        const uint8_t* B2 = static_cast<const uint8_t*>(rows2);
        if (one) hipLaunchKernelGGL((heat_fp8_kernel<1, 2, CONTRAST, ENS>), grid, block, 0, st, B, exps, T, heat, heatT, ldT, n, d, q, normalize, Tn, m, temperature, B2, exps2, source);
        else hipLaunchKernelGGL((heat_fp8_kernel<2, 2, CONTRAST, ENS>), grid, block, 0, st, B, exps, T, heat, heatT, ldT, n, d, q, normalize, Tn, m, temperature, B2, exps2, source);
    } else {
        const _Float16* B = static_cast<const _Float16*>(rows);
        const _Float16* B2 = static_cast<const _Float16*>(rows2);
        if (one) hipLaunchKernelGGL((heat_kernel<1, ENS == ENS_NONE ? 3 : ENS_WGS16, CONTRAST, ENS>), grid, block, 0, st, B, T, heat, heatT, ldT, n, d, q, normalize, Tn, m, temperature, B2, source);
        else hipLaunchKernelGGL((heat_kernel<2, ENS == ENS_NONE ? 3 : ENS_WGS16, CONTRAST, ENS>), grid, block, 0, st, B, T, heat, heatT, ldT, n, d, q, normalize, Tn, m, temperature, B2, source);
    }
}

// the negatives of a contrast search (osn_bank_search_contrast): null for the plain entries
struct Contrast {
    const void* negatives_f16;
    int m;
    float temperature;
};

// every search: `rows` are fp16 rows or, with `fp8`, e4m3 codes that go with the row exponents `exps`; `who` names the entry
// in the messages; `contrast` (nullable) turns the scores into relevancies; `ens` (nullable) is the second source
static int bank_search_impl(const char* who, bool fp8, const void* rows, const int8_t* exps, int64_t n, int d, const int64_t* scene_offsets,
                            int n_scenes, int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                            const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points, int64_t* counts,
                            int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream, const Contrast* contrast = nullptr,
                            const Ensemble* ens = nullptr) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int dm = fp8 ? 16 : 8;
    OSN_REQUIRE(n >= 0 && d >= dm && d % dm == 0 && q >= 1 && q <= 1024, OSN_E_ARG,
                "%s: need n >= 0, d %% %d == 0 and 1 <= q <= 1024 (n=%lld d=%d q=%d)", who, dm, (long long)n, d, q);
    OSN_REQUIRE(n_scenes >= 0 && n_scenes <= 65535 && max_scene_rows >= 0 && max_scene_rows < (int64_t(1) << 31), OSN_E_ARG,
                "%s: n_scenes=%d (0 .. 65535) max_scene_rows=%lld (< 2^31)", who, n_scenes, (long long)max_scene_rows);
    OSN_REQUIRE((normalize == 0 || normalize == 1) && k >= 1 && k <= 128, OSN_E_ARG, "%s: normalize=%d (0 or 1) k=%d (1 .. 128)", who,
                normalize, k);
    OSN_REQUIRE(queries_f16 && aligned16(queries_f16), OSN_E_ARG, "%s: queries must be non-null and 16-byte aligned", who);
    OSN_REQUIRE(n == 0 || (rows && aligned16(rows) && (exps || !fp8)), OSN_E_ARG,
                "%s: the bank's rows%s must be non-null, the rows 16-byte aligned", who, fp8 ? " and exponents" : "");
    OSN_REQUIRE(n_scenes == 0 || (scene_offsets && topk_scores_f16 && topk_points && err), OSN_E_ARG, "%s: null pointer", who);
    OSN_REQUIRE(!counts || thresholds, OSN_E_ARG, "%s: counts need thresholds", who);
    if (contrast) {
        OSN_REQUIRE(contrast->m >= 1 && contrast->m <= 1024, OSN_E_ARG, "%s: need 1 <= m <= 1024 negatives (m=%d)", who, contrast->m);
        OSN_REQUIRE(contrast->temperature > 0.f && contrast->temperature < INFINITY, OSN_E_ARG,
                    "%s: the temperature must be finite and > 0 (%g)", who, double(contrast->temperature));
        OSN_REQUIRE(contrast->negatives_f16 && aligned16(contrast->negatives_f16), OSN_E_ARG,
                    "%s: negatives must be non-null and 16-byte aligned", who);
    }
    if (ens) {
        OSN_REQUIRE(ens->mode == 0 || ens->mode == 1, OSN_E_ARG, "%s: mode=%d (0 vocabulary, 1 query)", who, ens->mode);
        OSN_REQUIRE(n == 0 || (ens->rows && aligned16(ens->rows) && (ens->exps || !fp8)), OSN_E_ARG,
                    "%s: the other bank's rows%s must be non-null, the rows 16-byte aligned", who, fp8 ? " and exponents" : "");
        OSN_REQUIRE(n == 0 || ens->mode == 1 || ens->source, OSN_E_ARG, "%s: vocabulary mode needs source [n]", who);
    }
    const SearchWs w = search_ws(n, n_scenes, q, k, max_scene_rows);
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= w.total, OSN_E_WS, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    char* p = static_cast<char*>(ws);
    _Float16* heatT = reinterpret_cast<_Float16*>(p + w.heatT);
    if (n > 0) {
        const _Float16* T = static_cast<const _Float16*>(queries_f16);
        _Float16* heat = static_cast<_Float16*>(heat_f16);
        const _Float16* Tn = contrast ? static_cast<const _Float16*>(contrast->negatives_f16) : nullptr;
        const int m = contrast ? contrast->m : 0;
        const float tau = contrast ? contrast->temperature : 0.f;
        const void* rows2 = ens ? ens->rows : nullptr;
        const int8_t* exps2 = ens ? ens->exps : nullptr;
        uint8_t* source = ens ? ens->source : nullptr;
        auto launch = [&](auto has_negatives) {
            constexpr bool C = decltype(has_negatives)::value;
            if (!ens) heat_launch<C, ENS_NONE>(fp8, rows, exps, T, heat, heatT, w.ldT, n, d, q, normalize, Tn, m, tau, rows2, exps2, source, st);
            else if (ens->mode == 0) heat_launch<C, ENS_VOCABULARY>(fp8, rows, exps, T, heat, heatT, w.ldT, n, d, q, normalize, Tn, m, tau, rows2, exps2, source, st);
            else heat_launch<C, ENS_QUERY>(fp8, rows, exps, T, heat, heatT, w.ldT, n, d, q, normalize, Tn, m, tau, rows2, exps2, source, st);
        };
        if (contrast) launch(std::true_type());
        else launch(std::false_type());
        OSN_LAUNCH_CHECK();
    }
    if (n_scenes == 0) return OSN_OK;
    return select_pass(w, p, n, scene_offsets, n_scenes, max_scene_rows, q, k, thresholds, topk_scores_f16, topk_points, counts, err, st);
}

extern "C" int osn_bank_search(const void* bank_f16, int64_t n, int d, const int64_t* scene_offsets, int n_scenes,
                               int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                               const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                               int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return bank_search_impl("osn_bank_search", false, bank_f16, nullptr, n, d, scene_offsets, n_scenes, max_scene_rows, queries_f16, q,
                            normalize, k, thresholds, heat_f16, topk_scores_f16, topk_points, counts, err, ws, ws_bytes, stream);
}

extern "C" int osn_bank_search_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* scene_offsets,
                                   int n_scenes, int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                                   const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                                   int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return bank_search_impl("osn_bank_search_fp8", true, codes, exps, n, d, scene_offsets, n_scenes, max_scene_rows,
                            queries_f16, q, normalize, k, thresholds, heat_f16, topk_scores_f16, topk_points, counts, err, ws,
                            ws_bytes, stream);
}

extern "C" int osn_bank_search_contrast(const void* bank_f16, int64_t n, int d, const int64_t* scene_offsets, int n_scenes,
                                        int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                                        const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                                        int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream,
                                        const void* negatives_f16, int m, float temperature) {
    const Contrast c = {negatives_f16, m, temperature};
    return bank_search_impl("osn_bank_search_contrast", false, bank_f16, nullptr, n, d, scene_offsets, n_scenes, max_scene_rows,
                            queries_f16, q, normalize, k, thresholds, heat_f16, topk_scores_f16, topk_points, counts, err, ws,
                            ws_bytes, stream, &c);
}

extern "C" int osn_bank_search_contrast_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* scene_offsets,
                                            int n_scenes, int64_t max_scene_rows, const void* queries_f16, int q, int normalize,
                                            int k, const float* thresholds, void* heat_f16, void* topk_scores_f16,
                                            int64_t* topk_points, int64_t* counts, int32_t* err, void* ws, size_t ws_bytes,
                                            osn_stream_t stream, const void* negatives_f16, int m, float temperature) {
    const Contrast c = {negatives_f16, m, temperature};
    return bank_search_impl("osn_bank_search_contrast_fp8", true, codes, exps, n, d, scene_offsets, n_scenes, max_scene_rows,
                            queries_f16, q, normalize, k, thresholds, heat_f16, topk_scores_f16, topk_points, counts, err, ws,
                            ws_bytes, stream, &c);
}

// two banks as one (include/openscene_amd.h): m = 0 with null negatives means plain scores
static int bank_search_ensemble_impl(const char* who, bool fp8, const void* rows, const int8_t* exps, const void* rows2,
                                     const int8_t* exps2, int64_t n, int d, const int64_t* scene_offsets, int n_scenes,
                                     int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                                     const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                                     int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream,
                                     const void* negatives_f16, int m, float temperature, int mode, uint8_t* source) {
    const Contrast c = {negatives_f16, m, temperature};
    const Ensemble e = {rows2, exps2, mode, source};
    const bool plain = m == 0 && !negatives_f16;
    return bank_search_impl(who, fp8, rows, exps, n, d, scene_offsets, n_scenes, max_scene_rows, queries_f16, q, normalize, k,
                            thresholds, heat_f16, topk_scores_f16, topk_points, counts, err, ws, ws_bytes, stream,
                            plain ? nullptr : &c, &e);
}

extern "C" int osn_bank_search_ensemble(const void* bank_f16, const void* other_f16, int64_t n, int d, const int64_t* scene_offsets,
                                        int n_scenes, int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                                        const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                                        int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream,
                                        const void* negatives_f16, int m, float temperature, int mode, uint8_t* source) {
    return bank_search_ensemble_impl("osn_bank_search_ensemble", false, bank_f16, nullptr, other_f16, nullptr, n, d, scene_offsets,
                                     n_scenes, max_scene_rows, queries_f16, q, normalize, k, thresholds, heat_f16, topk_scores_f16,
                                     topk_points, counts, err, ws, ws_bytes, stream, negatives_f16, m, temperature, mode, source);
}

extern "C" int osn_bank_search_ensemble_fp8(const uint8_t* codes, const int8_t* exps, const uint8_t* other_codes,
                                            const int8_t* other_exps, int64_t n, int d, const int64_t* scene_offsets, int n_scenes,
                                            int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                                            const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                                            int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream,
                                            const void* negatives_f16, int m, float temperature, int mode, uint8_t* source) {
    return bank_search_ensemble_impl("osn_bank_search_ensemble_fp8", true, codes, exps, other_codes, other_exps, n, d, scene_offsets,
                                     n_scenes, max_scene_rows, queries_f16, q, normalize, k, thresholds, heat_f16, topk_scores_f16,
                                     topk_points, counts, err, ws, ws_bytes, stream, negatives_f16, m, temperature, mode, source);
}
