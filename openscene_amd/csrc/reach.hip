// Nearest sources at any range on gfx950: for every query cell the nearest source cell of the same scene inside a Euclidean
// ball of `reach` cells, exactly.  On the integer lattice d2 = dx dx + dy dy + dz dz is an integer, so the result -- the
// minimum of the 64-bit key  uint32(d2) << 32 | uint32(id)  over the candidates -- is a pure function of the inputs: no
// floating point, no atomics across workgroups, and whatever the schedule two calls give the same bits.
//
//   osn_reach_nearest   per query (scene, x, y, z): the candidates are the sources of its scene with |dx|, |dy|, |dz| <= reach
//                       and d2 <= reach^2; -> dist2 (the d2 of the minimum key), nearest (its id); -1, -1 without a candidate
//
// The caller hands over sorted data (host plumbing, openscene_amd.ops.reach_nearest): the sources sorted by (scene, block),
// block = cell >> 3 per axis (arithmetic: a floor division, right for negative cells), as 16-byte entries (x, y, z, id); the
// table of the occupied blocks (scene, bx, by, bz) with the start of each block's entries; the queries sorted the same way;
// and WORK ITEMS (q_start, q_end, block_start, block_end): at most 256 consecutive sorted queries of one scene and the range
// of that scene's blocks.
//
// Work layout.  One workgroup per item, one query per lane.  The workgroup reduces the bounding box of its queries (LDS
// integer atomics), then walks the scene's blocks twice: first the blocks that touch the box, so that every lane has a good
// candidate early, then the others.  A block is skipped when its per-axis gap to the box exceeds `reach`, or when its
// squared gap exceeds the workgroup's bound: the largest current best d2 over the item's lanes (reach^2 for a lane without a
// candidate).  The bound is read after a barrier and only ever shrinks, so a stale value is merely loose; a block at EXACTLY
// the bound is visited (it may hold an equal d2 under a lower id).  A visited block is staged in LDS (512 entries: 8^3 cells;
// a longer block, one with repeated cells, in runs of 512) and every lane scans it after the same two tests against its own
// cell and its own best.  All branches around barriers depend on values every lane reads alike: the item, the block table,
// the box and the bound from LDS.
//
// Integer range.  Cells lie in |c| < 32767, so a difference reaches 65 532 and its square does not fit 32 bits.  No such
// square is formed: a per-axis distance is clamped to reach + 1 first (reach <= 4096), which alone puts d2 over reach^2 --
// 3 (reach + 1)^2 < 2^26 -- so an axis beyond reach rejects the candidate and no wrapped value is ever compared.
//
// Every index read from memory is checked before it is used: an item's query and block ranges, a block's entry range and
// coordinates, a query's place in the caller's order, every cell against the packable range.  A bad entry is skipped and
// recorded in the err word; the wrapper raises on it.
#include "common.h"

namespace osn {

using u64 = unsigned long long;
constexpr int REACH_T = 256;                 // lanes per workgroup = queries per item
constexpr int REACH_STAGE = 512;             // entries of one 8^3 block
constexpr int REACH_MAX = 4096;
constexpr int REACH_COORD = 32767;           // |cell| < this (the packable range of the coordinate keys)
constexpr int REACH_BLOCK = 4096;            // |block| <= this: cell >> 3
constexpr int REACH_E_ITEM = 1, REACH_E_BLOCK = 2, REACH_E_CELL = 4, REACH_E_ORDER = 8;
constexpr u64 REACH_NONE = ~u64(0);
constexpr int REACH_FAR = 1 << 30;           // the x of a staged entry no query reaches (|x - q| > reach, no overflow)

struct ReachArgs {
    const int4* q_cells; const int32_t* order; int64_t n_q;
    const int4* items; int64_t n_items;
    const int4* src; int64_t n_src;
    const int4* blocks; const int32_t* block_start; int64_t n_blocks;
    int reach;
    int32_t* dist2; int32_t* nearest; int32_t* err;
};

// The gap between the integer intervals [lo_a, hi_a] and [lo_b, hi_b]: 0 when they meet.
__device__ inline int axis_gap(int lo_a, int hi_a, int lo_b, int hi_b) { return max(0, max(lo_a - hi_b, lo_b - hi_a)); }

__device__ inline bool cell_ok(int x, int y, int z) {
    return x > -REACH_COORD && x < REACH_COORD && y > -REACH_COORD && y < REACH_COORD && z > -REACH_COORD && z < REACH_COORD;
}

__global__ __launch_bounds__(REACH_T) void reach_nearest_kernel(ReachArgs a) {
    __shared__ int4 stage[REACH_STAGE];
    __shared__ int box[6];
    __shared__ int worst[REACH_T / 64];
    const int t = threadIdx.x;
    const int4 item = a.items[blockIdx.x];
    const int64_t qs = item.x, qe = item.y, bs = item.z, be = item.w;
    if (qs < 0 || qe > a.n_q || qe < qs || qe - qs > REACH_T || bs < 0 || be > a.n_blocks || be < bs) {      // (the same for every lane)
        if (t == 0) atomicOr(a.err, REACH_E_ITEM);
        return;
    }
    const int reach = a.reach, reach2 = reach * reach, over = reach + 1;
    int64_t row = -1;                                        // where this lane's result goes; -1: nowhere
    bool active = false;                                     // this lane searches
    int qx = 0, qy = 0, qz = 0;
    if (qs + t < qe) {
        const int4 q = a.q_cells[qs + t];
        row = a.order ? a.order[qs + t] : qs + t;
        if (row < 0 || row >= a.n_q) { atomicOr(a.err, REACH_E_ORDER); row = -1; }
        qx = q.y; qy = q.z; qz = q.w;
        active = cell_ok(qx, qy, qz);
        if (!active) { atomicOr(a.err, REACH_E_CELL); qx = qy = qz = 0; }
    }
    if (t == 0) {
        box[0] = box[1] = box[2] = REACH_COORD;
        box[3] = box[4] = box[5] = -REACH_COORD;
    }
    __syncthreads();
    if (active) {
        atomicMin(&box[0], qx); atomicMin(&box[1], qy); atomicMin(&box[2], qz);
        atomicMax(&box[3], qx); atomicMax(&box[4], qy); atomicMax(&box[5], qz);
    }
    __syncthreads();
    const int lox = box[0], loy = box[1], loz = box[2], hix = box[3], hiy = box[4], hiz = box[5];
    u64 best = REACH_NONE;
    if (lox <= hix) {                                        // (some lane searches; the same for every lane)
        int bound = reach2;
        for (int pass = 0; pass < 2; ++pass) {
            for (int64_t b = bs; b < be; ++b) {
                const int4 bc = a.blocks[b];                 // (scene, bx, by, bz)
                const int64_t s = a.block_start[b], e = a.block_start[b + 1];
                if (s < 0 || e > a.n_src || e < s || bc.y < -REACH_BLOCK || bc.y > REACH_BLOCK ||
                    bc.z < -REACH_BLOCK || bc.z > REACH_BLOCK || bc.w < -REACH_BLOCK || bc.w > REACH_BLOCK) {
                    if (pass == 0 && t == 0) atomicOr(a.err, REACH_E_BLOCK);
                    continue;
                }
                if (s == e) continue;
                const int bx = bc.y * 8, by = bc.z * 8, bz = bc.w * 8;
                const int gx = axis_gap(bx, bx + 7, lox, hix), gy = axis_gap(by, by + 7, loy, hiy), gz = axis_gap(bz, bz + 7, loz, hiz);
                const bool touches = (gx | gy | gz) == 0;
                if (touches != (pass == 0)) continue;
                if (gx > reach || gy > reach || gz > reach) continue;            // (before any square)
                if (gx * gx + gy * gy + gz * gz > bound) continue;
                const int lx = axis_gap(bx, bx + 7, qx, qx), ly = axis_gap(by, by + 7, qy, qy), lz = axis_gap(bz, bz + 7, qz, qz);
                const bool near_me = active && lx <= reach && ly <= reach && lz <= reach;           // (before any square)
                const int gap2 = near_me ? lx * lx + ly * ly + lz * lz : 0;
                for (int64_t c0 = s; c0 < e; c0 += REACH_STAGE) {                // (one run, unless cells repeat)
                    const int n = int(min(e - c0, int64_t(REACH_STAGE)));
                    for (int i = t; i < n; i += REACH_T) {
                        int4 c = a.src[c0 + i];
                        if (!cell_ok(c.x, c.y, c.z)) { atomicOr(a.err, REACH_E_CELL); c.x = REACH_FAR; c.y = 0; c.z = 0; }
                        stage[i] = c;
                    }
                    __syncthreads();
                    if (near_me && gap2 <= (best == REACH_NONE ? reach2 : int(uint32_t(best >> 32)))) {
                        for (int i = 0; i < n; ++i) {
                            const int4 c = stage[i];             // (one address for the wave: a broadcast)
                            const int dx = min(abs(c.x - qx), over), dy = min(abs(c.y - qy), over), dz = min(abs(c.z - qz), over);
                            const int d2 = dx * dx + dy * dy + dz * dz;
                            const u64 key = (u64(uint32_t(d2)) << 32) | u64(uint32_t(c.w));
                            if (d2 <= reach2 && key < best) best = key;
                        }
                    }
                    int m = !active ? 0 : best == REACH_NONE ? reach2 : int(uint32_t(best >> 32));
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
                    if ((t & 63) == 0) worst[t >> 6] = m;
                    __syncthreads();                             // the scan is over: the stage is free, the bound is whole
                }
                bound = max(max(worst[0], worst[1]), max(worst[2], worst[3]));
            }
        }
    }
    if (row >= 0) {
        const bool some = best != REACH_NONE;
        a.dist2[row] = some ? int32_t(uint32_t(best >> 32)) : -1;
        a.nearest[row] = some ? int32_t(uint32_t(best)) : -1;
    }
}

}  // namespace osn

using namespace osn;

extern "C" int osn_reach_nearest(const int32_t* q_cells, const int32_t* order, int64_t n_queries, const int32_t* items, int64_t n_items,
                                 const int32_t* src, int64_t n_src, const int32_t* blocks, const int32_t* block_start, int64_t n_blocks,
                                 int reach, int32_t* dist2, int32_t* nearest, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t lim = int64_t(1) << 31;
    OSN_REQUIRE(n_queries >= 0 && n_queries < lim && n_items >= 0 && n_items < lim && n_src >= 0 && n_src < lim && n_blocks >= 0 && n_blocks < lim,
                OSN_E_ARG, "osn_reach_nearest: sizes out of range (n_queries=%lld n_items=%lld n_src=%lld n_blocks=%lld)", (long long)n_queries,
                (long long)n_items, (long long)n_src, (long long)n_blocks);
    OSN_REQUIRE(reach >= 1 && reach <= REACH_MAX, OSN_E_ARG, "osn_reach_nearest: reach=%d outside 1 .. %d", reach, REACH_MAX);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_reach_nearest: null err");
    if (n_queries == 0 || n_items == 0) return OSN_OK;
    OSN_REQUIRE(q_cells && items && block_start && dist2 && nearest && (n_src == 0 || src) && (n_blocks == 0 || blocks), OSN_E_ARG,
                "osn_reach_nearest: null pointer");
    OSN_REQUIRE(aligned16(q_cells) && aligned16(items) && aligned16(src) && aligned16(blocks), OSN_E_ARG,
                "osn_reach_nearest: q_cells, items, src and blocks must be 16-byte aligned");
    ReachArgs a;
    a.q_cells = reinterpret_cast<const int4*>(q_cells); a.order = order; a.n_q = n_queries;
    a.items = reinterpret_cast<const int4*>(items); a.n_items = n_items;
    a.src = reinterpret_cast<const int4*>(src); a.n_src = n_src;
    a.blocks = reinterpret_cast<const int4*>(blocks); a.block_start = block_start; a.n_blocks = n_blocks;
    a.reach = reach; a.dist2 = dist2; a.nearest = nearest; a.err = err;
    hipLaunchKernelGGL(reach_nearest_kernel, dim3(unsigned(n_items)), dim3(REACH_T), 0, st, a);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
