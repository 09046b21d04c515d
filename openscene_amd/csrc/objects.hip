// Objects in heat-maps on gfx950: connected components of the voxels that hold a point over a query's threshold, and one
// exact record per component (README "Applications": rare object search in a scene database, image-based 3-D object
// detection, interactive object search -- all of them want objects, not points).
//
//   osn_objects_label   activate -> union-find over the 3^3 self-map -> flatten -> number the components per (scene, query)
//   osn_objects_find    per-component records (integer atomics) -> per (scene, query) the best M objects
//
// Label.  One 32-bit word per (query, voxel): -1 = inactive, else a voxel row of the same component that is not larger
// than the word's own row ("parent").  Every edge (v, u) of the 13 "earlier" offsets of the self-map (the map is its own
// mirror, so these are all edges) is united once: find both roots, hook the LARGER root under the SMALLER with a
// compare-and-swap, start again from what the CAS returned when it lost.  Parents only ever decrease, a root is the
// smallest row of its tree, and a word that stopped being a root never becomes one again, so whatever order the hooks
// land in, the forest that remains has exactly one root per connected component: the component's smallest row.  The
// partition is a property of the graph, not of the schedule.  Finds read with agent-scope loads and halve the path as they
// go (a stale read only yields an older, still valid, ancestor: the CAS is the arbiter).  A 1-voxel-wide corridor of 10^4
// voxels costs 10^4 near-constant unions, not 10^4 sweeps.
//
// Numbering.  Roots draw a slot from their (scene, query)'s counter; a scan of the counters makes the components of an
// item contiguous.  Which root gets which slot depends on arrival order, and nothing that leaves the library does: the
// selection orders objects by (peak score, peak point), a total order.
//
// Reduce.  A workgroup stages 256 heat rows x 32 queries through LDS (the rows are read coalesced along Q), then a lane
// owns one point and walks the queries, so the 64 lanes of a wave hold 64 CONSECUTIVE points of ONE query -- neighbours in
// the scan, usually on the same object.  Lanes that target the same record are combined before ONE lane issues the atomics
// (components.h: wave_combine, its all-lanes contract and why the records are the same bits on every call).  Integer atomics
// only: count, 2^24 fixed-point int64 score sum, (score key, ~point) 64-bit max, and the voxel sums and box of BoxVox.
#include "components.h"      // the union-find, BoxVox and wave_combine: shared with regions.hip

namespace osn {

constexpr int OBJ_E_INVERSE = 1, OBJ_E_SCENE = 2, OBJ_E_OFFSETS = 4, OBJ_E_NBR = 8;
constexpr int OBJ_T = COMPONENTS_T;
constexpr int OBJ_QC = 32;          // queries of a staged tile
constexpr int OBJ_LD = OBJ_QC + 2;  // halfs per staged row: 17 words, odd -> lanes one row apart hit different banks
constexpr int OBJ_MAX_M = 64;

// monotone key of a finite fp16 score (-0 -> +0: equal values tie on the point, as search.hip)
__device__ inline uint32_t obj_key(uint16_t hb) {
    if (hb == 0x8000u) hb = 0;
    return (hb & 0x8000u) ? (~uint32_t(hb) & 0xFFFFu) : (uint32_t(hb) | 0x8000u);
}
__device__ inline bool obj_hit(uint16_t hb, float th) {
    if ((hb & 0x7C00u) == 0x7C00u) return false;            // NaN, +inf, -inf
    return (float)__builtin_bit_cast(_Float16, hb) >= th;
}

// ------------------------------------------------------------------------------------------------------ checks
__global__ void objects_check_kernel(const int64_t* __restrict__ off, int S, int64_t n, int32_t* __restrict__ err) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int64_t a = off[s], b = off[s + 1];
    if (a < 0 || b < a || b > n || (s == 0 && a != 0) || (s == S - 1 && b != n)) atomicOr(err, OBJ_E_OFFSETS);
}

// ------------------------------------------------------------------------------------------------------ activate
// element e = p * Q + q (q fastest: the heat rows are read as they lie); a hit marks its voxel as its own root
__global__ __launch_bounds__(OBJ_T) void objects_activate_kernel(const uint16_t* __restrict__ heat, int64_t n, int Q,
                                                                 const float* __restrict__ thr, const int32_t* __restrict__ inv,
                                                                 int64_t V, int32_t* __restrict__ label, int32_t* __restrict__ err) {
    const int64_t total = n * Q;
    for (int64_t e = int64_t(blockIdx.x) * OBJ_T + threadIdx.x; e < total; e += int64_t(gridDim.x) * OBJ_T) {
        const int64_t p = e / Q;
        const int q = int(e - p * Q);
        if (!obj_hit(heat[e], thr[q])) continue;
        const int v = inv[p];
        if (v < 0 || v >= V) { atomicOr(err, OBJ_E_INVERSE); continue; }
        label[int64_t(q) * V + v] = v;                       // (every hit of the voxel stores the same word)
    }
}

// ------------------------------------------------------------------------------------------------------ label
__global__ __launch_bounds__(OBJ_T) void objects_unite_kernel(int32_t* label, const int32_t* __restrict__ nbr, int64_t V,
                                                              int Q, int conn, int32_t* __restrict__ err) {
    const int64_t total = int64_t(Q) * V;
    const int n_off = conn == 26 ? 13 : 3;
    for (int64_t e = int64_t(blockIdx.x) * OBJ_T + threadIdx.x; e < total; e += int64_t(gridDim.x) * OBJ_T) {
        const int q = int(e / V);
        const int v = int(e - int64_t(q) * V);
        int32_t* L = label + int64_t(q) * V;
        if (L[v] < 0) continue;                              // (active words stay >= 0 for good: a plain load will do)
        for (int i = 0; i < n_off; ++i) {
            const int k = conn == 26 ? i : face_offset(i);
            const int u = nbr[int64_t(k) * V + v];
            if (u < 0) continue;
            if (u >= V) { atomicOr(err, OBJ_E_NBR); continue; }
            if (ld_agent(L + u) < 0) continue;
            uf_unite(L, v, u);
        }
    }
}

// every active word -> its root; roots count themselves into their (scene, query) and keep the slot they drew
__global__ __launch_bounds__(OBJ_T) void objects_flatten_kernel(int32_t* label, int64_t V, int Q) {
    const int64_t total = int64_t(Q) * V;
    for (int64_t e = int64_t(blockIdx.x) * OBJ_T + threadIdx.x; e < total; e += int64_t(gridDim.x) * OBJ_T) {
        const int q = int(e / V);
        const int v = int(e - int64_t(q) * V);
        int32_t* L = label + int64_t(q) * V;
        if (L[v] >= 0) uf_flatten(L, v);
    }
}

// slot[q][v] of a root = its number inside its (scene, query); the label words are left as they are
__global__ __launch_bounds__(OBJ_T) void objects_number_kernel(const int32_t* __restrict__ label, const int4* __restrict__ coords, int64_t V,
                                                               int Q, int S, uint32_t* __restrict__ item_count, int32_t* __restrict__ slot,
                                                               int32_t* __restrict__ err) {
    const int64_t total = int64_t(Q) * V;
    for (int64_t e = int64_t(blockIdx.x) * OBJ_T + threadIdx.x; e < total; e += int64_t(gridDim.x) * OBJ_T) {
        const int q = int(e / V);
        const int v = int(e - int64_t(q) * V);
        if (label[e] != v) continue;
        const int s = coords[v].x;
        if (s < 0 || s >= S) { atomicOr(err, OBJ_E_SCENE); slot[e] = -1; continue; }
        slot[e] = int32_t(atomicAdd(&item_count[int64_t(s) * Q + q], 1u));
    }
}

// one workgroup: item_start[i] = components of the items before i (uint32; the caller bounds Q * V below 2^31), [items] = all
__global__ __launch_bounds__(OBJ_T) void objects_scan_kernel(const uint32_t* __restrict__ item_count, int64_t items, uint32_t* __restrict__ item_start) {
    __shared__ uint32_t sh[OBJ_T];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < items; base += OBJ_T) {
        const int64_t i = base + tid;
        const uint32_t own = i < items ? item_count[i] : 0u;
        sh[tid] = own;
        __syncthreads();
        for (int o = 1; o < OBJ_T; o <<= 1) {
            const uint32_t v = sh[tid] + (tid >= o ? sh[tid - o] : 0u);
            __syncthreads();
            sh[tid] = v;
            __syncthreads();
        }
        const uint32_t c = carry;
        if (i < items) item_start[i] = c + sh[tid] - own;
        __syncthreads();
        if (tid == OBJ_T - 1) carry = c + sh[tid];
        __syncthreads();
    }
    if (tid == 0) item_start[items] = carry;
}

// ------------------------------------------------------------------------------------------------------ records
struct Records {                    // one array per field, C entries each
    uint32_t* n_points;
    uint32_t* n_voxels;
    u64* score_sum;                 // two's complement int64
    u64* peak;                      // (score key << 32) | ~point
    u64* vox_sum;                   // [3][C]
    uint32_t* box;                  // [6][C]: min x y z, max x y z, order-preserving
    int32_t* rank;                  // place among the kept objects of its item, or -1
};
constexpr size_t OBJ_REC_BYTES = 4 + 4 + 8 + 8 + 24 + 24 + 4;

static size_t records_bytes(int64_t c) { return align_up(size_t(c > 0 ? c : 1) * OBJ_REC_BYTES + 8 * 16, 256); }
static Records records_at(void* base, int64_t c) {
    const size_t C = size_t(c > 0 ? c : 1);
    char* p = static_cast<char*>(base);
    Records r;
    r.score_sum = reinterpret_cast<u64*>(p); p += C * 8;
    r.peak = reinterpret_cast<u64*>(p); p += C * 8;
    r.vox_sum = reinterpret_cast<u64*>(p); p += C * 24;
    r.box = reinterpret_cast<uint32_t*>(p); p += C * 24;
    r.n_points = reinterpret_cast<uint32_t*>(p); p += C * 4;
    r.n_voxels = reinterpret_cast<uint32_t*>(p); p += C * 4;
    r.rank = reinterpret_cast<int32_t*>(p);
    return r;
}
__device__ inline BoxArrays box_arrays(const Records& R, int64_t C) { return {R.vox_sum, R.box, R.box + 3 * C, C, 1}; }

__global__ void objects_preset_kernel(Records R, int64_t C) {
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= C) return;
    R.n_points[c] = 0; R.n_voxels[c] = 0; R.score_sum[c] = 0; R.peak[c] = 0; R.rank[c] = -1;
    BoxVox::preset(box_arrays(R, C), c);
}

// component of the active word (q, v), or -1
__device__ inline int64_t obj_component(const int32_t* __restrict__ label, const int32_t* __restrict__ slot, const int4* __restrict__ coords,
                                        const uint32_t* __restrict__ item_start, int64_t V, int Q, int S, int q, int v, int* scene) {
    const int r = label[int64_t(q) * V + v];
    if (r < 0 || r >= V) return -1;
    const int s = coords[r].x;
    if (s < 0 || s >= S) return -1;
    const int sl = slot[int64_t(q) * V + r];
    if (sl < 0) return -1;
    *scene = s;
    return int64_t(item_start[int64_t(s) * Q + q]) + sl;
}

__global__ __launch_bounds__(OBJ_T) void objects_voxels_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ slot,
                                                               const int4* __restrict__ coords, const uint32_t* __restrict__ item_start,
                                                               int64_t V, int Q, int S, int64_t C, Records R) {
    const int64_t total = int64_t(Q) * V;
    for (int64_t e = int64_t(blockIdx.x) * OBJ_T + threadIdx.x; e < total; e += int64_t(gridDim.x) * OBJ_T) {
        const int q = int(e / V);
        const int v = int(e - int64_t(q) * V);
        if (label[e] < 0) continue;
        int s;
        const int64_t c = obj_component(label, slot, coords, item_start, V, Q, S, q, v, &s);
        if (c >= 0 && c < C) atomicAdd(&R.n_voxels[c], 1u);
    }
}

// what a hit adds to its component's record
struct ObjHit {
    BoxVox b;
    u64 sc, pk;                     // 2^24 fixed-point score (sum); (score key << 32) | ~point (max)
    __device__ static ObjHit identity() { return {BoxVox::identity(), 0, 0}; }
    __device__ void merge_xor(int mask) {
        sc += shfl_xor_u64(sc, mask);
        const u64 o = shfl_xor_u64(pk, mask);
        pk = o > pk ? o : pk;
        b.merge_xor(mask);
    }
};

// COMBINE = false issues every hit's atomics on its own (tools/micro_objects.py measures the difference)
template <bool COMBINE>
__global__ __launch_bounds__(OBJ_T) void objects_reduce_kernel(const uint16_t* __restrict__ heat, const float* __restrict__ xyz, int64_t n, int Q,
                                                               const float* __restrict__ thr, const int32_t* __restrict__ inv,
                                                               const int4* __restrict__ coords, const int64_t* __restrict__ off,
                                                               const int32_t* __restrict__ label, const int32_t* __restrict__ slot,
                                                               const uint32_t* __restrict__ item_start, int64_t V, int S, int64_t C, Records R) {
    __shared__ uint16_t tile[OBJ_T][OBJ_LD];
    const int tid = threadIdx.x;
    const int64_t p0 = int64_t(blockIdx.x) * OBJ_T;
    const int64_t p = p0 + tid;
    const bool live = p < n;
    int v = -1, vx = 0, vy = 0, vz = 0, scene_p = -1;
    uint32_t bx = 0, by = 0, bz = 0, pt = 0;
    if (live) {
        v = inv[p];
        if (v < 0 || v >= V) v = -1;
    }
    if (v >= 0) {
        const int4 cv = coords[v];
        scene_p = cv.x; vx = cv.y; vy = cv.z; vz = cv.w;
        if (scene_p < 0 || scene_p >= S) v = -1;
    }
    if (v >= 0) {
        const int64_t o = off[scene_p];
        if (p < o || p - o >= (int64_t(1) << 31)) v = -1;
        else pt = uint32_t(p - o);
        bx = f2o(xyz[p * 3 + 0]); by = f2o(xyz[p * 3 + 1]); bz = f2o(xyz[p * 3 + 2]);
    }
    const BoxArrays A = box_arrays(R, C);
    const auto commit = [&](int c, const ObjHit& h, int cnt) {
        atomicAdd(&R.n_points[c], uint32_t(cnt));
        atomicAdd(&R.score_sum[c], h.sc);
        atomicMax(&R.peak[c], h.pk);
        h.b.commit(A, c);
    };
    for (int q0 = 0; q0 < Q; q0 += OBJ_QC) {
        const int qn = Q - q0 < OBJ_QC ? Q - q0 : OBJ_QC;
        __syncthreads();
        for (int e = tid; e < OBJ_T * qn; e += OBJ_T) {
            const int r = e / qn, c = e - r * qn;
            tile[r][c] = p0 + r < n ? heat[(p0 + r) * Q + q0 + c] : uint16_t(0x7E00);
        }
        __syncthreads();
        for (int c = 0; c < qn; ++c) {
            const int q = q0 + c;
            const uint16_t hb = tile[tid][c];
            int comp = -1;                                   // (C <= Q * V < 2^31)
            if (v >= 0 && obj_hit(hb, thr[q])) {
                int s;
                const int64_t c64 = obj_component(label, slot, coords, item_start, V, Q, S, q, v, &s);
                if (c64 >= 0 && c64 < C && s == scene_p) comp = int(c64);
            }
            if (!__ballot(comp >= 0)) continue;              // (wave-uniform; most waves of a sparse heat-map leave here)
            ObjHit h;
            h.b = BoxVox::point(vx, vy, vz, bx, by, bz);
            h.sc = u64((long long)((float)__builtin_bit_cast(_Float16, hb) * 16777216.0f));
            h.pk = (u64(obj_key(hb)) << 32) | u64(~pt);
            if (COMBINE) wave_combine<COMBINE_MIN>(comp, h, commit);
            else if (comp >= 0) commit(comp, h, 1);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ select
struct ObjOut {
    int64_t* n_points; int64_t* n_voxels; uint16_t* peak_score; int64_t* peak_point; int64_t* score_sum; int64_t* vox_sum;
    float* box_min; float* box_max; int64_t* n_objects;
};

// one workgroup per (scene, query): M rounds of "the largest peak below the last one" over the item's components (the peaks of
// an item are distinct: they name distinct points), so the order is (peak score desc, peak point asc) whatever the numbering
__global__ __launch_bounds__(OBJ_T) void objects_select_kernel(const uint32_t* __restrict__ item_start, Records R, int64_t C, int Q,
                                                               const uint16_t* __restrict__ heat, const int64_t* __restrict__ off,
                                                               int64_t n, uint32_t min_points, int M, ObjOut O) {
    __shared__ u64 wk[OBJ_T / 64];
    __shared__ uint32_t wc[OBJ_T / 64];
    __shared__ uint32_t wn[OBJ_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t item = blockIdx.x;
    const int s = int(item / Q), q = int(item - int64_t(s) * Q);
    int64_t a = item_start[item], b = item_start[item + 1];
    if (b > C) b = C;
    if (a > b) a = b;
    u64 prev = ~u64(0);
    uint32_t kept_total = 0;
    for (int r = 0; r < M; ++r) {
        u64 best = 0;
        uint32_t best_c = 0, passed = 0;
        for (int64_t c = a + tid; c < b; c += OBJ_T) {
            if (R.n_points[c] < min_points || R.n_points[c] == 0) continue;
            ++passed;
            const u64 k = R.peak[c];
            if (k < prev && k > best) { best = k; best_c = uint32_t(c - a); }
        }
#pragma unroll
        for (int mk = 32; mk >= 1; mk >>= 1) {
            const u64 ok = shfl_xor_u64(best, mk);
            const uint32_t oc = __shfl_xor(best_c, mk, 64);
            if (ok > best) { best = ok; best_c = oc; }
            passed += __shfl_xor(passed, mk, 64);
        }
        __syncthreads();
        if (lane == 0) { wk[wave] = best; wc[wave] = best_c; wn[wave] = passed; }
        __syncthreads();
        best = 0; best_c = 0; passed = 0;
        for (int w = 0; w < OBJ_T / 64; ++w) {
            if (wk[w] > best) { best = wk[w]; best_c = wc[w]; }
            passed += wn[w];
        }
        if (r == 0) kept_total = passed;
        const int64_t o = item * M + r;
        if (tid == 0) {
            if (best) {
                const int64_t c = a + best_c;
                const uint32_t pt = ~uint32_t(best);
                int64_t row = off[s] + int64_t(pt);
                if (row < 0 || row >= n) row = 0;            // (cannot happen: the point came from a checked offset)
                O.n_points[o] = R.n_points[c];
                O.n_voxels[o] = R.n_voxels[c];
                O.peak_score[o] = heat[row * Q + q];
                O.peak_point[o] = int64_t(pt);
                O.score_sum[o] = int64_t(R.score_sum[c]);
                for (int j = 0; j < 3; ++j) {
                    O.vox_sum[o * 3 + j] = int64_t(R.vox_sum[j * C + c]);
                    O.box_min[o * 3 + j] = o2f(R.box[j * C + c]);
                    O.box_max[o * 3 + j] = o2f(R.box[(3 + j) * C + c]);
                }
                R.rank[c] = r;
            } else {
                O.n_points[o] = 0; O.n_voxels[o] = 0; O.peak_score[o] = 0xFC00; O.peak_point[o] = -1; O.score_sum[o] = 0;
                for (int j = 0; j < 3; ++j) { O.vox_sum[o * 3 + j] = 0; O.box_min[o * 3 + j] = 0.f; O.box_max[o * 3 + j] = 0.f; }
            }
        }
        prev = best;                                         // (0 once the item has run out: nothing is below it)
    }
    if (tid == 0) O.n_objects[item] = int64_t(kept_total);
}

// point_object[p][q] = rank of the kept object the hit belongs to, else -1
__global__ __launch_bounds__(OBJ_T) void objects_point_ids_kernel(const uint16_t* __restrict__ heat, int64_t n, int Q, const float* __restrict__ thr,
                                                                  const int32_t* __restrict__ inv, const int4* __restrict__ coords,
                                                                  const int32_t* __restrict__ label, const int32_t* __restrict__ slot,
                                                                  const uint32_t* __restrict__ item_start, int64_t V, int S, int64_t C, Records R,
                                                                  int32_t* __restrict__ point_object) {
    const int64_t total = n * Q;
    for (int64_t e = int64_t(blockIdx.x) * OBJ_T + threadIdx.x; e < total; e += int64_t(gridDim.x) * OBJ_T) {
        const int64_t p = e / Q;
        const int q = int(e - p * Q);
        int32_t out = -1;
        if (obj_hit(heat[e], thr[q])) {
            const int v = inv[p];
            if (v >= 0 && v < V) {
                int s;
                const int64_t c = obj_component(label, slot, coords, item_start, V, Q, S, q, v, &s);
                if (c >= 0 && c < C) out = R.rank[c];
            }
        }
        point_object[e] = out;
    }
}

struct ObjectsWs {
    size_t label, slot, item_count, item_start, total;
};
static ObjectsWs objects_ws(int64_t V, int S, int Q) {
    ObjectsWs w;
    const size_t words = size_t(Q > 0 ? Q : 1) * size_t(V > 0 ? V : 1);
    const size_t items = size_t(S > 0 ? S : 0) * size_t(Q > 0 ? Q : 1);
    size_t o = 0;
    w.label = o; o += align_up(words * 4, 256);
    w.slot = o; o += align_up(words * 4, 256);
    w.item_count = o; o += align_up((items + 1) * 4, 256);
    w.item_start = o; o += align_up((items + 1) * 4, 256);
    w.total = o;
    return w;
}

}  // namespace osn

using namespace osn;

extern "C" size_t osn_objects_ws_bytes(int64_t n_voxels, int n_scenes, int q) { return objects_ws(n_voxels, n_scenes, q).total; }

extern "C" size_t osn_objects_records_bytes(int64_t n_components) { return records_bytes(n_components); }

static int objects_args(const char* who, int64_t n, int q, int64_t V, int S) {
    OSN_REQUIRE(n >= 0 && n < (int64_t(1) << 22), OSN_E_ARG, "%s: need 0 <= n < 2^22 points per call (n=%lld)", who, (long long)n);
    OSN_REQUIRE(q >= 1 && q <= 1024, OSN_E_ARG, "%s: need 1 <= q <= 1024 (q=%d)", who, q);
    OSN_REQUIRE(V >= 0 && V <= n && int64_t(q) * V < (int64_t(1) << 31), OSN_E_ARG, "%s: need 0 <= n_voxels <= n and q * n_voxels < 2^31 (n_voxels=%lld)",
                who, (long long)V);
    OSN_REQUIRE(S >= 0 && S <= 65535 && int64_t(S) * q < (int64_t(1) << 24), OSN_E_ARG, "%s: n_scenes=%d (0 .. 65535, n_scenes * q < 2^24)", who, S);
    return OSN_OK;
}

extern "C" int osn_objects_label(const void* heat_f16, int64_t n, int q, const float* thresholds, const int32_t* inverse,
                                 const int32_t* coords4, int64_t n_voxels, const int32_t* nbr, int connectivity,
                                 const int64_t* scene_offsets, int n_scenes, int32_t* err, void* ws, size_t ws_bytes,
                                 int64_t* n_components_host, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t V = n_voxels;
    if (int rc = objects_args("osn_objects_label", n, q, V, n_scenes)) return rc;
    OSN_REQUIRE(connectivity == 6 || connectivity == 26, OSN_E_ARG, "osn_objects_label: connectivity=%d (6 or 26)", connectivity);
    OSN_REQUIRE(err && n_components_host && thresholds, OSN_E_ARG, "osn_objects_label: null pointer");
    OSN_REQUIRE(n == 0 || (heat_f16 && inverse), OSN_E_ARG, "osn_objects_label: null pointer");
    OSN_REQUIRE(V == 0 || (coords4 && nbr && aligned16(coords4)), OSN_E_ARG, "osn_objects_label: the voxel rows must be non-null and 16-byte aligned");
    OSN_REQUIRE(n_scenes == 0 || scene_offsets, OSN_E_ARG, "osn_objects_label: null scene_offsets");
    const ObjectsWs w = objects_ws(V, n_scenes, q);
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= w.total, OSN_E_WS, "osn_objects_label: workspace too small (%zu < %zu)", ws_bytes, w.total);
    char* p = static_cast<char*>(ws);
    int32_t* label = reinterpret_cast<int32_t*>(p + w.label);
    int32_t* slot = reinterpret_cast<int32_t*>(p + w.slot);
    uint32_t* item_count = reinterpret_cast<uint32_t*>(p + w.item_count);
    uint32_t* item_start = reinterpret_cast<uint32_t*>(p + w.item_start);
    const int64_t items = int64_t(n_scenes) * q;
    const int64_t words = int64_t(q) * V;
    OSN_HIP(hipMemsetAsync(err, 0, 4, st));
    OSN_HIP(hipMemsetAsync(item_count, 0, size_t(items + 1) * 4, st));
    if (words > 0) {
        OSN_HIP(hipMemsetAsync(label, 0xFF, size_t(words) * 4, st));
        OSN_HIP(hipMemsetAsync(slot, 0xFF, size_t(words) * 4, st));
    }
    if (n_scenes > 0)
        hipLaunchKernelGGL(objects_check_kernel, dim3(unsigned(cdiv(n_scenes, 256))), dim3(256), 0, st, scene_offsets, n_scenes, n, err);
    if (n > 0 && words > 0 && n_scenes > 0) {
        const int4* c4 = reinterpret_cast<const int4*>(coords4);
        hipLaunchKernelGGL(objects_activate_kernel, dim3(components_grid(n * q)), dim3(OBJ_T), 0, st, static_cast<const uint16_t*>(heat_f16), n, q,
                           thresholds, inverse, V, label, err);
        hipLaunchKernelGGL(objects_unite_kernel, dim3(components_grid(words)), dim3(OBJ_T), 0, st, label, nbr, V, q, connectivity, err);
        hipLaunchKernelGGL(objects_flatten_kernel, dim3(components_grid(words)), dim3(OBJ_T), 0, st, label, V, q);
        hipLaunchKernelGGL(objects_number_kernel, dim3(components_grid(words)), dim3(OBJ_T), 0, st, label, c4, V, q, n_scenes, item_count, slot, err);
    }
    hipLaunchKernelGGL(objects_scan_kernel, dim3(1), dim3(OBJ_T), 0, st, item_count, items, item_start);
    OSN_LAUNCH_CHECK();
    uint32_t total = 0;
    int32_t h = 0;
    OSN_HIP(hipMemcpyAsync(&total, item_start + items, 4, hipMemcpyDeviceToHost, st));
    OSN_HIP(hipMemcpyAsync(&h, err, 4, hipMemcpyDeviceToHost, st));
    OSN_HIP(hipStreamSynchronize(st));
    OSN_REQUIRE(!(h & OBJ_E_OFFSETS), OSN_E_ARG, "osn_objects_label: scene_offsets must start at 0, ascend and end at n");
    OSN_REQUIRE(!(h & OBJ_E_INVERSE), OSN_E_ARG, "osn_objects_label: a point's voxel row outside [0, n_voxels)");
    OSN_REQUIRE(!(h & OBJ_E_SCENE), OSN_E_ARG, "osn_objects_label: a voxel's batch column outside [0, n_scenes)");
    OSN_REQUIRE(!(h & OBJ_E_NBR), OSN_E_ARG, "osn_objects_label: a neighbour row outside [-1, n_voxels)");
    *n_components_host = int64_t(total);
    return OSN_OK;
}

extern "C" int osn_objects_find(const void* heat_f16, const float* xyz, int64_t n, int q, const float* thresholds,
                                const int32_t* inverse, const int32_t* coords4, int64_t n_voxels, const int64_t* scene_offsets,
                                int n_scenes, int64_t n_components, int min_points, int max_objects, int combine,
                                int64_t* out_n_points, int64_t* out_n_voxels, void* out_peak_score_f16, int64_t* out_peak_point,
                                int64_t* out_score_sum, int64_t* out_vox_sum, float* out_box_min, float* out_box_max,
                                int64_t* out_n_objects, int32_t* point_object, const void* ws, size_t ws_bytes, void* records,
                                size_t records_bytes_given, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t V = n_voxels, C = n_components;
    if (int rc = objects_args("osn_objects_find", n, q, V, n_scenes)) return rc;
    OSN_REQUIRE(max_objects >= 1 && max_objects <= OBJ_MAX_M && min_points >= 1, OSN_E_ARG,
                "osn_objects_find: max_objects=%d (1 .. %d) min_points=%d (>= 1)", max_objects, OBJ_MAX_M, min_points);
    OSN_REQUIRE(C >= 0 && C <= int64_t(q) * V, OSN_E_ARG, "osn_objects_find: n_components=%lld outside [0, q * n_voxels]", (long long)C);
    const ObjectsWs w = objects_ws(V, n_scenes, q);
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= w.total, OSN_E_WS, "osn_objects_find: workspace too small (%zu < %zu)", ws_bytes, w.total);
    OSN_REQUIRE(records && aligned16(records) && records_bytes_given >= records_bytes(C), OSN_E_WS,
                "osn_objects_find: record buffer too small (%zu < %zu)", records_bytes_given, records_bytes(C));
    OSN_REQUIRE(thresholds && (n == 0 || (heat_f16 && xyz && inverse)) && (V == 0 || (coords4 && aligned16(coords4))), OSN_E_ARG,
                "osn_objects_find: null or misaligned input");
    if (n_scenes == 0) return OSN_OK;
    OSN_REQUIRE(scene_offsets && out_n_points && out_n_voxels && out_peak_score_f16 && out_peak_point && out_score_sum && out_vox_sum &&
                    out_box_min && out_box_max && out_n_objects, OSN_E_ARG, "osn_objects_find: null output");
    const char* p = static_cast<const char*>(ws);
    const int32_t* label = reinterpret_cast<const int32_t*>(p + w.label);
    const int32_t* slot = reinterpret_cast<const int32_t*>(p + w.slot);
    const uint32_t* item_start = reinterpret_cast<const uint32_t*>(p + w.item_start);
    const Records R = records_at(records, C);
    const int4* c4 = reinterpret_cast<const int4*>(coords4);
    const uint16_t* heat = static_cast<const uint16_t*>(heat_f16);
    const int64_t words = int64_t(q) * V;
    if (C > 0) {
        hipLaunchKernelGGL(objects_preset_kernel, dim3(unsigned(cdiv(C, 256))), dim3(256), 0, st, R, C);
        hipLaunchKernelGGL(objects_voxels_kernel, dim3(components_grid(words)), dim3(OBJ_T), 0, st, label, slot, c4, item_start, V, q, n_scenes, C, R);
        const dim3 grid(unsigned(cdiv(n, OBJ_T)));
        if (combine)
            hipLaunchKernelGGL(objects_reduce_kernel<true>, grid, dim3(OBJ_T), 0, st, heat, xyz, n, q, thresholds, inverse, c4, scene_offsets,
                               label, slot, item_start, V, n_scenes, C, R);
        else
            hipLaunchKernelGGL(objects_reduce_kernel<false>, grid, dim3(OBJ_T), 0, st, heat, xyz, n, q, thresholds, inverse, c4, scene_offsets,
                               label, slot, item_start, V, n_scenes, C, R);
    }
    ObjOut O;
    O.n_points = out_n_points; O.n_voxels = out_n_voxels; O.peak_score = static_cast<uint16_t*>(out_peak_score_f16);
    O.peak_point = out_peak_point; O.score_sum = out_score_sum; O.vox_sum = out_vox_sum; O.box_min = out_box_min; O.box_max = out_box_max;
    O.n_objects = out_n_objects;
    hipLaunchKernelGGL(objects_select_kernel, dim3(unsigned(int64_t(n_scenes) * q)), dim3(OBJ_T), 0, st, item_start, R, C, q, heat, scene_offsets,
                       n, uint32_t(min_points), max_objects, O);
    if (point_object && n > 0)
        hipLaunchKernelGGL(objects_point_ids_kernel, dim3(components_grid(n * q)), dim3(OBJ_T), 0, st, heat, n, q, thresholds, inverse, c4, label, slot,
                           item_start, V, n_scenes, C, R, point_object);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
