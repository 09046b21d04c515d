// Internal entry points of coords.hip for the batched map builder (maps.hip): the same launches as the extern "C" functions, with the
// option of leaving out their memsets ("prefilled": osn_maps_build clears the regions of ALL its jobs with one launch, fill_batch).
#pragma once
#include "common.h"

namespace osn {

// Regions a launch presets: byte pattern `value` over [ptr, ptr + bytes); ptr and bytes multiples of 4.
struct FillJob {
    void* ptr;
    uint64_t bytes;
    uint32_t value;          // the byte, replicated (0x00000000 / 0xFFFFFFFF / 0x7F7F7F7F)
    uint32_t pad;
};
constexpr int FILL_BATCH = 48;
struct FillJobs {
    FillJob j[FILL_BATCH];
};
// every job of `jobs[0 .. n)` in ONE launch per FILL_BATCH jobs (n == 0: nothing)
int fill_batch(const FillJob* jobs, int n, hipStream_t st);

int kmap_build_impl(const uint64_t* in_table_keys, const int32_t* in_table_vals, int64_t cap, const int32_t* out_coords4, int64_t n_out,
                    int ksize, int offset_scale, int32_t* nbr, int64_t* counts, bool prefilled, hipStream_t st);
int kmap_build_self_impl(const uint64_t* table_keys, const int32_t* table_vals, int64_t cap, const int32_t* coords4, int64_t n, int ksize,
                         int offset_scale, int32_t* nbr, int64_t* counts, bool prefilled, hipStream_t st);
// The self map of the odd kernel `ksize` from the finished self map of the wider odd kernel `ksize_big` over the same rows with the
// same offset scale: its offsets are a subset of the wider map's, so its K rows (and counts; counts_big may be null only if counts
// is) are copies.  Writes every entry of nbr and counts: needs no preset.
int kmap_derive_self_impl(const int32_t* nbr_big, const int64_t* counts_big, int ksize_big, int64_t n, int ksize, int32_t* nbr,
                          int64_t* counts, hipStream_t st);
// ---- block occupancy of a level: a second open-addressing table over the 4^3 blocks of the level's cells.  Cell (x', y', z') =
// coordinate / scale (the level's rows are multiples of its tensor stride); key = pack_key(batch, x' >> 2, y' >> 2, z' >> 2), value =
// one 64-bit word with bit (x' & 3) + 4 (y' & 3) + 16 (z' & 3) set for every row.  A self map of a 3^3 / 5^3 kernel looks up the
// few block words around a row and probes the hash table only where a bit is set.  Buffer: [bad flag, 256 bytes][words][keys];
// *bad != 0: some row is no multiple of `scale` (or outside the packable range) -- the builder then probes every offset.
struct OccView {
    int32_t* bad;
    unsigned long long* words;
    uint64_t* keys;
    int64_t cap;             // power of two >= 2 * rows (there are at most `rows` blocks)
    size_t bytes;
};
inline int64_t occ_capacity(int64_t rows) {
    int64_t cap = 1024;
    while (cap < 2 * rows) cap <<= 1;
    return cap;
}
inline OccView occ_view(void* base, int64_t rows) {
    OccView v;
    char* p = static_cast<char*>(base);
    v.cap = occ_capacity(rows);
    v.bad = reinterpret_cast<int32_t*>(p);
    v.words = reinterpret_cast<unsigned long long*>(p + 256);
    v.keys = reinterpret_cast<uint64_t*>(p + 256 + size_t(v.cap) * 8);
    v.bytes = 256 + size_t(v.cap) * 16;
    return v;
}
// the table of `n` rows (buffer preset: flag and words zero, keys 0xFF), one launch
int occ_fill_impl(const OccView& occ, const int32_t* coords4, int64_t n, int scale, hipStream_t st);
// osn_kmap_build_self (ksize 3 or 5, counts and the table's upper half preset) probing only the occupied cells
int kmap_build_self_occ_impl(const uint64_t* table_keys, const int32_t* table_vals, int64_t cap, const OccView& occ,
                             const int32_t* coords4, int64_t n, int ksize, int offset_scale, int32_t* nbr, int64_t* counts,
                             hipStream_t st);
// osn_maps_set_legacy: the launch sequence of the earlier rounds (maps.hip)
bool maps_legacy();
int kmap_transpose_impl(const int32_t* nbr, int64_t n_out, int K, int64_t n_in, int32_t* tbl, bool prefilled, hipStream_t st);

}  // namespace osn
