// Every kernel map of a scene from ONE call, on several streams.
//
// Replaces the Python-level walk over [ME] CoordinateManager.kernel_map for the convolutions of a MinkUNet forward
// (models/mink_unet.py:47-113: one 5^3 map, five 3^3 maps, four 2^3 stride-2 maps and their transposes), i.e. what
// CoordinateManager.prebuild issued as ~90 separate C-ABI calls: per map the neighbour table (+ per-offset pair counts),
// the transposed table of a strided map, the tile-ordered copies, the tile lists and the pair lists.  The maps of
// different pyramid levels do not depend on each other, and each is a chain of latency-bound launches that leaves most of
// the chip idle -- so the chains are dealt to up to OSN_MAPS_MAX_STREAMS streams (fork after the pyramid, join at the end;
// nothing outside sees the extra streams).  Host-only code: it calls the library's own entry points, so every table is
// bit for bit what the per-map calls produce.
#include "common.h"
#include "events.h"
#include "coords_impl.h"
#include <atomic>
#include <vector>

using namespace osn;

// osn_maps_set_legacy: every self map probed, pair_plan_kernel a launch of its own (tests, A/B)
static std::atomic<int> g_maps_legacy{0};
bool osn::maps_legacy() { return g_maps_legacy.load(std::memory_order_relaxed) != 0; }
extern "C" int osn_maps_set_legacy(int on) { return g_maps_legacy.exchange(on ? 1 : 0); }

extern "C" size_t osn_maps_occupancy_bytes(int64_t rows) { return occ_view(nullptr, rows > 0 ? rows : 1).bytes; }

extern "C" int osn_maps_build(const osn_map_level* levels, int n_levels, const osn_map_job* jobs, int n_jobs,
                              const osn_stream_t* streams, void* const* ws, const uint64_t* ws_bytes, int n_streams,
                              osn_events_t* events) {
    return osn_maps_build_occ(levels, n_levels, jobs, n_jobs, streams, ws, ws_bytes, n_streams, events, nullptr);
}

extern "C" int osn_maps_build_occ(const osn_map_level* levels, int n_levels, const osn_map_job* jobs, int n_jobs,
                                  const osn_stream_t* streams, void* const* ws, const uint64_t* ws_bytes, int n_streams,
                                  osn_events_t* events, void* const* occ) {
    OSN_REQUIRE(levels && jobs && streams && ws && ws_bytes && n_levels >= 1 && n_jobs >= 0 && n_streams >= 1 &&
                    n_streams <= OSN_MAPS_MAX_STREAMS,
                OSN_E_ARG, "osn_maps_build: bad arguments (%d levels, %d jobs, %d streams)", n_levels, n_jobs, n_streams);
    OSN_REQUIRE(n_streams == 1 || (events && events_count(events) >= n_streams + 1), OSN_E_ARG,
                "osn_maps_build: %d streams need an event pool of at least %d events", n_streams, n_streams + 1);
    hipStream_t main = static_cast<hipStream_t>(streams[0]);
    // A 3^3 self map behind a 5^3 self map of the same level and scale is 27 of that table's 125 rows: from[j] = the 5^3 job it is
    // copied from (on that job's stream, behind it; no probe, no preset), -1 = built by probing
    std::vector<int> from(size_t(n_jobs > 0 ? n_jobs : 0), -1);
    if (!maps_legacy())
        for (int j = 0; j < n_jobs; ++j) {
            const osn_map_job& q = jobs[j];
            if (!q.self_map || q.ksize != 3 || !q.nbr_fwd) continue;
            for (int i = 0; i < j && from[j] < 0; ++i) {
                const osn_map_job& b = jobs[i];
                if (b.self_map && b.ksize == 5 && b.lvl_in == q.lvl_in && b.lvl_out == q.lvl_out && b.scale == q.scale && b.nbr_fwd &&
                    (b.counts || !q.counts) && b.lvl_in >= 0 && b.lvl_in < n_levels && b.lvl_in == b.lvl_out)
                    from[j] = i;
            }
        }
    // Block occupancy: a level whose occ[] buffer is given gets its table from the first probed 3^3 / 5^3 self map of the level, on
    // that job's stream in front of it; occ_job[l] = that job.  Self maps of the level with the same scale on the same stream read
    // it too; any other job probes every offset as before.
    std::vector<int> occ_job(size_t(n_levels), -1);
    auto lane_of = [&](const osn_map_job& q) { return q.stream >= 0 && q.stream < n_streams ? q.stream : 0; };
    auto occ_source = [&](int j) -> int {            // the job whose occupancy table job j reads, -1: none
        const osn_map_job& q = jobs[j];
        if (!occ || maps_legacy() || from[j] >= 0 || !q.self_map || (q.ksize != 3 && q.ksize != 5) || !q.nbr_fwd || q.scale < 1 ||
            q.lvl_in < 0 || q.lvl_in >= n_levels || q.lvl_in != q.lvl_out || !occ[q.lvl_in] || levels[q.lvl_in].rows < 1)
            return -1;
        const int s = occ_job[size_t(q.lvl_in)];
        if (s < 0) return j;
        return jobs[s].scale == q.scale && lane_of(jobs[s]) == lane_of(q) ? s : -1;
    };
    // Round 6: what the per-map entry points preset with one hipMemsetAsync each (pair counts: zero; the upper half of a self map's
    // table and a transposed table: -1) is cleared for ALL jobs by one launch in front of the fork (~20 launches of 3 - 8 us per scene)
    {
        std::vector<FillJob> fills;
        for (int j = 0; j < n_jobs; ++j) {
            if (occ_source(j) != j) continue;
            occ_job[size_t(jobs[j].lvl_in)] = j;
            const OccView v = occ_view(occ[jobs[j].lvl_in], levels[jobs[j].lvl_in].rows);
            fills.push_back(FillJob{v.bad, 256u + uint64_t(v.cap) * 8u, 0u, 0u});                    // flag and words
            fills.push_back(FillJob{v.keys, uint64_t(v.cap) * 8u, 0xFFFFFFFFu, 0u});
        }
        for (int j = 0; j < n_jobs; ++j) {
            const osn_map_job& q = jobs[j];
            if (from[j] >= 0) continue;
            if (q.lvl_in < 0 || q.lvl_in >= n_levels || q.lvl_out < 0 || q.lvl_out >= n_levels || q.ksize < 1 || q.ksize > 7 || !q.nbr_fwd) continue;
            const int K = q.ksize * q.ksize * q.ksize;
            const int64_t n_in = levels[q.lvl_in].rows;
            if (q.counts) fills.push_back(FillJob{q.counts, uint64_t(K) * 8u, 0u, 0u});
            if (q.self_map) {
                if (K > 1 && n_in > 0) fills.push_back(FillJob{q.nbr_fwd + int64_t(K / 2 + 1) * n_in, uint64_t(K / 2) * uint64_t(n_in) * 4u, 0xFFFFFFFFu, 0u});
            } else if (q.nbr_bwd && n_in > 0) {
                fills.push_back(FillJob{q.nbr_bwd, uint64_t(K) * uint64_t(n_in) * 4u, 0xFFFFFFFFu, 0u});
            }
        }
        const int rc = fill_batch(fills.data(), int(fills.size()), main);
        if (rc) return rc;
    }
    // fork: the side streams see the pyramid (coordinates + hash tables) the main stream has queued
    if (n_streams > 1) {
        hipEvent_t e0 = events_get(events, 0);
        OSN_HIP(hipEventRecord(e0, main));
        for (int s = 1; s < n_streams; ++s) OSN_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(streams[s]), e0, 0));
    }
    bool used[OSN_MAPS_MAX_STREAMS] = {false};
    for (int j = 0; j < n_jobs; ++j) {
        const osn_map_job& q = jobs[j];
        OSN_REQUIRE(q.lvl_in >= 0 && q.lvl_in < n_levels && q.lvl_out >= 0 && q.lvl_out < n_levels && q.ksize >= 1 && q.ksize <= 7,
                    OSN_E_ARG, "osn_maps_build: job %d: levels / kernel size", j);
        const osn_map_job& qs = from[j] >= 0 ? jobs[from[j]] : q;          // (a copied table: the stream of its source)
        const int si = qs.stream >= 0 && qs.stream < n_streams ? qs.stream : 0;
        used[si] = true;
        osn_stream_t st = streams[si];
        const osn_map_level& li = levels[q.lvl_in];
        const osn_map_level& lo = levels[q.lvl_out];
        const int K = q.ksize * q.ksize * q.ksize;
        OSN_REQUIRE(q.nbr_fwd && li.rows >= 1 && lo.rows >= 1, OSN_E_ARG, "osn_maps_build: job %d: null table or empty level", j);
        int rc;
        if (q.self_map) {
            OSN_REQUIRE(q.lvl_in == q.lvl_out && (q.ksize & 1), OSN_E_ARG, "osn_maps_build: job %d: a self map needs one level and an odd kernel", j);
            if (from[j] >= 0)
                rc = kmap_derive_self_impl(qs.nbr_fwd, qs.counts, qs.ksize, li.rows, q.ksize, q.nbr_fwd, q.counts, static_cast<hipStream_t>(st));
            else if (const int os = occ_source(j); os >= 0) {
                const OccView v = occ_view(occ[q.lvl_in], li.rows);
                rc = os == j ? occ_fill_impl(v, li.coords4, li.rows, q.scale, static_cast<hipStream_t>(st)) : OSN_OK;
                if (!rc)
                    rc = kmap_build_self_occ_impl(li.keys, li.vals, li.cap, v, li.coords4, li.rows, q.ksize, q.scale, q.nbr_fwd, q.counts,
                                                  static_cast<hipStream_t>(st));
            } else
                rc = kmap_build_self_impl(li.keys, li.vals, li.cap, li.coords4, li.rows, q.ksize, q.scale, q.nbr_fwd, q.counts, true,
                                          static_cast<hipStream_t>(st));
        } else {
            rc = kmap_build_impl(li.keys, li.vals, li.cap, lo.coords4, lo.rows, q.ksize, q.scale, q.nbr_fwd, q.counts, true,
                                 static_cast<hipStream_t>(st));
            if (!rc && q.nbr_bwd) rc = kmap_transpose_impl(q.nbr_fwd, lo.rows, K, li.rows, q.nbr_bwd, true, static_cast<hipStream_t>(st));
        }
        if (rc) return rc;
        // tile-ordered copies (rows sorted by offset-occupancy mask) of the forward / input-gradient tables
        if (q.sorted_fwd) {
            rc = osn_kmap_sort(q.nbr_fwd, lo.rows, K, q.counts, q.order_fwd, q.sorted_fwd, q.gmask_fwd, ws[si], size_t(ws_bytes[si]), st);
            if (rc) return rc;
        }
        if (q.sorted_bwd) {
            OSN_REQUIRE(q.nbr_bwd, OSN_E_ARG, "osn_maps_build: job %d: tile order of a missing input-gradient table", j);
            rc = osn_kmap_sort(q.nbr_bwd, li.rows, K, q.counts, q.order_bwd, q.sorted_bwd, q.gmask_bwd, ws[si], size_t(ws_bytes[si]), st);
            if (rc) return rc;
        }
        // tile lists (of the tile-ordered table where one exists) and the pair lists of the forward lists
        if (q.tl_fwd) {
            rc = osn_tile_lists_build(q.sorted_fwd ? q.sorted_fwd : q.nbr_fwd, lo.rows, K, q.bm_fwd, q.tl_fwd, st);
            if (rc) return rc;
            if (q.pl_fwd) {
                rc = osn_pair_lists_build(q.tl_fwd, q.sorted_fwd ? q.order_fwd : nullptr, lo.rows, K, q.bm_fwd, q.pl_fwd, st);
                if (rc) return rc;
            }
        }
        if (q.tl_bwd) {
            OSN_REQUIRE(q.nbr_bwd, OSN_E_ARG, "osn_maps_build: job %d: tile lists of a missing input-gradient table", j);
            rc = osn_tile_lists_build(q.sorted_bwd ? q.sorted_bwd : q.nbr_bwd, li.rows, K, q.bm_bwd, q.tl_bwd, st);
            if (rc) return rc;
        }
    }
    // join
    for (int s = 1; s < n_streams; ++s) {
        if (!used[s]) continue;
        hipEvent_t e = events_get(events, s);
        OSN_HIP(hipEventRecord(e, static_cast<hipStream_t>(streams[s])));
        OSN_HIP(hipStreamWaitEvent(main, e, 0));
    }
    return OSN_OK;
}
