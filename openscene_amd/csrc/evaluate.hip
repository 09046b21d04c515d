// Open-vocabulary evaluation on gfx950: per-point prediction (argmax of the test-repeat vote, or given ids) -> optional
// class mapper -> optional no-feature mask -> one int64 confusion matrix, in one streaming pass.
//
// Replaces run/evaluate.py:397-424 and util/metric.py:9-25:
//     pred_logit = store.float().max(1)[1];  pred_logit = mapper[pred_logit];  pred_logit[~mask] = 256
//     confusion = np.bincount(pred_ids[idxs] * (C + 1) + gt_ids[idxs], ...)      (gt 255 ignored)
// The matrix is (c_out + 1) x c_out, [pred, gt]: rows 0 .. c_out-1 are metric.confusion_matrix, row c_out counts the
// no-feature points (NO_FEATURE_ID = 256) of each gt class.  Every number metric.evaluate prints is a sum over it.
//
// A row of c_in <= 8 G votes lives in a group of G lanes (lane g holds columns g, g + G, ...; one group-wide load is G
// consecutive halves of the row), G per c_in bucket as in seg.hip.  The counts go to an int32 histogram in LDS and are
// added to the global int64 matrix once per workgroup (integer adds: exact in any order), or -- when the histogram does
// not fit or is not wanted -- straight to global memory with int64 atomics.
#include "common.h"

#include <atomic>

namespace osn {

constexpr int EV_PER = 8;                // votes per lane
constexpr int EV_THREADS = 512;
constexpr int EV_NO_FEATURE = 256;       // util/metric.py NO_FEATURE_ID
constexpr int EV_IGNORE = 255;           // util/metric.py UNKNOWN_ID
// An LDS histogram holds (c + 1) * c int32: 103 KB at 160 classes, the most it may take (one workgroup per CU).  hist = -1
// chooses it up to EV_LDS_AUTO_MAX_C classes.  Measured (profiles/r09_micro_eval.jsonl): LDS is faster
// at 20 (17x), 16 and 90 classes (1.13x); global int64 atomics are faster at 128 (1.40x) and 160 (2.9x).
constexpr int EV_LDS_MAX_C = 160;
constexpr int EV_LDS_AUTO_MAX_C = 90;
constexpr int EV_MAX_WG_PER_CU = 4;

// Tensor.max(1)[1] on CPU: the first NaN wins; otherwise the largest value, the lowest column among equal ones
// (-0.0 == +0.0)
__device__ inline bool ev_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// err bits: 1 = a prediction outside the mapper, 2 = a gt outside [0, c_out) that is not 255, 4 = a counted prediction
// outside [0, c_out) that is not 256
template <int G>
__global__ __launch_bounds__(EV_THREADS) void eval_confusion_kernel(const _Float16* __restrict__ votes, const int64_t* __restrict__ ids,
                                                                    int64_t n, int c_in, const int64_t* __restrict__ labels,
                                                                    const int64_t* __restrict__ mapper, int64_t n_map,
                                                                    const uint8_t* __restrict__ has_feature, int c_out,
                                                                    unsigned long long* __restrict__ conf, int hist,
                                                                    int32_t* __restrict__ err) {
    extern __shared__ unsigned int sh_hist[];          // [(c_out + 1) * c_out] when hist
    constexpr int RPI = EV_THREADS / G;                // rows per workgroup and iteration
    const int tid = threadIdx.x, g = tid & (G - 1);
    const int cells = (c_out + 1) * c_out;
    if (hist) {
        for (int i = tid; i < cells; i += EV_THREADS) sh_hist[i] = 0;
        __syncthreads();
    }
    int e = 0;
    for (int64_t j0 = int64_t(blockIdx.x) * RPI; j0 < n; j0 += int64_t(gridDim.x) * RPI) {
        const int64_t j = j0 + tid / G;
        if (j >= n) continue;                          // uniform over a group: the shuffles stay inside live groups
        int64_t pr;
        if (ids) {
            pr = ids[j];
        } else {
            const _Float16* x = votes + j * int64_t(c_in);
            float bv = -INFINITY;
            int bi = 0x7fffffff;
#pragma unroll
            for (int t = 0; t < EV_PER; ++t) {
                const int k = g + G * t;
                if (k < c_in) {
                    const float v = (float)x[k];
                    if (ev_better(v, k, bv, bi)) { bv = v; bi = k; }
                }
            }
#pragma unroll
            for (int m = G / 2; m >= 1; m >>= 1) {
                const float ov = __shfl_xor(bv, m, 64);
                const int oi = __shfl_xor(bi, m, 64);
                if (ev_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            pr = bi;
        }
        if (g != 0) continue;
        bool count = true;
        if (mapper) {
            if (pr < 0 || pr >= n_map) { e |= 1; count = false; }
            else pr = mapper[pr];
        }
        if (has_feature && !has_feature[j]) pr = EV_NO_FEATURE;
        const int64_t y = labels[j];
        if (y == EV_IGNORE) count = false;
        else if (y < 0 || y >= c_out) { e |= 2; count = false; }
        int row = 0;
        if (pr == EV_NO_FEATURE) row = c_out;
        else if (pr >= 0 && pr < c_out) row = int(pr);
        else if (count) { e |= 4; count = false; }
        if (count) {
            const int cell = row * c_out + int(y);
            if (hist) atomicAdd(&sh_hist[cell], 1u);
            else atomicAdd(&conf[cell], 1ull);
        }
    }
    if (e) atomicOr(err, e);
    if (hist) {
        __syncthreads();
        for (int i = tid; i < cells; i += EV_THREADS)
            if (sh_hist[i]) atomicAdd(&conf[i], (unsigned long long)sh_hist[i]);
    }
}

inline int ev_group(int c) {
    return c <= 8 ? 1 : c <= 16 ? 2 : c <= 32 ? 4 : c <= 64 ? 8 : c <= 128 ? 16 : 32;
}

}  // namespace osn

using namespace osn;

extern "C" int osn_eval_confusion(const void* votes_f16, const int64_t* ids, int64_t n, int c_in, const int64_t* labels,
                                  const int64_t* mapper, int64_t n_map, const uint8_t* has_feature, int c_out,
                                  int64_t* confusion, int32_t* err, int hist, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 0 && n <= (int64_t(1) << 31) && c_out >= 1 && c_out < EV_IGNORE && hist >= -1 && hist <= 1, OSN_E_ARG,
                "osn_eval_confusion: n=%lld c_out=%d hist=%d (needs n <= 2^31, 1 <= c_out <= 254, hist in {-1, 0, 1})",
                (long long)n, c_out, hist);
    OSN_REQUIRE(confusion && err, OSN_E_ARG, "osn_eval_confusion: null pointer");
    if (n == 0) return OSN_OK;                    // (an empty tensor's pointer may be null)
    OSN_REQUIRE((votes_f16 != nullptr) != (ids != nullptr), OSN_E_ARG, "osn_eval_confusion: give exactly one of votes and ids");
    OSN_REQUIRE(!votes_f16 || (c_in >= 1 && c_in <= 8 * 32), OSN_E_ARG, "osn_eval_confusion: c_in=%d (1 .. 256 votes per row)", c_in);
    OSN_REQUIRE(!mapper || n_map >= 1, OSN_E_ARG, "osn_eval_confusion: empty mapper");
    OSN_REQUIRE(labels, OSN_E_ARG, "osn_eval_confusion: null labels");
    const int G = votes_f16 ? ev_group(c_in) : 1;
    const size_t hist_bytes = size_t(c_out + 1) * c_out * 4;
    const bool use_lds = hist == 1 || (hist == -1 && c_out <= EV_LDS_AUTO_MAX_C);
    // compute units of the current device, queried once per device (the grid is a few workgroups per CU)
    static std::atomic<int> cu_cache[64];
    int dev_id = 0;
    OSN_HIP(hipGetDevice(&dev_id));
    const bool dev_slot_ok = dev_id >= 0 && dev_id < 64;
    int cus = dev_slot_ok ? cu_cache[dev_id].load(std::memory_order_relaxed) : 0;
    if (cus <= 0) {
        OSN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id));
        if (cus <= 0) cus = 256;
        if (dev_slot_ok) cu_cache[dev_id].store(cus, std::memory_order_relaxed);
    }
    const int64_t want = cdiv(n, EV_THREADS / G);
    const int64_t cap = int64_t(cus) * EV_MAX_WG_PER_CU;
    const unsigned grid = unsigned(want < cap ? want : cap);
    unsigned long long* conf = reinterpret_cast<unsigned long long*>(confusion);
    const _Float16* v = static_cast<const _Float16*>(votes_f16);
    const size_t smem = use_lds ? hist_bytes : 0;
#define OSN_EV(G_)                                                                                                          \
    do {                                                                                                                   \
        auto kern = eval_confusion_kernel<G_>;                                                                             \
        if (smem > 65536) {                         /* the dynamic-LDS opt-in beyond 64 KB, once per (instance, device) */ \
            static std::atomic<signed char> attr_state[64];                                                                \
            signed char stt = dev_slot_ok ? attr_state[dev_id].load(std::memory_order_relaxed) : 0;                        \
            if (stt == 0) {                                                                                                \
                stt = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                          int(size_t(EV_LDS_MAX_C + 1) * EV_LDS_MAX_C * 4)) == hipSuccess ? 1 : -1;        \
                if (dev_slot_ok) attr_state[dev_id].store(stt, std::memory_order_relaxed);                                 \
            }                                                                                                              \
            OSN_REQUIRE(stt > 0, OSN_E_HIP, "osn_eval_confusion: the device refused %zu bytes of LDS", smem);              \
        }                                                                                                                  \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(EV_THREADS), smem, st, v, ids, n, c_in, labels, mapper, n_map,           \
                           has_feature, c_out, conf, int(use_lds), err);                                                   \
    } while (0)
    OSN_REQUIRE(!use_lds || c_out <= EV_LDS_MAX_C, OSN_E_ARG, "osn_eval_confusion: an LDS histogram takes at most %d classes",
                EV_LDS_MAX_C);
    switch (G) {
        case 1: OSN_EV(1); break;
        case 2: OSN_EV(2); break;
        case 4: OSN_EV(4); break;
        case 8: OSN_EV(8); break;
        case 16: OSN_EV(16); break;
        default: OSN_EV(32); break;
    }
#undef OSN_EV
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

// 0 = fine, else OSN_E_ARG with the error bits spelled out (synchronises the stream)
extern "C" int osn_eval_check(const int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_eval_check: null pointer");
    int32_t h = 0;
    OSN_HIP(hipMemcpyAsync(&h, err, 4, hipMemcpyDeviceToHost, st));
    OSN_HIP(hipStreamSynchronize(st));
    OSN_REQUIRE(!(h & 1), OSN_E_ARG, "osn_eval_confusion: a prediction outside the class mapper (mapper[...] raises in the reference)");
    OSN_REQUIRE(!(h & 2), OSN_E_ARG, "osn_eval_confusion: a gt label outside [0, C) that is not 255");
    OSN_REQUIRE(!(h & 4), OSN_E_ARG, "osn_eval_confusion: a prediction outside [0, C) that is not 256 (no feature)");
    return OSN_OK;
}
