// Worst error, in ulps of the exact result, of the device's expf and log1pf on the argument ranges the segmentation head
// (csrc/seg.hip) uses them on: expf(v - max) on [-104, 0], log1pf(s1) on [0, 255] and down to 1e-30.  The reference is
// the host's long-double expl / log1pl of the same fp32 argument.  tests/seg_bounds.py takes E_EXP and E_LOG1P from the
// printed figures (twice the worst, rounded up, at least 2).
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wall -DNDEBUG tools/probe_libm.hip -o tools/probes/bin/probe_libm
//     tools/probes/bin/probe_libm                      (the optimisation flags of openscene_amd/build.py; a few seconds)
//
// A result below FLT_MIN is measured in units of 2^-149, the spacing of the denormals, and reported on its own line.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));          \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)

__global__ void eval_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int fn) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    y[i] = fn == 0 ? expf(x[i]) : log1pf(x[i]);
}

struct Worst {
    double ulps = 0, at = 0;          // results that are normal fp32 numbers
    double sub = 0, sub_at = 0;       // results below FLT_MIN, in units of 2^-149
    int64_t bad = 0;                  // NaN or infinite results
};

static Worst measure(const std::vector<float>& x, int fn) {
    const int64_t n = int64_t(x.size());
    float *dx = nullptr, *dy = nullptr;
    CHECK(hipMalloc(&dx, n * sizeof(float)));
    CHECK(hipMalloc(&dy, n * sizeof(float)));
    CHECK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, dx, dy, n, fn);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<float> y(n);
    CHECK(hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    CHECK(hipFree(dx));
    CHECK(hipFree(dy));
    Worst w;
    for (int64_t i = 0; i < n; ++i) {
        const long double ref = fn == 0 ? expl((long double)x[i]) : log1pl((long double)x[i]);
        if (!std::isfinite(y[i])) { ++w.bad; continue; }
        const long double err = fabsl((long double)y[i] - ref);
        if (ref < (long double)FLT_MIN) {
            const double u = double(err / ldexpl(1.0L, -149));
            if (u > w.sub) { w.sub = u; w.sub_at = x[i]; }
        } else {
            int e;
            frexpl(ref, &e);                                   // ref = f 2^e, f in [0.5, 1): ulp = 2^(e - 24)
            const double u = double(err / ldexpl(1.0L, e - 24));
            if (u > w.ulps) { w.ulps = u; w.at = x[i]; }
        }
    }
    return w;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main() {
    int rt = 0, dev_count = 0;
    CHECK(hipGetDeviceCount(&dev_count));
    CHECK(hipRuntimeGetVersion(&rt));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    std::printf("device %s  HIP %d.%d.%d  runtime %d\n", prop.gcnArchName, HIP_VERSION_MAJOR, HIP_VERSION_MINOR, HIP_VERSION_PATCH, rt);

    // expf: every multiple of 2^-15 in [-104, 0], and as many pseudo-random fp32 values of the same range (full mantissas)
    std::vector<float> x;
    const int64_t steps = int64_t(104) << 15;
    x.reserve(size_t(2 * steps + 2));
    for (int64_t i = 0; i <= steps; ++i) x.push_back(-float(i) * 0x1p-15f);
    uint32_t s = 12345u;
    for (int64_t i = 0; i < steps; ++i) x.push_back(-104.f * (float(lcg(s) >> 8) * 0x1p-24f) * (1.f + float(lcg(s) >> 9) * 0x1p-46f));
    Worst w = measure(x, 0);
    std::printf("expf   [-104, 0]  %lld arguments  worst %.4f ulp at %.9g   denormal results: worst %.4f x 2^-149 at %.9g   non-finite %lld\n",
                (long long)x.size(), w.ulps, w.at, w.sub, w.sub_at, (long long)w.bad);

    // log1pf: every multiple of 2^-14 in [0, 255], pseudo-random values of the range, and a logarithmic grid 1e-30 .. 1
    x.clear();
    const int64_t lsteps = int64_t(255) << 14;
    for (int64_t i = 0; i <= lsteps; ++i) x.push_back(float(i) * 0x1p-14f);
    for (int64_t i = 0; i < lsteps; ++i) x.push_back(255.f * (float(lcg(s) >> 8) * 0x1p-24f));
    Worst wl = measure(x, 1);
    std::printf("log1pf [0, 255]   %lld arguments  worst %.4f ulp at %.9g   non-finite %lld\n", (long long)x.size(), wl.ulps, wl.at,
                (long long)wl.bad);
    x.clear();
    const int64_t gsteps = int64_t(1) << 21;
    for (int64_t i = 0; i <= gsteps; ++i) x.push_back(float(std::pow(10.0, -30.0 + 30.0 * double(i) / double(gsteps))));
    Worst wg = measure(x, 1);
    std::printf("log1pf [1e-30, 1] %lld arguments  worst %.4f ulp at %.9g   non-finite %lld\n", (long long)x.size(), wg.ulps, wg.at,
                (long long)wg.bad);
    std::printf("E_EXP measured %.4f  E_LOG1P measured %.4f\n", w.ulps, wl.ulps > wg.ulps ? wl.ulps : wg.ulps);
    return 0;
}
