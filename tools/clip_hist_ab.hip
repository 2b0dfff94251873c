// A/B of the two ways the histogram pass of the per-tensor clip search gives its counts out (csrc/clip_params_kernels.hpp): per-block rows + a fold
// launch against 64-bit integer global adds, both as the library would launch them (the zeroing launch of the global-add form included), interleaved
// in one process on cold rotating inputs at numel 27 264 000, float32 and bfloat16 bit patterns of N(0,1) data.  The counts of the two forms are
// compared before anything is timed.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -amdgpu-kernarg-preload-count=12 -Ipi-quant_amd/csrc -Iinclude tools/clip_hist_ab.hip -o tools/clip_hist_ab
//   tools/clip_hist_ab [rounds]
#define PQ_MINMAX_HELPERS_ONLY
#include "clip_params_kernels.hpp"
#include "tuning.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace pq;

#define CK(e)                                                                     \
    do {                                                                          \
        hipError_t err_ = (e);                                                    \
        if (err_ != hipSuccess) {                                                 \
            std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));        \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

namespace pq {
void check_hip(hipError_t e, const char* what, const char*, int) {
    if (e != hipSuccess) {
        std::fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e));
        std::exit(1);
    }
}
}  // namespace pq

constexpr int64_t kNumel = 27264000;

template <int DT_IN, bool GLOBAL_ADDS>
void pass(const void* x, const int32_t* keys, uint32_t* partials, unsigned rows, unsigned long long* hist, hipStream_t s) {
    if (GLOBAL_ADDS) {
        hipLaunchKernelGGL(clip_fold_kernel, dim3(kClipBins / kClipFoldBins), dim3(kClipFoldBlock), 0, s, partials, 0u, hist, 1);
        hipLaunchKernelGGL((clip_histogram_kernel<DT_IN, kClipHistU, kMinmaxNT, kClipHistBlock, true>), dim3(rows), dim3(kClipHistBlock), 0, s, x, kNumel, keys,
                           reinterpret_cast<uint32_t*>(hist), 0, rows, 1);
    } else {
        hipLaunchKernelGGL((clip_histogram_kernel<DT_IN, kClipHistU, kMinmaxNT, kClipHistBlock, false>), dim3(rows), dim3(kClipHistBlock), 0, s, x, kNumel, keys, partials, 0,
                           rows, 1);
        hipLaunchKernelGGL(clip_fold_kernel, dim3(kClipBins / kClipFoldBins), dim3(kClipFoldBlock), 0, s, partials, rows, hist, 1);
    }
}

template <int DT_IN>
void run(const char* name, const std::vector<float>& host, int rounds, unsigned rows) {
    const size_t esize = DT_IN == DT_F32 ? 4 : 2;
    const int nbuf = static_cast<int>(3.3e9 / (kNumel * esize)) + 1;
    std::vector<uint16_t> half;
    const void* src = host.data();
    if (DT_IN == DT_BF16) {
        half.resize(kNumel);
        for (int64_t i = 0; i < kNumel; ++i) {
            uint32_t u;
            std::memcpy(&u, &host[i], 4);
            half[i] = static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
        src = half.data();
    }
    float lo = 3.4e38f, hi = -3.4e38f;
    for (int64_t i = 0; i < kNumel; ++i) {
        float v = host[i];
        if (DT_IN == DT_BF16) {
            const uint32_t u = static_cast<uint32_t>(half[i]) << 16;
            std::memcpy(&v, &u, 4);
        }
        lo = std::min(lo, v);
        hi = std::max(hi, v);
    }
    const int32_t hkeys[2] = {float_to_key(lo), float_to_key(-hi)};
    std::vector<void*> xs(nbuf);
    for (auto& p : xs) {
        CK(hipMalloc(&p, kNumel * esize));
        CK(hipMemcpy(p, src, kNumel * esize, hipMemcpyHostToDevice));
    }
    int32_t* keys;
    uint32_t* partials;
    unsigned long long *hist_a, *hist_b;
    CK(hipMalloc(reinterpret_cast<void**>(&keys), 8));
    CK(hipMemcpy(keys, hkeys, 8, hipMemcpyHostToDevice));
    CK(hipMalloc(reinterpret_cast<void**>(&partials), static_cast<size_t>(rows) * kClipBins * 4));
    CK(hipMalloc(reinterpret_cast<void**>(&hist_a), kClipBins * 8));
    CK(hipMalloc(reinterpret_cast<void**>(&hist_b), kClipBins * 8));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    pass<DT_IN, false>(xs[0], keys, partials, rows, hist_a, s);
    pass<DT_IN, true>(xs[0], keys, partials, rows, hist_b, s);
    CK(hipStreamSynchronize(s));
    std::vector<unsigned long long> a(kClipBins), b(kClipBins);
    CK(hipMemcpy(a.data(), hist_a, kClipBins * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), hist_b, kClipBins * 8, hipMemcpyDeviceToHost));
    unsigned long long total = 0;
    for (int i = 0; i < kClipBins; ++i) total += a[i];
    if (a != b || total != static_cast<unsigned long long>(kNumel)) {
        std::fprintf(stderr, "%s: the two forms disagree (total %llu)\n", name, total);
        std::exit(1);
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int per_window = 40;
    std::vector<float> us[2];
    int k = 0;
    for (int r = 0; r < rounds; ++r) {
        for (int form = 0; form < 2; ++form) {
            CK(hipEventRecord(e0, s));
            for (int i = 0; i < per_window; ++i, ++k) {
                if (form == 0) pass<DT_IN, false>(xs[k % nbuf], keys, partials, rows, hist_a, s);
                else pass<DT_IN, true>(xs[k % nbuf], keys, partials, rows, hist_b, s);
            }
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            us[form].push_back(ms * 1000.0f / per_window);
        }
    }
    for (int form = 0; form < 2; ++form) {
        std::sort(us[form].begin(), us[form].end());
        std::printf("%-5s %-22s median %7.2f us  (min %7.2f, max %7.2f, %d windows of %d)\n", name, form == 0 ? "rows + fold" : "64-bit global adds",
                    us[form][us[form].size() / 2], us[form].front(), us[form].back(), rounds, per_window);
    }
    for (auto p : xs) CK(hipFree(p));
    CK(hipFree(keys));
    CK(hipFree(partials));
    CK(hipFree(hist_a));
    CK(hipFree(hist_b));
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 7;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const unsigned rows = static_cast<unsigned>(prop.multiProcessorCount) * kClipHistBlocksPerCU;
    std::vector<float> host(kNumel);
    std::mt19937 gen(1);
    std::normal_distribution<float> dist(0.0f, 1.0f);
    for (auto& v : host) v = dist(gen);
    std::printf("numel %lld, %u blocks of %d threads\n", static_cast<long long>(kNumel), rows, kClipHistBlock);
    run<DT_F32>("f32", host, rounds, rows);
    run<DT_BF16>("bf16", host, rounds, rows);
    return 0;
}
