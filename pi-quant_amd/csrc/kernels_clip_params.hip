// Instantiation and launch of the histogram clip search for per-tensor parameters (clip_params_kernels.hpp): the histogram pass with its fold, the
// search and the choice -- the twentieth kernel unit, on the same flags (-ffp-contract=off: every step of a candidate's error is rounded on its own).
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "clip_params_kernels.hpp"
#include "piquant_hip.h"
#include "tuning.hpp"

#include <algorithm>

namespace pq {

static_assert(kClipBins == PIQUANT_HIP_CLIP_BINS && kClipMaxSteps == PIQUANT_HIP_CLIP_MAX_STEPS, "the header's constants");

size_t clip_partial_rows(int num_cu) { return static_cast<size_t>(std::max(num_cu, 1)) * kClipHistBlocksPerCU; }
size_t clip_partial_bytes(int num_cu) { return clip_partial_rows(num_cu) * kClipBins * sizeof(uint32_t); }

namespace {

template <int DT_IN>
uint32_t clip_histogram_t(const void* in, int64_t numel, const int32_t* keys, uint32_t* partials, size_t rows, hipStream_t stream) {
    constexpr int EPV = InVec<DT_IN>::EPV, ESIZE = DT_IN == DT_F32 ? 4 : 2;
    const int vectors = reinterpret_cast<uintptr_t>(in) % ESIZE == 0 ? 1 : 0;   // not even element-aligned: element by element
    int head = 0;
    if (vectors) {   // the scan's rule: start at the next 16-byte boundary, block 0 counts the few elements in front of it
        head = static_cast<int>(std::min<int64_t>(static_cast<int64_t>((16u - (reinterpret_cast<uintptr_t>(in) & 15u)) & 15u) / ESIZE, numel));
        in = static_cast<const uint8_t*>(in) + static_cast<int64_t>(head) * ESIZE;
        numel -= head;
    }
    const int64_t per_block = static_cast<int64_t>(kClipHistBlock) * (vectors ? kClipHistU * EPV : 1);
    const int64_t grid = std::max<int64_t>(std::min<int64_t>((numel + per_block - 1) / per_block, static_cast<int64_t>(rows)), 1);
    // a block's counts are 32 bits wide: its share, head included, stays below 2^32 elements
    if ((numel + grid - 1) / grid + kClipHistBlock * kClipHistU * EPV + 16 >= (int64_t {1} << 32))
        panic("clip_histogram: %lld elements over %lld blocks overflow a block's 32-bit counts", static_cast<long long>(numel), static_cast<long long>(grid));
    hipLaunchKernelGGL((clip_histogram_kernel<DT_IN, kClipHistU, kMinmaxNT, kClipHistBlock, kClipHistGlobalAdds>), dim3(static_cast<unsigned>(grid)), dim3(kClipHistBlock), 0,
                       stream, in, numel, keys, partials, head, static_cast<uint32_t>(grid), vectors);
    return static_cast<uint32_t>(grid);
}

}  // namespace

void launch_clip_histogram(const void* in, int dt_in, int64_t numel, const int32_t* keys, uint32_t* partials, size_t partial_rows, uint64_t* hist, bool init,
                           hipStream_t stream) {
    uint32_t rows = 0;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "count words");
    if (kClipHistGlobalAdds) {   // the blocks add to the caller's counts themselves: zero them first where asked, no fold behind
        if (init) hipLaunchKernelGGL(clip_fold_kernel, dim3(kClipBins / kClipFoldBins), dim3(kClipFoldBlock), 0, stream, partials, 0u, reinterpret_cast<unsigned long long*>(hist), 1);
        partials = reinterpret_cast<uint32_t*>(hist);
    }
    if (numel > 0) {
        if (partial_rows < 1) panic("clip_histogram: no scratch rows");
        switch (dt_in) {
            case DT_F32: rows = clip_histogram_t<DT_F32>(in, numel, keys, partials, partial_rows, stream); break;
            case DT_BF16: rows = clip_histogram_t<DT_BF16>(in, numel, keys, partials, partial_rows, stream); break;
            default: panic("clip_histogram needs a float dtype, got %d", dt_in);
        }
    } else if (!init) {
        return;   // nothing to count, nothing to zero
    }
    if (!kClipHistGlobalAdds)
        hipLaunchKernelGGL(clip_fold_kernel, dim3(kClipBins / kClipFoldBins), dim3(kClipFoldBlock), 0, stream, partials, rows, reinterpret_cast<unsigned long long*>(hist),
                           init ? 1 : 0);
    PQ_HIP(hipGetLastError());
}

void launch_clip_search(const int32_t* keys, const uint64_t* hist, int bits, int steps, double* errors_scratch, void* device_param_record, int32_t* device_choice,
                        double* device_errors, hipStream_t stream) {
    if (steps < 1 || steps > kClipMaxSteps) panic("clip search: %d steps, 1 to %d are possible", steps, kClipMaxSteps);
    if (steps > 1)
        hipLaunchKernelGGL(clip_search_kernel, dim3(steps), dim3(kClipSearchBlock), 0, stream, keys, reinterpret_cast<const unsigned long long*>(hist), bits, errors_scratch);
    hipLaunchKernelGGL(clip_choose_kernel, dim3(1), dim3(64), 0, stream, keys, errors_scratch, bits, steps, static_cast<ParamRecord*>(device_param_record), device_choice,
                       device_errors);
    PQ_HIP(hipGetLastError());
}

void launch_clip_unsearched(int32_t* device_choice, double* device_errors, hipStream_t stream) {
    if (!device_choice && !device_errors) return;
    hipLaunchKernelGGL(clip_unsearched_kernel, dim3(1), dim3(64), 0, stream, device_choice, device_errors);
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
