// Instantiation and launch of the error-feedback group-wise quantize (grouped_kernels.hpp: quantize_grouped_ef_kernel, its batch and its
// guarded form).  A translation unit of its own: its instances compile next to kernels.hip and kernels_grouped.hip.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

struct EfFamily {
    static constexpr const char* name = "quantize_grouped_ef";
    template <class F>
    static void with_pipeline_type(int dt_in, F&& f) {
        with_float_type(dt_in, f);
    }
    template <int DT_IN, int BITS, int MODE, int G>
    static auto single() {
        return &quantize_grouped_ef_kernel<DT_IN, BITS, MODE, G>;
    }
    template <int DT_IN, int BITS, int MODE, int G>
    static auto batch() {
        return &quantize_grouped_ef_batch_kernel<DT_IN, BITS, MODE, G>;
    }
    template <int DT_IN, int BITS, int MODE>
    static auto guarded() {
        return &quantize_grouped_ef_scalar_kernel<DT_IN, BITS, MODE>;
    }
};

}  // namespace

void launch_quantize_grouped_ef_batch(const GroupedEfBatchLaunch& b, hipStream_t stream) { launch_grouped_ef_batch<EfFamily>(b, stream); }

void launch_quantize_grouped_ef_guarded(const GroupedEfLaunch& q, hipStream_t stream, int num_cu) { launch_grouped_ef_guarded<EfFamily>(q, stream, num_cu); }

}  // namespace pq
