// Instantiation and launch of the fused grouped reduce + quantize with error feedback (grouped_kernels.hpp: reduce_quantize_grouped_ef_kernel).
// A translation unit of its own: its instances compile next to kernels.hip, kernels_grouped.hip and kernels_grouped_ef.hip.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

struct ReduceEfFamily {
    static constexpr const char* name = "reduce_quantize_grouped_ef";
    static constexpr bool residual = true;
    template <class F>
    static void with_pipeline_type(int dt_in, F&& f) {
        with_float_type(dt_in, f);
    }
    template <int DT_ACC, int BITS, int MODE, int G>
    static auto kernel() {
        return &reduce_quantize_grouped_ef_kernel<DT_ACC, BITS, MODE, G>;
    }
};

}  // namespace

void launch_reduce_quantize_grouped_ef(const GroupedReduceLaunch& r, hipStream_t stream) { launch_grouped_reduce<ReduceEfFamily>(r, stream); }

}  // namespace pq
