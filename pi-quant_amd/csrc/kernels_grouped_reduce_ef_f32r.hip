// Instantiation and launch of the fused grouped reduce + quantize with error feedback of a bfloat16 accumulator with a float32 residual
// (grouped_kernels.hpp: reduce_quantize_grouped_ef_f32r_kernel).  A translation unit of its own, the sixth: its 72 instances compile next to the
// other kernel units.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

// the pipeline behind the widening load is the float32 one: bit widths, rounding modes and group sizes dispatch as for a float32 tensor
struct ReduceEfF32rFamily {
    static constexpr const char* name = "reduce_quantize_grouped_ef_mixed";
    static constexpr bool residual = true;
    template <class F>
    static void with_pipeline_type(int, F&& f) {
        f(std::integral_constant<int, DT_F32> {});
    }
    template <int DT, int BITS, int MODE, int G>
    static auto kernel() {
        return &reduce_quantize_grouped_ef_f32r_kernel<BITS, MODE, G>;
    }
};

}  // namespace

void launch_reduce_quantize_grouped_ef_f32r(const GroupedReduceLaunch& r, hipStream_t stream) {
    // the type check stays in front of the shared body's term-count check, where it was
    if (r.numel > 0 && r.dt_in != DT_BF16)
        panic("%s: a float32 residual goes with a bfloat16 accumulator (type %d)", ReduceEfF32rFamily::name, r.dt_in);
    launch_grouped_reduce<ReduceEfF32rFamily>(r, stream);
}

}  // namespace pq
