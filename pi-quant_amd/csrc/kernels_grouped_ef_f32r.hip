// Instantiation and launch of the error-feedback group-wise quantize of a bfloat16 tensor with a float32 residual (grouped_kernels.hpp:
// quantize_grouped_ef_f32r_kernel, its batch and its guarded form).  A translation unit of its own: its instances compile next to the other
// kernel units.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

// the pipeline behind the widening load is the float32 one: bit widths, rounding modes and group sizes dispatch as for a float32 tensor
struct EfF32rFamily {
    static constexpr const char* name = "quantize_grouped_ef_mixed";
    template <class F>
    static void with_pipeline_type(int dt_in, F&& f) {
        if (dt_in != DT_BF16) panic("%s: a float32 residual goes with a bfloat16 tensor (type %d)", name, dt_in);
        f(std::integral_constant<int, DT_F32> {});
    }
    template <int DT, int BITS, int MODE, int G>
    static auto single() {
        return &quantize_grouped_ef_f32r_kernel<BITS, MODE, G>;
    }
    template <int DT, int BITS, int MODE, int G>
    static auto batch() {
        return &quantize_grouped_ef_f32r_batch_kernel<BITS, MODE, G>;
    }
    template <int DT, int BITS, int MODE>
    static auto guarded() {
        return &quantize_grouped_ef_f32r_scalar_kernel<BITS, MODE>;
    }
};

}  // namespace

void launch_quantize_grouped_ef_f32r_batch(const GroupedEfBatchLaunch& b, hipStream_t stream) { launch_grouped_ef_batch<EfF32rFamily>(b, stream); }

void launch_quantize_grouped_ef_f32r_guarded(const GroupedEfLaunch& q, hipStream_t stream, int num_cu) {
    launch_grouped_ef_guarded<EfF32rFamily>(q, stream, num_cu);
}

}  // namespace pq
