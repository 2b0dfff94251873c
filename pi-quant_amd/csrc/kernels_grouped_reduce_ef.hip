// Instantiation and launch of the fused grouped reduce + quantize with error feedback (grouped_kernels.hpp: reduce_quantize_grouped_ef_kernel).
// A translation unit of its own: its instances compile next to kernels.hip, kernels_grouped.hip and kernels_grouped_ef.hip.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

void launch_reduce_quantize_grouped_ef(const GroupedReduceLaunch& r, hipStream_t stream) {
    static_assert(kGroupedReduceMaxInputs == kGroupedReduceMaxTerms, "host and device term limits");
    if (r.numel <= 0) return;
    if (r.count < 0 || r.count > kGroupedReduceMaxTerms) panic("reduce_quantize_grouped_ef: %d terms, at most %d per launch", r.count, kGroupedReduceMaxTerms);
    const QuantParams p = grouped_call_params(r.rm);
    GroupedTerms terms {};
    for (int i = 0; i < r.count; ++i) {
        terms.in[i] = static_cast<const uint8_t*>(r.term[i].in);
        terms.scales[i] = r.term[i].scales;
        terms.zero_points[i] = r.term[i].zero_points;
    }
    terms.count = r.count;
    const int64_t ngroups = (r.numel + r.group_size - 1) / r.group_size;
    with_float_type(r.dt_in, [&](auto di) {
        constexpr int DT_ACC = decltype(di)::value;
        with_quant_bits(r.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_ACC, BITS>(r.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(r.group_size, "reduce_quantize_grouped_ef", [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_ACC, BITS, G>::NG;
                    const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, "reduce_quantize_grouped_ef"));
                    PQ_LAUNCH((reduce_quantize_grouped_ef_kernel<DT_ACC, BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, r.in, r.residual,
                              static_cast<uint8_t*>(r.out), r.numel, r.scales, r.zero_points, ngroups, p, terms);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
