// Instantiation and launch of the fused grouped reduce + quantize with error feedback of a bfloat16 accumulator with a float32 residual
// (grouped_kernels.hpp: reduce_quantize_grouped_ef_f32r_kernel).  A translation unit of its own, the sixth: its 72 instances compile next to the
// other kernel units.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

void launch_reduce_quantize_grouped_ef_f32r(const GroupedReduceLaunch& r, hipStream_t stream) {
    static_assert(kGroupedReduceMaxInputs == kGroupedReduceMaxTerms, "host and device term limits");
    const char* name = "reduce_quantize_grouped_ef_mixed";
    if (r.numel <= 0) return;
    if (r.dt_in != DT_BF16) panic("%s: a float32 residual goes with a bfloat16 accumulator (type %d)", name, r.dt_in);
    if (r.count < 0 || r.count > kGroupedReduceMaxTerms) panic("%s: %d terms, at most %d per launch", name, r.count, kGroupedReduceMaxTerms);
    const QuantParams p = grouped_call_params(r.rm);
    GroupedTerms terms {};
    for (int i = 0; i < r.count; ++i) {
        terms.in[i] = static_cast<const uint8_t*>(r.term[i].in);
        terms.scales[i] = r.term[i].scales;
        terms.zero_points[i] = r.term[i].zero_points;
    }
    terms.count = r.count;
    const int64_t ngroups = (r.numel + r.group_size - 1) / r.group_size;
    // the pipeline behind the widening load is the float32 one: bit widths, rounding modes and group sizes dispatch as for a float32 tensor
    with_quant_bits(r.dt_out, [&](auto bi) {
        constexpr int BITS = decltype(bi)::value;
        with_round_mode<DT_F32, BITS>(r.rm.round_mode, [&](auto mi) {
            constexpr int MODE = decltype(mi)::value;
            with_group_size(r.group_size, name, [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, name));
                PQ_LAUNCH((reduce_quantize_grouped_ef_f32r_kernel<BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, r.in, r.residual,
                          static_cast<uint8_t*>(r.out), r.numel, r.scales, r.zero_points, ngroups, p, terms);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
