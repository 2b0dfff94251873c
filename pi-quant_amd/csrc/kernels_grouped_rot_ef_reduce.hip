// Instantiation and launch of the rotated grouped reduce + quantize with error feedback (grouped_rot_ef_kernels.hpp:
// reduce_quantize_grouped_rotated_ef_kernel): its 144 streaming instances (two accumulator types, three widths, three rounding modes, eight group
// sizes) and the 18 guarded ones, which also serve the call without terms, compile next to the other kernel units, on the same flags.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_rot_ef_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

// The pipeline is the float32 one whatever the accumulator's type, and the residual is float32.
void launch_reduce_quantize_grouped_rotated_ef(const GroupedReduceLaunch& r, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu) {
    static_assert(kGroupedReduceMaxInputs == kGroupedReduceMaxTerms, "host and device term limits");
    const char* name = "reduce_quantize_grouped_rotated_ef";
    if (r.numel <= 0) return;
    if (r.count < 0 || r.count > kGroupedReduceMaxTerms) panic("%s: %d terms, at most %d", name, r.count, kGroupedReduceMaxTerms);
    const QuantParams p = grouped_call_params(r.rm);
    GroupedTerms terms {};
    for (int i = 0; i < r.count; ++i) {
        terms.in[i] = static_cast<const uint8_t*>(r.term[i].in);
        terms.scales[i] = r.term[i].scales;
        terms.zero_points[i] = r.term[i].zero_points;
    }
    terms.count = r.count;
    const int64_t ngroups = (r.numel + r.group_size - 1) / r.group_size;
    const uint32_t lo = static_cast<uint32_t>(rot_seed), hi = static_cast<uint32_t>(rot_seed >> 32);
    uint8_t* out = static_cast<uint8_t*>(r.out);
    float* residual = static_cast<float*>(r.residual);
    with_float_type(r.dt_in, [&](auto di) {
        constexpr int DT_ACC = decltype(di)::value;
        with_quant_bits(r.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_F32, BITS>(r.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                if (guarded) {
                    if (r.group_size < kGroupedMinG || r.group_size > kGroupedMaxG || (r.group_size & (r.group_size - 1)) != 0)
                        panic("%s: group size %lld", name, static_cast<long long>(r.group_size));
                    const int64_t cap = static_cast<int64_t>(64) * (num_cu > 0 ? num_cu : 256);
                    const dim3 grid(static_cast<unsigned>(ngroups < cap ? ngroups : cap));   // one wave (one block) per group, grid-stride beyond
                    PQ_LAUNCH((reduce_quantize_grouped_rotated_ef_scalar_kernel<DT_ACC, BITS, MODE>), grid, dim3(kGroupedRotGuardedBlock), 0, stream, r.in,
                              residual, out, r.numel, r.group_size, r.scales, r.zero_points, ngroups, lo, hi, p.threshold, p.seed_lo, p.seed_hi, p.index_base,
                              terms);
                    return;
                }
                with_group_size(r.group_size, name, [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                    const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, name));
                    PQ_LAUNCH((reduce_quantize_grouped_rotated_ef_kernel<DT_ACC, BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, r.in, residual, out,
                              r.numel, r.scales, r.zero_points, ngroups, lo, hi, p, terms);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
