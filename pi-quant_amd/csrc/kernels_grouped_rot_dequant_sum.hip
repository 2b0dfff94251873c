// Instantiation and launch of the rotated grouped dequantize-sum (grouped_rot_kernels.hpp: dequantize_sum_grouped_rotated_kernel): its 96 streaming
// instances (six dtype pairs, eight group sizes, SET and ADD) and 12 guarded ones compile next to the other kernel units, on the same flags.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_rot_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

void launch_dequantize_sum_grouped_rotated(const GroupedDequantSumLaunch& d, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu) {
    static_assert(kGroupedReduceMaxInputs == kGroupedReduceMaxTerms, "host and device term limits");
    const char* name = "dequantize_sum_grouped_rotated";
    if (d.numel <= 0) return;
    if (d.count < 1 || d.count > kGroupedReduceMaxTerms) panic("%s: %d terms, 1 to %d", name, d.count, kGroupedReduceMaxTerms);
    GroupedTerms terms {};
    for (int i = 0; i < d.count; ++i) {
        terms.in[i] = static_cast<const uint8_t*>(d.term[i].in);
        terms.scales[i] = d.term[i].scales;
        terms.zero_points[i] = d.term[i].zero_points;
    }
    terms.count = d.count;
    const int64_t ngroups = (d.numel + d.group_size - 1) / d.group_size;
    const uint32_t lo = static_cast<uint32_t>(rot_seed), hi = static_cast<uint32_t>(rot_seed >> 32);
    with_float_type(d.dt_out, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_quant_bits(d.dt_in, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            if (guarded) {
                if (d.group_size < kGroupedMinG || d.group_size > kGroupedMaxG || (d.group_size & (d.group_size - 1)) != 0)
                    panic("%s: group size %lld", name, static_cast<long long>(d.group_size));
                const int64_t cap = static_cast<int64_t>(64) * (num_cu > 0 ? num_cu : 256);
                const dim3 grid(static_cast<unsigned>(ngroups < cap ? ngroups : cap));   // one wave (one block) per group, grid-stride beyond
                if (d.op == OP_ADD) PQ_LAUNCH((dequantize_sum_grouped_rotated_scalar_kernel<DT, BITS, OP_ADD>), grid, dim3(kGroupedRotGuardedBlock), 0, stream,
                                              d.out, d.numel, d.group_size, ngroups, lo, hi, terms);
                else PQ_LAUNCH((dequantize_sum_grouped_rotated_scalar_kernel<DT, BITS, OP_SET>), grid, dim3(kGroupedRotGuardedBlock), 0, stream, d.out, d.numel,
                               d.group_size, ngroups, lo, hi, terms);
                return;
            }
            with_group_size(d.group_size, name, [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, name));
                if (d.op == OP_ADD) PQ_LAUNCH((dequantize_sum_grouped_rotated_kernel<DT, BITS, OP_ADD, G>), grid, dim3(kGroupedBlock), 0, stream, d.out, d.numel,
                                              ngroups, lo, hi, terms);
                else PQ_LAUNCH((dequantize_sum_grouped_rotated_kernel<DT, BITS, OP_SET, G>), grid, dim3(kGroupedBlock), 0, stream, d.out, d.numel, ngroups, lo,
                               hi, terms);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
