// Instantiation and launch of the group-wise quantize with a per-group clip search (grouped_clip_kernels.hpp): the streaming kernel, its batch and
// the guarded kernel -- the nineteenth kernel unit, on the same flags (-ffp-contract=off: every step of a candidate's error is rounded on its own).
// The number of candidates is a kernel argument, so the instances are those of quantize_grouped: two tensor types, three widths, three rounding
// modes, eight group sizes.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_clip_kernels.hpp"
#include "grouped_dispatch.hpp"
#include "stop_event.hpp"

namespace pq {

void launch_quantize_grouped_clipped_batch(const GroupedQuantBatchLaunch& b, int steps, hipStream_t stream) {
    const char* name = "quantize_grouped_clipped";
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("%s_batch: %d tensors, at most %d per launch", name, b.count, kGroupedBatchMax);
    if (steps < 1 || steps > kGroupedClipMaxSteps) panic("%s: %d steps, 1 to %d are possible", name, steps, kGroupedClipMaxSteps);
    const QuantParams p = grouped_call_params(b.rm);
    with_float_type(b.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_quant_bits(b.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_IN, BITS>(b.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(b.group_size, name, [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_IN, BITS, G>::NG;
                    GroupedClipBatchArgs a {};
                    for (int t = 0; t < b.count; ++t) {
                        a.in[t] = b.t[t].in;
                        a.out[t] = static_cast<uint8_t*>(b.t[t].out);
                        a.scales[t] = b.t[t].scales;
                        a.zero_points[t] = b.t[t].zero_points;
                        a.choices[t] = b.t[t].choices;
                        a.numel[t] = b.t[t].numel;
                    }
                    a.count = b.count;
                    const int64_t chunks = fill_chunk_table(a, static_cast<int64_t>(G) * NG);
                    if (chunks == 0) return;
                    const dim3 grid(grouped_blocks(chunks, name));
                    if (b.count == 1)   // the single call: its arguments arrive as leading scalars, no table
                        PQ_LAUNCH((quantize_grouped_clipped_kernel<DT_IN, BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, a.in[0], a.out[0], a.numel[0],
                                  a.scales[0], a.zero_points[0], (a.numel[0] + G - 1) / G, a.choices[0], steps, p);
                    else PQ_LAUNCH((quantize_grouped_clipped_batch_kernel<DT_IN, BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, a, steps, p);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_quantize_grouped_clipped_guarded(const GroupedQuantLaunch& q, int steps, hipStream_t stream, int num_cu) {
    const char* name = "quantize_grouped_clipped";
    if (q.numel <= 0) return;
    if (steps < 1 || steps > kGroupedClipMaxSteps) panic("%s: %d steps, 1 to %d are possible", name, steps, kGroupedClipMaxSteps);
    if (q.group_size < kGroupedMinG || q.group_size > kGroupedMaxG || (q.group_size & (q.group_size - 1)) != 0)
        panic("%s: group size %lld (a power of two in [%d, %d] is needed)", name, static_cast<long long>(q.group_size), kGroupedMinG, kGroupedMaxG);
    const QuantParams p = grouped_call_params(q.rm);
    const int64_t ngroups = (q.numel + q.group_size - 1) / q.group_size;
    const dim3 grid(grouped_guarded_blocks(ngroups, num_cu));
    with_float_type(q.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_quant_bits(q.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_IN, BITS>(q.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                PQ_LAUNCH((quantize_grouped_clipped_scalar_kernel<DT_IN, BITS, MODE>), grid, dim3(kGroupedBlock), 0, stream, q.in, static_cast<uint8_t*>(q.out),
                          q.numel, q.group_size, q.scales, q.zero_points, ngroups, q.choices, steps, p);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
