// Instantiation and launch of the batched rotated grouped quantize with error feedback (grouped_rot_ef_kernels.hpp:
// quantize_grouped_rotated_ef_batch_kernel): its 144 instances (two tensor types, three widths, three rounding modes, eight group sizes) compile
// next to the other kernel units, on the same flags.  A batch of one goes to launch_quantize_grouped_rotated_ef (kernels_grouped_rot_ef_quant.hip),
// so the single-tensor kernels are instantiated there only.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_rot_ef_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

// The pipeline is the float32 one whatever the tensors' type, and every residual is float32; the chunk table's unit is the float32 tile's chunk.
void launch_quantize_grouped_rotated_ef_batch(const GroupedEfBatchLaunch& b, uint64_t rot_seed, hipStream_t stream) {
    const char* name = "quantize_grouped_rotated_ef";
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("%s_batch: %d tensors, at most %d per launch", name, b.count, kGroupedBatchMax);
    if (b.count == 1) {   // the single call: its arguments arrive as leading scalars, no table
        launch_quantize_grouped_rotated_ef(GroupedEfLaunch {b.t[0], b}, rot_seed, false, stream, 0);
        return;
    }
    const QuantParams p = grouped_call_params(b.rm);
    const uint32_t lo = static_cast<uint32_t>(rot_seed), hi = static_cast<uint32_t>(rot_seed >> 32);
    with_float_type(b.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_quant_bits(b.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_F32, BITS>(b.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(b.group_size, name, [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                    GroupedEfBatchArgs a {};
                    for (int t = 0; t < b.count; ++t) {
                        a.in[t] = b.t[t].in;
                        a.residual[t] = b.t[t].residual;
                        a.out[t] = static_cast<uint8_t*>(b.t[t].out);
                        a.scales[t] = b.t[t].scales;
                        a.zero_points[t] = b.t[t].zero_points;
                        a.numel[t] = b.t[t].numel;
                    }
                    a.count = b.count;
                    const int64_t chunks = fill_chunk_table(a, static_cast<int64_t>(G) * NG);
                    if (chunks == 0) return;
                    const dim3 grid(grouped_blocks(chunks, name));
                    PQ_LAUNCH((quantize_grouped_rotated_ef_batch_kernel<DT_IN, BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, a, lo, hi, p);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
