// Instantiation and launch of the batched rotated grouped dequantize (grouped_rot_kernels.hpp: dequantize_grouped_rotated_batch_kernel): its 96
// instances (two output types, three widths, SET and ADD, eight group sizes) compile next to the other kernel units, on the same flags.  A batch of
// one goes to launch_dequantize_grouped_rotated (kernels_grouped_rot.hip), so the single-tensor kernels are instantiated there only.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_rot_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

// The chunk table's unit is the chunk of the float32 QUANTIZE tile (G * NG elements), the tile the rotated dequantize sits on -- not
// GroupedDequantTile's CHUNK_ELEMS, which launch_dequantize_grouped_batch hands to fill_chunk_table.
void launch_dequantize_grouped_rotated_batch(const GroupedDequantBatchLaunch& b, uint64_t rot_seed, hipStream_t stream) {
    const char* name = "dequantize_grouped_rotated";
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("%s_batch: %d tensors, at most %d per launch", name, b.count, kGroupedBatchMax);
    if (b.count == 1) {   // the single call: its arguments arrive as leading scalars, no table
        launch_dequantize_grouped_rotated(GroupedDequantLaunch {b.t[0], b}, rot_seed, false, stream, 0);
        return;
    }
    const uint32_t lo = static_cast<uint32_t>(rot_seed), hi = static_cast<uint32_t>(rot_seed >> 32);
    with_float_type(b.dt_out, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_quant_bits(b.dt_in, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_group_size(b.group_size, name, [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                GroupedDequantBatchArgs a {};
                for (int t = 0; t < b.count; ++t) {
                    a.in[t] = static_cast<const uint8_t*>(b.t[t].in);
                    a.out[t] = b.t[t].out;
                    a.scales[t] = b.t[t].scales;
                    a.zero_points[t] = b.t[t].zero_points;
                    a.numel[t] = b.t[t].numel;
                }
                a.count = b.count;
                const int64_t chunks = fill_chunk_table(a, static_cast<int64_t>(G) * NG);
                if (chunks == 0) return;
                const dim3 grid(grouped_blocks(chunks, name));
                if (b.op == OP_ADD) PQ_LAUNCH((dequantize_grouped_rotated_batch_kernel<DT, BITS, OP_ADD, G>), grid, dim3(kGroupedBlock), 0, stream, a, lo, hi);
                else PQ_LAUNCH((dequantize_grouped_rotated_batch_kernel<DT, BITS, OP_SET, G>), grid, dim3(kGroupedBlock), 0, stream, a, lo, hi);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
