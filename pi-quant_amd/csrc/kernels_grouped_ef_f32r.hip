// Instantiation and launch of the error-feedback group-wise quantize of a bfloat16 tensor with a float32 residual (grouped_kernels.hpp:
// quantize_grouped_ef_f32r_kernel, its batch and its guarded form).  A translation unit of its own: its instances compile next to the other
// kernel units.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

// the pipeline behind the widening load is the float32 one: bit widths, rounding modes and group sizes dispatch as for a float32 tensor
void launch_quantize_grouped_ef_f32r_batch(const GroupedEfBatchLaunch& b, hipStream_t stream) {
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("quantize_grouped_ef_mixed_batch: %d tensors, at most %d per launch", b.count, kGroupedBatchMax);
    if (b.dt_in != DT_BF16) panic("quantize_grouped_ef_mixed_batch: a float32 residual goes with a bfloat16 tensor (type %d)", b.dt_in);
    const QuantParams p = grouped_call_params(b.threshold, b.seed, b.index_base);
    with_quant_bits(b.dt_out, [&](auto bi) {
        constexpr int BITS = decltype(bi)::value;
        with_round_mode<DT_F32, BITS>(b.round_mode, [&](auto mi) {
            constexpr int MODE = decltype(mi)::value;
            with_group_size(b.group_size, "quantize_grouped_ef_mixed_batch", [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                GroupedEfBatchArgs a {};
                int64_t chunks = 0;
                for (int t = 0; t < b.count; ++t) {
                    a.in[t] = b.in[t];
                    a.residual[t] = b.residual[t];
                    a.out[t] = static_cast<uint8_t*>(b.out[t]);
                    a.scales[t] = b.scales[t];
                    a.zero_points[t] = b.zero_points[t];
                    a.numel[t] = b.numel[t];
                    a.chunk_begin[t] = chunks;
                    chunks += ((b.numel[t] + G - 1) / G + NG - 1) / NG;
                }
                a.chunk_begin[b.count] = chunks;
                a.count = b.count;
                if (chunks == 0) return;
                const dim3 grid(grouped_blocks(chunks, "quantize_grouped_ef_mixed_batch"));
                if (b.count == 1)   // the single call: its arguments arrive as leading scalars, no table
                    PQ_LAUNCH((quantize_grouped_ef_f32r_kernel<BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, a.in[0], a.residual[0], a.out[0], a.numel[0],
                              a.scales[0], a.zero_points[0], (a.numel[0] + G - 1) / G, p);
                else PQ_LAUNCH((quantize_grouped_ef_f32r_batch_kernel<BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, a, p);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_quantize_grouped_ef_f32r_guarded(const GroupedEfBatchLaunch& b, int t, hipStream_t stream, int num_cu) {
    const int64_t numel = b.numel[t];
    if (numel <= 0) return;
    if (b.dt_in != DT_BF16) panic("quantize_grouped_ef_mixed: a float32 residual goes with a bfloat16 tensor (type %d)", b.dt_in);
    const QuantParams p = grouped_call_params(b.threshold, b.seed, b.index_base);
    const int64_t ngroups = (numel + b.group_size - 1) / b.group_size;
    const int64_t want = (ngroups + kGroupedBlock / 64 - 1) / (kGroupedBlock / 64), cap = static_cast<int64_t>(16) * (num_cu > 0 ? num_cu : 256);
    const dim3 grid(static_cast<unsigned>(want < cap ? want : cap));   // one wave per group, grid-stride beyond 16 blocks per CU
    with_quant_bits(b.dt_out, [&](auto bi) {
        constexpr int BITS = decltype(bi)::value;
        with_round_mode<DT_F32, BITS>(b.round_mode, [&](auto mi) {
            constexpr int MODE = decltype(mi)::value;
            PQ_LAUNCH((quantize_grouped_ef_f32r_scalar_kernel<BITS, MODE>), grid, dim3(kGroupedBlock), 0, stream, b.in[t], b.residual[t],
                      static_cast<uint8_t*>(b.out[t]), numel, b.group_size, b.scales[t], b.zero_points[t], ngroups, p.threshold, p.seed_lo, p.seed_hi, p.index_base);
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
