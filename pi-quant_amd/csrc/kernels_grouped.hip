// Instantiation and launch of the batched group-wise kernels and the fused grouped reduce + quantize (grouped_kernels.hpp).  A translation
// unit of its own: the ~500 instances compile next to kernels.hip instead of behind it.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

void launch_quantize_grouped_batch(const GroupedQuantBatchLaunch& b, hipStream_t stream) {
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("quantize_grouped_batch: %d tensors, at most %d per launch", b.count, kGroupedBatchMax);
    const QuantParams p = grouped_call_params(b.rm);
    with_float_type(b.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_quant_bits(b.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_IN, BITS>(b.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(b.group_size, "quantize_grouped_batch", [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_IN, BITS, G>::NG;
                    GroupedQuantBatchArgs a {};
                    for (int t = 0; t < b.count; ++t) {
                        a.in[t] = b.t[t].in;
                        a.out[t] = static_cast<uint8_t*>(b.t[t].out);
                        a.scales[t] = b.t[t].scales;
                        a.zero_points[t] = b.t[t].zero_points;
                        a.numel[t] = b.t[t].numel;
                    }
                    a.count = b.count;
                    const int64_t chunks = fill_chunk_table(a, static_cast<int64_t>(G) * NG);
                    if (chunks == 0) return;
                    const dim3 grid(grouped_blocks(chunks, "quantize_grouped_batch"));
                    if (b.params_given) PQ_LAUNCH((quantize_grouped_batch_kernel<DT_IN, BITS, MODE, G, true>), grid, dim3(kGroupedBlock), 0, stream, a, p);
                    else PQ_LAUNCH((quantize_grouped_batch_kernel<DT_IN, BITS, MODE, G, false>), grid, dim3(kGroupedBlock), 0, stream, a, p);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_dequantize_grouped_batch(const GroupedDequantBatchLaunch& b, hipStream_t stream) {
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("dequantize_grouped_batch: %d tensors, at most %d per launch", b.count, kGroupedBatchMax);
    with_quant_bits(b.dt_in, [&](auto bi) {
        constexpr int BITS = decltype(bi)::value;
        with_float_type(b.dt_out, [&](auto di) {
            constexpr int DT_OUT = decltype(di)::value;
            with_group_size(b.group_size, "dequantize_grouped_batch", [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int64_t CE = GroupedDequantTile<BITS, DT_OUT>::CHUNK_ELEMS;
                GroupedDequantBatchArgs a {};
                for (int t = 0; t < b.count; ++t) {
                    a.in[t] = static_cast<const uint8_t*>(b.t[t].in);
                    a.out[t] = b.t[t].out;
                    a.scales[t] = b.t[t].scales;
                    a.zero_points[t] = b.t[t].zero_points;
                    a.numel[t] = b.t[t].numel;
                }
                a.count = b.count;
                const int64_t chunks = fill_chunk_table(a, CE);
                if (chunks == 0) return;
                const dim3 grid(grouped_blocks(chunks, "dequantize_grouped_batch"));
                if (b.op == OP_ADD) PQ_LAUNCH((dequantize_grouped_batch_kernel<BITS, DT_OUT, OP_ADD, G>), grid, dim3(kGroupedBlock), 0, stream, a);
                else PQ_LAUNCH((dequantize_grouped_batch_kernel<BITS, DT_OUT, OP_SET, G>), grid, dim3(kGroupedBlock), 0, stream, a);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

namespace {

struct ReduceFamily {
    static constexpr const char* name = "reduce_quantize_grouped";
    static constexpr bool residual = false;
    template <class F>
    static void with_pipeline_type(int dt_in, F&& f) {
        with_float_type(dt_in, f);
    }
    template <int DT_ACC, int BITS, int MODE, int G>
    static auto kernel() {
        return &reduce_quantize_grouped_kernel<DT_ACC, BITS, MODE, G>;
    }
};

}  // namespace

void launch_reduce_quantize_grouped(const GroupedReduceLaunch& r, hipStream_t stream) { launch_grouped_reduce<ReduceFamily>(r, stream); }

}  // namespace pq
