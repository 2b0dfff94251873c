// Instantiation and launch of the batched MX quantize and dequantize (mx_reduce_kernels.hpp: the single kernels' tiles over up to 16 tensors) --
// the twenty-third kernel unit.  A batch of one goes to the single launchers (kernels_mx.hip), whose arguments arrive as leading scalars.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "mx_reduce_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

void launch_quantize_mx_batch(const MxQuantBatchLaunch& b, hipStream_t stream) {
    static_assert(kMxMaxInputs == kMxBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kMxBatchMax) panic("quantize_mx_batch: %d tensors, at most %d per launch", b.count, kMxBatchMax);
    if (b.count == 1) {
        launch_quantize_mx(b.t[0], stream, 0);
        return;
    }
    with_float_type(b.t[0].dt_in, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_mx_format(b.t[0].fmt, [&](auto fi) {
            constexpr int FMT = decltype(fi)::value;
            MxQuantBatchArgs a {};
            for (int t = 0; t < b.count; ++t) {
                a.in[t] = b.t[t].in;
                a.codes[t] = static_cast<uint8_t*>(b.t[t].codes);
                a.scales[t] = b.t[t].scales;
                a.numel[t] = b.t[t].numel;
            }
            a.count = b.count;
            const int64_t chunks = fill_chunk_table(a, MxQuantTile<DT, FMT>::TILE_ELEMS);
            if (chunks == 0) return;
            if (b.t[0].stochastic) {
                MxSrBatchArgs sr {};
                sr.seed = b.t[0].seed;
                for (int t = 0; t < b.count; ++t) sr.index_base[t] = b.t[t].index_base;
                PQ_LAUNCH((quantize_mx_sr_batch_kernel<DT, FMT>), dim3(grouped_blocks(chunks, "quantize_mx_sr_batch")), dim3(kGroupedBlock), 0, stream, a, sr);
                return;
            }
            PQ_LAUNCH((quantize_mx_batch_kernel<DT, FMT>), dim3(grouped_blocks(chunks, "quantize_mx_batch")), dim3(kGroupedBlock), 0, stream, a);
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_dequantize_mx_batch(const MxDequantBatchLaunch& b, hipStream_t stream) {
    if (b.count <= 0) return;
    if (b.count > kMxBatchMax) panic("dequantize_mx_batch: %d tensors, at most %d per launch", b.count, kMxBatchMax);
    if (b.count == 1) {
        launch_dequantize_mx(b.t[0], stream, 0);
        return;
    }
    with_mx_format(b.t[0].fmt, [&](auto fi) {
        constexpr int FMT = decltype(fi)::value;
        with_float_type(b.t[0].dt_out, [&](auto di) {
            constexpr int DT = decltype(di)::value;
            MxDequantBatchArgs a {};
            for (int t = 0; t < b.count; ++t) {
                a.codes[t] = static_cast<const uint8_t*>(b.t[t].codes);
                a.scales[t] = b.t[t].scales;
                a.out[t] = b.t[t].out;
                a.numel[t] = b.t[t].numel;
            }
            a.count = b.count;
            const int64_t chunks = fill_chunk_table(a, MxDequantTile<FMT, DT>::TILE_ELEMS);
            if (chunks == 0) return;
            const dim3 grid(grouped_blocks(chunks, "dequantize_mx_batch"));
            if (b.t[0].op == OP_ADD) PQ_LAUNCH((dequantize_mx_batch_kernel<FMT, DT, OP_ADD>), grid, dim3(kGroupedBlock), 0, stream, a);
            else PQ_LAUNCH((dequantize_mx_batch_kernel<FMT, DT, OP_SET>), grid, dim3(kGroupedBlock), 0, stream, a);
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
