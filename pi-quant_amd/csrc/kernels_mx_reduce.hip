// Instantiation and launch of the MX wire's fused kernels (mx_reduce_kernels.hpp): reduce + quantize (2 accumulator types x 2 formats, streaming
// and guarded) and dequantize-sum (2 formats x 2 output types x SET / ADD) -- the twenty-second kernel unit.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "mx_reduce_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

void launch_reduce_quantize_mx(const MxReduceLaunch& r, bool guarded, hipStream_t stream, int num_cu) {
    if (r.numel <= 0) return;
    const MxTerms terms = mx_terms_of(r, "reduce_quantize_mx", 0);
    const int64_t nblocks = (r.numel + kMxBlock - 1) / kMxBlock;
    uint8_t* codes = static_cast<uint8_t*>(r.codes);
    with_float_type(r.dt_acc, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_mx_format(r.fmt, [&](auto fi) {
            constexpr int FMT = decltype(fi)::value;
            if (guarded) {
                PQ_LAUNCH((reduce_quantize_mx_guarded_kernel<DT, FMT>), dim3(mx_guarded_blocks(nblocks, num_cu)), dim3(kGroupedBlock), 0, stream, r.acc, codes,
                          r.scales, r.numel, nblocks, terms);
            } else {
                constexpr int64_t TE = MxQuantTile<DT, FMT>::TILE_ELEMS;
                const dim3 grid(grouped_blocks((r.numel + TE - 1) / TE, "reduce_quantize_mx"));
                PQ_LAUNCH((reduce_quantize_mx_kernel<DT, FMT>), grid, dim3(kGroupedBlock), 0, stream, r.acc, codes, r.scales, r.numel, nblocks, terms);
            }
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_dequantize_sum_mx(const MxDequantSumLaunch& d, hipStream_t stream) {
    if (d.numel <= 0) return;
    const MxTerms terms = mx_terms_of(d, "dequantize_sum_mx", 1);
    const int64_t nblocks = (d.numel + kMxBlock - 1) / kMxBlock;
    with_mx_format(d.fmt, [&](auto fi) {
        constexpr int FMT = decltype(fi)::value;
        with_float_type(d.dt_out, [&](auto di) {
            constexpr int DT = decltype(di)::value;
            constexpr int64_t TE = MxDequantTile<FMT, DT>::TILE_ELEMS;
            const dim3 grid(grouped_blocks((d.numel + TE - 1) / TE, "dequantize_sum_mx"));
            if (d.op == OP_ADD) PQ_LAUNCH((dequantize_sum_mx_kernel<FMT, DT, OP_ADD>), grid, dim3(kGroupedBlock), 0, stream, d.out, d.numel, nblocks, terms);
            else PQ_LAUNCH((dequantize_sum_mx_kernel<FMT, DT, OP_SET>), grid, dim3(kGroupedBlock), 0, stream, d.out, d.numel, nblocks, terms);
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
