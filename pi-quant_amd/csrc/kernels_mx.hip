// Instantiation and launch of the MX block-format kernels (mx_kernels.hpp): the twenty-first kernel unit.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "mx_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void launch_quantize_mx(const MxQuantLaunch& q, hipStream_t stream, int num_cu) {
    if (q.numel <= 0) return;
    const int64_t nblocks = (q.numel + kMxBlock - 1) / kMxBlock;
    const bool streams = aligned16(q.in) && aligned16(q.codes) && aligned16(q.scales);
    uint8_t* codes = static_cast<uint8_t*>(q.codes);
    with_float_type(q.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_mx_format(q.fmt, [&](auto fi) {
            constexpr int FMT = decltype(fi)::value;
            constexpr int64_t TE = MxQuantTile<DT_IN, FMT>::TILE_ELEMS;
            if (q.stochastic) {
                if (streams) {
                    const dim3 grid(grouped_blocks((q.numel + TE - 1) / TE, "quantize_mx_sr"));
                    PQ_LAUNCH((quantize_mx_sr_kernel<DT_IN, FMT>), grid, dim3(kGroupedBlock), 0, stream, q.in, codes, q.scales, q.numel, nblocks, q.seed,
                              q.index_base);
                } else {
                    PQ_LAUNCH((quantize_mx_sr_guarded_kernel<DT_IN, FMT>), dim3(mx_guarded_blocks(nblocks, num_cu)), dim3(kGroupedBlock), 0, stream, q.in, codes,
                              q.scales, q.numel, nblocks, q.seed, q.index_base);
                }
            } else if (streams) {
                const dim3 grid(grouped_blocks((q.numel + TE - 1) / TE, "quantize_mx"));
                PQ_LAUNCH((quantize_mx_kernel<DT_IN, FMT>), grid, dim3(kGroupedBlock), 0, stream, q.in, codes, q.scales, q.numel, nblocks);
            } else {
                PQ_LAUNCH((quantize_mx_guarded_kernel<DT_IN, FMT>), dim3(mx_guarded_blocks(nblocks, num_cu)), dim3(kGroupedBlock), 0, stream, q.in, codes,
                          q.scales, q.numel, nblocks);
            }
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_dequantize_mx(const MxDequantLaunch& d, hipStream_t stream, int num_cu) {
    if (d.numel <= 0) return;
    const int64_t nblocks = (d.numel + kMxBlock - 1) / kMxBlock;
    const bool streams = aligned16(d.codes) && aligned16(d.scales) && aligned16(d.out);
    const uint8_t* codes = static_cast<const uint8_t*>(d.codes);
    with_mx_format(d.fmt, [&](auto fi) {
        constexpr int FMT = decltype(fi)::value;
        with_float_type(d.dt_out, [&](auto di) {
            constexpr int DT_OUT = decltype(di)::value;
            auto with_op = [&](auto oi) {
                constexpr int OP = decltype(oi)::value;
                if (streams) {
                    constexpr int64_t TE = MxDequantTile<FMT, DT_OUT>::TILE_ELEMS;
                    const dim3 grid(grouped_blocks((d.numel + TE - 1) / TE, "dequantize_mx"));
                    PQ_LAUNCH((dequantize_mx_kernel<FMT, DT_OUT, OP>), grid, dim3(kGroupedBlock), 0, stream, codes, d.scales, d.out, d.numel, nblocks);
                } else {
                    PQ_LAUNCH((dequantize_mx_guarded_kernel<FMT, DT_OUT, OP>), dim3(mx_guarded_blocks(d.numel, num_cu)), dim3(kGroupedBlock), 0, stream, codes,
                              d.scales, d.out, d.numel);
                }
            };
            if (d.op == OP_ADD) with_op(std::integral_constant<int, OP_ADD> {});
            else with_op(std::integral_constant<int, OP_SET> {});
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
