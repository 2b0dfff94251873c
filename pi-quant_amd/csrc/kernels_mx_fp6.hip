// Instantiation and launch of the MXFP6 kernels (mx_fp6_kernels.hpp): the twenty-fifth kernel unit.  The FP6 formats have a format switch of their
// own: with_mx_format (grouped_dispatch.hpp) stays FP4 / FP8, so the batch, reduce and error-feedback kernels are not instantiated for formats they
// are not written for.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "mx_fp6_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <class F>
inline void with_mx_fp6_format(int fmt, F&& f) {
    switch (fmt) {
        case MX_FP6_E2M3: f(std::integral_constant<int, MX_FP6_E2M3> {}); return;
        case MX_FP6_E3M2: f(std::integral_constant<int, MX_FP6_E3M2> {}); return;
        default: panic("invalid MXFP6 format %d", fmt);
    }
}

}  // namespace

void launch_quantize_mx_fp6(const MxQuantLaunch& q, hipStream_t stream, int num_cu) {
    if (q.numel <= 0) return;
    const int64_t nblocks = (q.numel + kMxBlock - 1) / kMxBlock;
    const bool streams = aligned16(q.in) && aligned16(q.codes) && aligned16(q.scales);
    uint8_t* codes = static_cast<uint8_t*>(q.codes);
    with_float_type(q.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_mx_fp6_format(q.fmt, [&](auto fi) {
            constexpr int FMT = decltype(fi)::value;
            if (q.stochastic) {
                if (streams) {
                    const dim3 grid(grouped_blocks((q.numel + kMx6TileElems - 1) / kMx6TileElems, "quantize_mx_sr (FP6)"));
                    PQ_LAUNCH((quantize_mx_fp6_sr_kernel<DT_IN, FMT>), grid, dim3(kGroupedBlock), 0, stream, q.in, codes, q.scales, q.numel, nblocks, q.seed,
                              q.index_base);
                } else {
                    PQ_LAUNCH((quantize_mx_fp6_sr_guarded_kernel<DT_IN, FMT>), dim3(mx_guarded_blocks(nblocks, num_cu)), dim3(kGroupedBlock), 0, stream, q.in,
                              codes, q.scales, q.numel, nblocks, q.seed, q.index_base);
                }
            } else if (streams) {
                const dim3 grid(grouped_blocks((q.numel + kMx6TileElems - 1) / kMx6TileElems, "quantize_mx (FP6)"));
                PQ_LAUNCH((quantize_mx_fp6_kernel<DT_IN, FMT>), grid, dim3(kGroupedBlock), 0, stream, q.in, codes, q.scales, q.numel, nblocks);
            } else {
                PQ_LAUNCH((quantize_mx_fp6_guarded_kernel<DT_IN, FMT>), dim3(mx_guarded_blocks(nblocks, num_cu)), dim3(kGroupedBlock), 0, stream, q.in, codes,
                          q.scales, q.numel, nblocks);
            }
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_dequantize_mx_fp6(const MxDequantLaunch& d, hipStream_t stream, int num_cu) {
    if (d.numel <= 0) return;
    const int64_t nblocks = (d.numel + kMxBlock - 1) / kMxBlock;
    const bool streams = aligned16(d.codes) && aligned16(d.scales) && aligned16(d.out);
    const uint8_t* codes = static_cast<const uint8_t*>(d.codes);
    with_mx_fp6_format(d.fmt, [&](auto fi) {
        constexpr int FMT = decltype(fi)::value;
        with_float_type(d.dt_out, [&](auto di) {
            constexpr int DT_OUT = decltype(di)::value;
            auto with_op = [&](auto oi) {
                constexpr int OP = decltype(oi)::value;
                if (streams) {
                    const dim3 grid(grouped_blocks((d.numel + kMx6TileElems - 1) / kMx6TileElems, "dequantize_mx (FP6)"));
                    PQ_LAUNCH((dequantize_mx_fp6_kernel<FMT, DT_OUT, OP>), grid, dim3(kGroupedBlock), 0, stream, codes, d.scales, d.out, d.numel, nblocks);
                } else {
                    PQ_LAUNCH((dequantize_mx_fp6_guarded_kernel<FMT, DT_OUT, OP>), dim3(mx_guarded_blocks(nblocks, num_cu)), dim3(kGroupedBlock), 0, stream,
                              codes, d.scales, d.out, d.numel, nblocks);
                }
            };
            if (d.op == OP_ADD) with_op(std::integral_constant<int, OP_ADD> {});
            else with_op(std::integral_constant<int, OP_SET> {});
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
