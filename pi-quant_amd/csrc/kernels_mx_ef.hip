// Instantiation and launch of the MX error-feedback kernels (mx_ef_kernels.hpp): the single call, its batch and the fused reduce (2 float types x
// 2 formats each) and their guarded form -- the twenty-fourth kernel unit.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "mx_ef_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline bool streams(const MxEfLaunch& q) { return aligned16(q.in) && aligned16(q.residual) && aligned16(q.codes) && aligned16(q.scales); }

// f(DT, FMT) as integral constants
template <class F>
void with_mx_ef_pair(int dt, int fmt, F&& f) {
    with_float_type(dt, [&](auto di) { with_mx_format(fmt, [&](auto fi) { f(di, fi); }); });
}

}  // namespace

void launch_reduce_quantize_mx_ef(const MxReduceEfLaunch& r, bool guarded, hipStream_t stream, int num_cu) {
    if (r.numel <= 0) return;
    const MxTerms terms = mx_terms_of(r, "reduce_quantize_mx_ef", 0);
    const int64_t nblocks = (r.numel + kMxBlock - 1) / kMxBlock;
    uint8_t* codes = static_cast<uint8_t*>(r.codes);
    with_mx_ef_pair(r.dt_acc, r.fmt, [&](auto di, auto fi) {
        constexpr int DT = decltype(di)::value, FMT = decltype(fi)::value;
        if (guarded) {
            PQ_LAUNCH((reduce_quantize_mx_ef_guarded_kernel<DT, FMT>), dim3(mx_guarded_blocks(nblocks, num_cu)), dim3(kGroupedBlock), 0, stream, r.acc, r.residual,
                      codes, r.scales, r.numel, nblocks, terms);
        } else {
            constexpr int64_t TE = MxQuantTile<DT, FMT>::TILE_ELEMS;
            const dim3 grid(grouped_blocks((r.numel + TE - 1) / TE, "reduce_quantize_mx_ef"));
            PQ_LAUNCH((reduce_quantize_mx_ef_kernel<DT, FMT>), grid, dim3(kGroupedBlock), 0, stream, r.acc, r.residual, codes, r.scales, r.numel, nblocks, terms);
        }
    });
    PQ_HIP(hipGetLastError());
}

void launch_quantize_mx_ef(const MxEfLaunch& q, hipStream_t stream, int num_cu) {
    if (q.numel <= 0) return;
    if (!streams(q)) {   // the guarded kernel with no terms
        launch_reduce_quantize_mx_ef(MxReduceEfLaunch {q.in, q.residual, q.codes, q.scales, q.numel, q.dt_in, q.fmt, {}, 0}, true, stream, num_cu);
        return;
    }
    const int64_t nblocks = (q.numel + kMxBlock - 1) / kMxBlock;
    with_mx_ef_pair(q.dt_in, q.fmt, [&](auto di, auto fi) {
        constexpr int DT = decltype(di)::value, FMT = decltype(fi)::value;
        constexpr int64_t TE = MxQuantTile<DT, FMT>::TILE_ELEMS;
        const dim3 grid(grouped_blocks((q.numel + TE - 1) / TE, "quantize_mx_ef"));
        PQ_LAUNCH((quantize_mx_ef_kernel<DT, FMT>), grid, dim3(kGroupedBlock), 0, stream, q.in, q.residual, static_cast<uint8_t*>(q.codes), q.scales, q.numel,
                  nblocks);
    });
    PQ_HIP(hipGetLastError());
}

void launch_quantize_mx_ef_batch(const MxEfBatchLaunch& b, hipStream_t stream) {
    static_assert(kMxMaxInputs == kMxBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kMxBatchMax) panic("quantize_mx_ef_batch: %d tensors, at most %d per launch", b.count, kMxBatchMax);
    if (b.count == 1) {   // the single kernel: its arguments arrive as leading scalars
        launch_quantize_mx_ef(b.t[0], stream, 0);
        return;
    }
    with_mx_ef_pair(b.t[0].dt_in, b.t[0].fmt, [&](auto di, auto fi) {
        constexpr int DT = decltype(di)::value, FMT = decltype(fi)::value;
        MxEfBatchArgs a {};
        for (int t = 0; t < b.count; ++t) {
            a.in[t] = b.t[t].in;
            a.residual[t] = b.t[t].residual;
            a.codes[t] = static_cast<uint8_t*>(b.t[t].codes);
            a.scales[t] = b.t[t].scales;
            a.numel[t] = b.t[t].numel;
        }
        a.count = b.count;
        const int64_t chunks = fill_chunk_table(a, MxQuantTile<DT, FMT>::TILE_ELEMS);
        if (chunks == 0) return;
        PQ_LAUNCH((quantize_mx_ef_batch_kernel<DT, FMT>), dim3(grouped_blocks(chunks, "quantize_mx_ef_batch")), dim3(kGroupedBlock), 0, stream, a);
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
