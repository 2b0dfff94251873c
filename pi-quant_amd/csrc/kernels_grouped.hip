// Instantiation and launch of the batched group-wise kernels and the fused grouped reduce + quantize (grouped_kernels.hpp).  A translation
// unit of its own: the ~500 instances compile next to kernels.hip instead of behind it.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_kernels.hpp"
#include "stop_event.hpp"

#include <type_traits>

namespace pq {

namespace {

// compile-time dispatch of the grouped batch / reduce launches: f(std::integral_constant<int, value>) for the runtime value
template <class F>
void with_group_size(int64_t group_size, const char* what, F&& f) {
    switch (group_size) {
        case 32: f(std::integral_constant<int, 32> {}); return;
        case 64: f(std::integral_constant<int, 64> {}); return;
        case 128: f(std::integral_constant<int, 128> {}); return;
        case 256: f(std::integral_constant<int, 256> {}); return;
        case 512: f(std::integral_constant<int, 512> {}); return;
        case 1024: f(std::integral_constant<int, 1024> {}); return;
        case 2048: f(std::integral_constant<int, 2048> {}); return;
        case 4096: f(std::integral_constant<int, 4096> {}); return;
        default: panic("%s: group size %lld (a power of two in [%d, %d] is needed)", what, static_cast<long long>(group_size), kGroupedMinG, kGroupedMaxG);
    }
}

template <class F>
void with_float_type(int dt, F&& f) {
    switch (dt) {
        case DT_F32: f(std::integral_constant<int, DT_F32> {}); return;
        case DT_BF16: f(std::integral_constant<int, DT_BF16> {}); return;
        default: panic("invalid float type %d", dt);
    }
}

template <class F>
void with_quant_bits(int dt, F&& f) {
    switch (dt) {
        case DT_UINT8: f(std::integral_constant<int, 8> {}); return;
        case DT_UINT4: f(std::integral_constant<int, 4> {}); return;
        case DT_UINT2: f(std::integral_constant<int, 2> {}); return;
        default: panic("invalid quantized type %d", dt);
    }
}

// the rounding modes of quantize_grouped_mode: the nearest step of quantize_uniform for the pair
template <int DT_IN, int BITS, class F>
void with_round_mode(int round_mode, F&& f) {
    switch (round_mode) {
        case RM_NEAREST_FAST:
        case RM_NEAREST_I64:
            if constexpr (DT_IN == DT_F32 && BITS == 2) f(std::integral_constant<int, RM_NEAREST_I64> {});
            else f(std::integral_constant<int, RM_NEAREST_FAST> {});
            return;
        case RM_STOCH_CALL: f(std::integral_constant<int, RM_STOCH_CALL> {}); return;
        case RM_STOCH_ELEM: f(std::integral_constant<int, RM_STOCH_ELEM> {}); return;
        default: panic("invalid rounding mode %d", round_mode);
    }
}

QuantParams grouped_call_params(float threshold, uint64_t seed, uint64_t index_base) {
    QuantParams p {};
    p.threshold = threshold;
    p.seed_lo = static_cast<uint32_t>(seed);
    p.seed_hi = static_cast<uint32_t>(seed >> 32);
    p.index_base = index_base;
    return p;
}

unsigned grouped_blocks(int64_t chunks, const char* what) {
    const int64_t blocks = (chunks + kGroupedBlock / 64 - 1) / (kGroupedBlock / 64);
    if (blocks > 0x7fffffff) panic("%s: %lld blocks in one launch", what, static_cast<long long>(blocks));
    return static_cast<unsigned>(blocks);
}

}  // namespace

void launch_quantize_grouped_batch(const GroupedQuantBatchLaunch& b, hipStream_t stream) {
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("quantize_grouped_batch: %d tensors, at most %d per launch", b.count, kGroupedBatchMax);
    const QuantParams p = grouped_call_params(b.threshold, b.seed, b.index_base);
    with_float_type(b.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_quant_bits(b.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_IN, BITS>(b.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(b.group_size, "quantize_grouped_batch", [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_IN, BITS, G>::NG;
                    GroupedQuantBatchArgs a {};
                    int64_t chunks = 0;
                    for (int t = 0; t < b.count; ++t) {
                        a.in[t] = b.in[t];
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
                int64_t chunks = 0;
                for (int t = 0; t < b.count; ++t) {
                    a.in[t] = static_cast<const uint8_t*>(b.in[t]);
                    a.out[t] = b.out[t];
                    a.scales[t] = b.scales[t];
                    a.zero_points[t] = b.zero_points[t];
                    a.numel[t] = b.numel[t];
                    a.chunk_begin[t] = chunks;
                    chunks += (b.numel[t] + CE - 1) / CE;
                }
                a.chunk_begin[b.count] = chunks;
                a.count = b.count;
                if (chunks == 0) return;
                const dim3 grid(grouped_blocks(chunks, "dequantize_grouped_batch"));
                if (b.op == OP_ADD) PQ_LAUNCH((dequantize_grouped_batch_kernel<BITS, DT_OUT, OP_ADD, G>), grid, dim3(kGroupedBlock), 0, stream, a);
                else PQ_LAUNCH((dequantize_grouped_batch_kernel<BITS, DT_OUT, OP_SET, G>), grid, dim3(kGroupedBlock), 0, stream, a);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_reduce_quantize_grouped(const GroupedReduceLaunch& r, hipStream_t stream) {
    static_assert(kGroupedReduceMaxInputs == kGroupedReduceMaxTerms, "host and device term limits");
    if (r.numel <= 0) return;
    if (r.count < 0 || r.count > kGroupedReduceMaxTerms) panic("reduce_quantize_grouped: %d terms, at most %d per launch", r.count, kGroupedReduceMaxTerms);
    const QuantParams p = grouped_call_params(r.threshold, r.seed, r.index_base);
    GroupedTerms terms {};
    for (int i = 0; i < r.count; ++i) {
        terms.in[i] = static_cast<const uint8_t*>(r.in[i]);
        terms.scales[i] = r.in_scales[i];
        terms.zero_points[i] = r.in_zero_points[i];
    }
    terms.count = r.count;
    const int64_t ngroups = (r.numel + r.group_size - 1) / r.group_size;
    with_float_type(r.dt_acc, [&](auto di) {
        constexpr int DT_ACC = decltype(di)::value;
        with_quant_bits(r.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_ACC, BITS>(r.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(r.group_size, "reduce_quantize_grouped", [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_ACC, BITS, G>::NG;
                    const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, "reduce_quantize_grouped"));
                    PQ_LAUNCH((reduce_quantize_grouped_kernel<DT_ACC, BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, r.acc, static_cast<uint8_t*>(r.out),
                              r.numel, r.scales, r.zero_points, ngroups, p, terms);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
