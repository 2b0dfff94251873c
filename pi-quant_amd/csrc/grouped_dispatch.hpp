// Host code shared by the translation units that instantiate the grouped kernels (kernels_grouped.hip, kernels_grouped_ef.hip,
// kernels_grouped_ef_f32r.hip, kernels_grouped_reduce_ef.hip, kernels_grouped_reduce_ef_f32r.hip, kernels_grouped_requant*.hip, kernels_grouped_dequant_sum.hip, kernels_grouped_rot*.hip, kernels_grouped_clip.hip): runtime group size / types / rounding mode -> std::integral_constant, the per-call
// QuantParams, the chunk table and grids, and the launch bodies of the error-feedback kernel families and of the fused reduce kernels.
#pragma once

#include "launch.hpp"

#include "grouped_kernels.hpp"
#include "stop_event.hpp"

#include <type_traits>

namespace pq {

// compile-time dispatch of the grouped batch / reduce launches: f(std::integral_constant<int, value>) for the runtime value
template <class F>
inline void with_group_size(int64_t group_size, const char* what, F&& f) {
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
inline void with_float_type(int dt, F&& f) {
    switch (dt) {
        case DT_F32: f(std::integral_constant<int, DT_F32> {}); return;
        case DT_BF16: f(std::integral_constant<int, DT_BF16> {}); return;
        default: panic("invalid float type %d", dt);
    }
}

template <class F>
inline void with_quant_bits(int dt, F&& f) {
    switch (dt) {
        case DT_UINT8: f(std::integral_constant<int, 8> {}); return;
        case DT_UINT4: f(std::integral_constant<int, 4> {}); return;
        case DT_UINT2: f(std::integral_constant<int, 2> {}); return;
        default: panic("invalid quantized type %d", dt);
    }
}

// the rounding modes of quantize_grouped_mode: the nearest step of quantize_uniform for the pair
template <int DT_IN, int BITS, class F>
inline void with_round_mode(int round_mode, F&& f) {
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

inline QuantParams grouped_call_params(const RoundModeFields& rm) {
    QuantParams p {};
    p.threshold = rm.threshold;
    p.seed_lo = static_cast<uint32_t>(rm.seed);
    p.seed_hi = static_cast<uint32_t>(rm.seed >> 32);
    p.index_base = rm.index_base;
    return p;
}

inline unsigned grouped_blocks(int64_t chunks, const char* what) {
    const int64_t blocks = (chunks + kGroupedBlock / 64 - 1) / (kGroupedBlock / 64);
    if (blocks > 0x7fffffff) panic("%s: %lld blocks in one launch", what, static_cast<long long>(blocks));
    return static_cast<unsigned>(blocks);
}

// Grid of the guarded (element-by-element) kernels: one wave per group, grid-stride beyond 16 blocks per CU (256 CUs when num_cu is not known).
inline unsigned grouped_guarded_blocks(int64_t ngroups, int num_cu) {
    const int64_t want = (ngroups + kGroupedBlock / 64 - 1) / (kGroupedBlock / 64), cap = static_cast<int64_t>(16) * (num_cu > 0 ? num_cu : 256);
    return static_cast<unsigned>(want < cap ? want : cap);
}

// chunk_begin[] of a batch argument table whose count and numel[] are set: tensor t owns chunks [chunk_begin[t], chunk_begin[t + 1]) of
// chunk_elems elements each -- G * NG for the <G, NG> tile of a quantize kernel (NG whole groups per chunk), the tile's CHUNK_ELEMS for
// dequantize.  Returns the total.
template <class Args>
inline int64_t fill_chunk_table(Args& a, int64_t chunk_elems) {
    int64_t chunks = 0;
    for (int t = 0; t < a.count; ++t) {
        a.chunk_begin[t] = chunks;
        chunks += (a.numel[t] + chunk_elems - 1) / chunk_elems;
    }
    a.chunk_begin[a.count] = chunks;
    return chunks;
}

// Launch bodies of an error-feedback kernel family; each family's unit instantiates them once (kernels_grouped_ef.hip: the residual has the
// tensor's type; kernels_grouped_ef_f32r.hip: a bfloat16 tensor with a float32 residual).  Family::name names it in messages;
// Family::with_pipeline_type(dt_in, f) calls f(std::integral_constant<int, DT>) for the type DT that picks the tile, the rounding modes and the
// kernels; Family::single / batch <DT, BITS, MODE, G>() and Family::guarded <DT, BITS, MODE>() return the kernels.
template <class Family>
void launch_grouped_ef_batch(const GroupedEfBatchLaunch& b, hipStream_t stream) {
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("%s_batch: %d tensors, at most %d per launch", Family::name, b.count, kGroupedBatchMax);
    const QuantParams p = grouped_call_params(b.rm);
    Family::with_pipeline_type(b.dt_in, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_quant_bits(b.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT, BITS>(b.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(b.group_size, Family::name, [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT, BITS, G>::NG;
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
                    const dim3 grid(grouped_blocks(chunks, Family::name));
                    if (b.count == 1)   // the single call: its arguments arrive as leading scalars, no table
                        PQ_LAUNCH((Family::template single<DT, BITS, MODE, G>()), grid, dim3(kGroupedBlock), 0, stream, a.in[0], a.residual[0], a.out[0],
                                  a.numel[0], a.scales[0], a.zero_points[0], (a.numel[0] + G - 1) / G, p);
                    else PQ_LAUNCH((Family::template batch<DT, BITS, MODE, G>()), grid, dim3(kGroupedBlock), 0, stream, a, p);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

template <class Family>
void launch_grouped_ef_guarded(const GroupedEfLaunch& q, hipStream_t stream, int num_cu) {
    if (q.numel <= 0) return;
    const QuantParams p = grouped_call_params(q.rm);
    const int64_t ngroups = (q.numel + q.group_size - 1) / q.group_size;
    const dim3 grid(grouped_guarded_blocks(ngroups, num_cu));
    Family::with_pipeline_type(q.dt_in, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_quant_bits(q.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT, BITS>(q.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                PQ_LAUNCH((Family::template guarded<DT, BITS, MODE>()), grid, dim3(kGroupedBlock), 0, stream, q.in, q.residual, static_cast<uint8_t*>(q.out),
                          q.numel, q.group_size, q.scales, q.zero_points, ngroups, p.threshold, p.seed_lo, p.seed_hi, p.index_base);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

// Launch body of a fused reduce + quantize kernel; each of the three units instantiates it once (kernels_grouped.hip: the plain reduce;
// kernels_grouped_reduce_ef.hip: with error feedback; kernels_grouped_reduce_ef_f32r.hip: a bfloat16 accumulator with a float32 residual).
// Family::name names it in messages; Family::with_pipeline_type(dt_in, f) checks the accumulator's type and calls f(std::integral_constant<int, DT>)
// for the type DT that picks the tile and the rounding modes; Family::kernel<DT, BITS, MODE, G>() returns the kernel, which takes the residual
// behind the accumulator when Family::residual is set.
template <class Family>
void launch_grouped_reduce(const GroupedReduceLaunch& r, hipStream_t stream) {
    static_assert(kGroupedReduceMaxInputs == kGroupedReduceMaxTerms, "host and device term limits");
    if (r.numel <= 0) return;
    if (r.count < 0 || r.count > kGroupedReduceMaxTerms) panic("%s: %d terms, at most %d per launch", Family::name, r.count, kGroupedReduceMaxTerms);
    const QuantParams p = grouped_call_params(r.rm);
    GroupedTerms terms {};
    for (int i = 0; i < r.count; ++i) {
        terms.in[i] = static_cast<const uint8_t*>(r.term[i].in);
        terms.scales[i] = r.term[i].scales;
        terms.zero_points[i] = r.term[i].zero_points;
    }
    terms.count = r.count;
    const int64_t ngroups = (r.numel + r.group_size - 1) / r.group_size;
    Family::with_pipeline_type(r.dt_in, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_quant_bits(r.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT, BITS>(r.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(r.group_size, Family::name, [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT, BITS, G>::NG;
                    const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, Family::name));
                    if constexpr (Family::residual)
                        PQ_LAUNCH((Family::template kernel<DT, BITS, MODE, G>()), grid, dim3(kGroupedBlock), 0, stream, r.in, r.residual,
                                  static_cast<uint8_t*>(r.out), r.numel, r.scales, r.zero_points, ngroups, p, terms);
                    else
                        PQ_LAUNCH((Family::template kernel<DT, BITS, MODE, G>()), grid, dim3(kGroupedBlock), 0, stream, r.in, static_cast<uint8_t*>(r.out),
                                  r.numel, r.scales, r.zero_points, ngroups, p, terms);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

// Launch body of the grouped dequantize-sum, instantiated once, in kernels_grouped_dequant_sum.hip (a template like the bodies above, so that no other
// unit instantiates its kernels).  Family::name names it in messages; Family::kernel<DT_OUT, BITS, OP, G>() returns the kernel.  The grid is the
// fused reduce's: one wave per chunk of the GroupedQuantTile of the OUTPUT type.
template <class Family>
void launch_grouped_dequant_sum(const GroupedDequantSumLaunch& d, hipStream_t stream) {
    const char* name = Family::name;
    if (d.numel <= 0) return;
    if (d.count < 1 || d.count > kGroupedReduceMaxTerms) panic("%s: %d terms, 1 to %d per launch", name, d.count, kGroupedReduceMaxTerms);
    GroupedTerms terms {};
    for (int i = 0; i < d.count; ++i) {
        terms.in[i] = static_cast<const uint8_t*>(d.term[i].in);
        terms.scales[i] = d.term[i].scales;
        terms.zero_points[i] = d.term[i].zero_points;
    }
    terms.count = d.count;
    const int64_t ngroups = (d.numel + d.group_size - 1) / d.group_size;
    with_float_type(d.dt_out, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_quant_bits(d.dt_in, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_group_size(d.group_size, name, [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int NG = GroupedQuantTile<DT, BITS, G>::NG;
                const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, name));
                if (d.op == OP_ADD) PQ_LAUNCH((Family::template kernel<DT, BITS, OP_ADD, G>()), grid, dim3(kGroupedBlock), 0, stream, d.out, d.numel, ngroups, terms);
                else PQ_LAUNCH((Family::template kernel<DT, BITS, OP_SET, G>()), grid, dim3(kGroupedBlock), 0, stream, d.out, d.numel, ngroups, terms);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
