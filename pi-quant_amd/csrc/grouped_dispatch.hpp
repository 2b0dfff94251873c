// Compile-time dispatch shared by the translation units that instantiate the grouped kernels (kernels_grouped.hip, kernels_grouped_ef.hip, kernels_grouped_reduce_ef.hip):
// runtime group size / types / rounding mode -> std::integral_constant, and the per-call QuantParams.
#pragma once

#include "launch.hpp"

#include "grouped_kernels.hpp"

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

inline QuantParams grouped_call_params(float threshold, uint64_t seed, uint64_t index_base) {
    QuantParams p {};
    p.threshold = threshold;
    p.seed_lo = static_cast<uint32_t>(seed);
    p.seed_hi = static_cast<uint32_t>(seed >> 32);
    p.index_base = index_base;
    return p;
}

inline unsigned grouped_blocks(int64_t chunks, const char* what) {
    const int64_t blocks = (chunks + kGroupedBlock / 64 - 1) / (kGroupedBlock / 64);
    if (blocks > 0x7fffffff) panic("%s: %lld blocks in one launch", what, static_cast<long long>(blocks));
    return static_cast<unsigned>(blocks);
}

}  // namespace pq
