// OCP microscaling (MX) block formats for gfx950: 32 elements of FP4 E2M1 or FP8 E4M3 under one power-of-two scale byte (E8M0).  The definition is
// in include/piquant_hip.h (piquant_hip_quantize_mx); this file is the two streaming kernels, their guarded forms and the steps they share.
//
// Quantize: ONE streaming launch that reads the input once -- no scan, no atomics, no grid barrier, no block barrier.  A wave owns a tile of NV rows
// of 64 consecutive 16-byte input vectors (row r, lane l: vector r * 64 + l of the tile, one coalesced 1 KiB nt load per row, all NV issued before
// the first use).  A block is LPB consecutive lanes of one row: 8 lanes of a float32 row (8 blocks a row), 4 of a bfloat16 row (16 blocks a row).
//   amax      on the raw words: & 0x7fffffff, NaN lanes zeroed, unsigned integer max (the order of |x| for everything that is not a NaN) over the
//             lane's elements, then over the block's lanes by DPP exchanges: row_half_mirror (lane i <- lane 7 - i of its run of 8) and the two
//             quad permutes -- VALU only, no LDS traffic
//   scale     s = max((amax >> 23) - emax, 0): integer arithmetic on the exponent field (a denormal amax has field 0, an infinite one 255)
//   codes     v_cvt_scalef32_pk_fp4_f32 / v_cvt_scalef32_pk_fp8_f32 with the float whose bits are s << 23 as the scale operand.  Two things are
//             added to make the instructions agree with the definition (tools/probe_mx_cvt.hip): a NaN input is replaced by +0 in front
//             of the FP4 conversion (the instruction gives +-6), and behind the FP8 conversion -- which does NOT saturate: anything above 464 in the
//             scaled domain and an infinity come out as the NaN byte -- the NaN bytes of lanes whose input was no NaN are stepped down to +-448
//             (mx_fp8_saturate: the byte minus one, four codes a dword).  Denormal inputs and s = 0 need nothing.
//   stores    a lane has OB = 2 .. 8 code bytes per row, so the tile's codes are transposed through the wave's own LDS slice (same-wave ordering,
//             wave_lds_sync) and leave as 16-byte-per-lane write-through stores; the lane that starts a block parks the block's scale byte in the
//             slice too, and the tile's 32 or 64 scale bytes leave as one contiguous run of 16-byte stores.
// A ragged last tile reads the missing elements as quiet NaNs (grouped_load), which change no amax and encode to nibble 0 in FP4, and stops its
// stores at the tensor's last code byte and last scale byte.
//
// Dequantize, the mirror image: a wave owns 2 KiB of codes (two 16-byte nt loads per lane), staged through its LDS slice so that every lane ends with
// the codes of its own 16-byte output vector; the tile's 64 (FP8) or 128 (FP4) scale bytes are loaded once into the slice.  The conversions are
// v_cvt_scalef32_pk_f32_{fp4,fp8} and, for a bfloat16 SET, v_cvt_scalef32_pk_bf16_{fp4,fp8}, again with s << 23 as the scale operand: every code
// under every scale byte agrees with the definition as it is (s = 0, s = 0xFF -> NaN, NaN codes, overflow to infinity, denormal results and their
// bfloat16 rounding included), nothing is added.  ADD is the grouped dequantize's: __fadd_rn in float32, bfloat16 then rounded once.
#pragma once

#include "grouped_kernels.hpp"

#include <type_traits>

namespace pq {

typedef short s16x2 __attribute__((ext_vector_type(2)));

constexpr int kMxBlock = 32;   // the format codes MX_FP4_E2M1 / MX_FP8_E4M3: launch.hpp

template <int FMT>
struct MxFormat {
    static constexpr int BITS = FMT == MX_FP4_E2M1 ? 4 : 8;
    static constexpr int EMAX = FMT == MX_FP4_E2M1 ? 2 : 8;
};

// f(std::integral_constant<int, J>) for J = 0 .. N - 1: the conversions take their byte / word selector as an immediate
template <int J, int N, class F>
__device__ __forceinline__ void mx_static_for(F&& f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J> {});
        mx_static_for<J + 1, N>(f);
    }
}

__device__ __forceinline__ bool mx_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

// |x| as an unsigned key, 0 for a NaN: its unsigned order is the order of |x|
__device__ __forceinline__ uint32_t mx_abs_key(uint32_t bits) { return mx_is_nan(bits) ? 0u : bits & 0x7fffffffu; }

// the maximum over aligned runs of LPB = 4 or 8 lanes; every lane of a run ends with it
template <int LPB>
__device__ __forceinline__ uint32_t mx_block_max(uint32_t key) {
    static_assert(LPB == 4 || LPB == 8, "a block is 8 lanes of a float32 row or 4 of a bfloat16 row");
    auto dpp = [](uint32_t x, auto ctrl) {
        const int i = static_cast<int>(x);
        return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(i, i, decltype(ctrl)::value, 0xf, 0xf, false));
    };
    auto umax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    if constexpr (LPB == 8) key = umax(key, dpp(key, std::integral_constant<int, 0x141> {}));   // row_half_mirror
    key = umax(key, dpp(key, std::integral_constant<int, 0xb1> {}));                           // quad_perm [1,0,3,2]
    return umax(key, dpp(key, std::integral_constant<int, 0x4e> {}));                          // quad_perm [2,3,0,1]
}

template <int FMT>
__device__ __forceinline__ uint32_t mx_scale_byte(uint32_t amax_key) {
    const int s = static_cast<int>(amax_key >> 23) - MxFormat<FMT>::EMAX;   // max(E, 1) - emax is below 0 wherever E - emax is
    return static_cast<uint32_t>(s > 0 ? s : 0);
}

__device__ __forceinline__ float mx_scale_operand(uint32_t s) { return __uint_as_float(s << 23); }

// ---- stochastic rounding: what the RM = MX_SR instantiations add ---------------------------------------------------------------------------------
enum : int { MX_RN = 0, MX_SR = 1 };

// The four element formats as the rounding sees them: mantissa bits, the exponent of the smallest normal, emax and the mantissa field (float32) of
// the largest magnitude (6, 448, 7.5, 28).
template <int FMT>
struct MxSrFormat {
    static constexpr int MBITS = FMT == MX_FP4_E2M1 ? 1 : FMT == MX_FP6_E3M2 ? 2 : 3;
    static constexpr int EMIN = FMT == MX_FP8_E4M3 ? -6 : FMT == MX_FP6_E3M2 ? -2 : 0;
    static constexpr int EMAX = FMT == MX_FP8_E4M3 ? 8 : FMT == MX_FP6_E3M2 ? 4 : 2;
    static constexpr uint32_t TOP_MANT = FMT == MX_FP4_E2M1 ? 0x400000u : FMT == MX_FP6_E2M3 ? 0x700000u : 0x600000u;
};

// The scale byte with headroom: one more than max(E - emax, 0) when the finite amax (key: mx_abs_key's, exponent field E >= emax) has a mantissa
// above the top magnitude's, so that no finite element exceeds the top in the scaled domain.
template <int FMT>
__device__ __forceinline__ uint32_t mx_sr_scale_byte(uint32_t amax_key) {
    using F = MxSrFormat<FMT>;
    const int s = static_cast<int>(amax_key >> 23) - F::EMAX;
    const bool bump = s >= 0 && amax_key < 0x7f800000u && (amax_key & 0x7fffffu) > F::TOP_MANT;
    return static_cast<uint32_t>(s > 0 ? s : 0) + (bump ? 1u : 0u);
}

// The keys of the counter hash (device_math.hpp: element_key) a tile can meet, from the global index g0 of its first element: the tile is far
// shorter than 2^32 elements, so an element's upper half is g0's or the next one -- the next exactly when the lower half has wrapped.
struct MxSrKeys {
    uint32_t lo0, key0, key1;
};

__device__ __forceinline__ MxSrKeys mx_sr_keys(uint64_t seed, uint64_t g0) {
    const uint32_t seed_lo = static_cast<uint32_t>(seed), seed_hi = static_cast<uint32_t>(seed >> 32), hi0 = static_cast<uint32_t>(g0 >> 32);
    return {static_cast<uint32_t>(g0), mix32(hi0 ^ seed_hi) + seed_lo, mix32((hi0 + 1u) ^ seed_hi) + seed_lo};
}

// floor(element_threshold(seed, g0 + off) * 2^24)
__device__ __forceinline__ uint32_t mx_sr_threshold(const MxSrKeys& k, uint32_t off) {
    const uint32_t lo = k.lo0 + off;
    return mix32(lo ^ (lo < k.lo0 ? k.key1 : k.key0)) >> 8;
}

// x (float32 bits) under scale byte s -> the float32 bits of its stochastically rounded value IN THE SCALED DOMAIN, x's sign kept: a magnitude the
// format holds exactly (its denormals included), so that the nearest conversion under the scale operand 1.0 only encodes it.  t is the element's
// 24-bit hash word.  With v = |x| * 2^(127 - s) in the binade of exponent field kf, the format's step there is 2^(e - 127 - MBITS), e = max(kf,
// EMIN + 127); w = floor(v / step * 2^24) = (significand << (MBITS + 1)) >> (e - kf), and (w + t) >> 24 is the definition's choice between lo and
// hi in units of the step.  A v below 2^-126 (kf = 0, also a rounded-off ldexp) is more than 2^24 steps below the first one and gives 0 like every
// w < 2^24 - t.  Infinities and NaNs pass through for the conversion and its fix-ups.
template <int FMT>
__device__ __forceinline__ uint32_t mx_sr_round(uint32_t x, uint32_t s, uint32_t t) {
    using F = MxSrFormat<FMT>;
    constexpr int FMIN = F::EMIN + 127;
    const uint32_t v = __float_as_uint(__builtin_amdgcn_ldexpf(__uint_as_float(x & 0x7fffffffu), 127 - static_cast<int>(s)));
    const int kf = static_cast<int>(v >> 23);
    const int e = kf > FMIN ? kf : FMIN;
    const int d = e - kf < 31 ? e - kf : 31;
    const uint32_t w = (((v & 0x7fffffu) | 0x800000u) << (F::MBITS + 1)) >> d;
    const uint32_t m = (w + t) >> 24;                               // 0 .. 2^(MBITS + 1), in steps
    const uint32_t r = m == 0 ? 0u : __float_as_uint(static_cast<float>(m)) + (static_cast<uint32_t>(e - 127 - F::MBITS) << 23);
    return (kf == 255 ? v : r) | (x & 0x80000000u);
}

// Behind the FP8 conversion: w holds four codes; notnan has 0x01 in byte j when element j was no NaN.  A NaN byte (0x7f / 0xff) of such an
// element stands for "above 464" or an infinity: one less is the largest finite code of its sign.  No borrow leaves a byte.
__device__ __forceinline__ uint32_t mx_fp8_saturate(uint32_t w, uint32_t notnan) {
    const uint32_t nan_byte = (((w & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u) >> 7;
    return w - (nan_byte & notnan);
}

// The codes of the N = 4 or 8 elements whose float32 bits are in x, under scale byte s: N * BITS / 8 bytes, element 0 lowest, in w
// RM = MX_SR: t holds the elements' hash words; every element is rounded in the scaled domain first (mx_sr_round) and encoded under scale byte 127.
template <int FMT, int N, int RM = MX_RN>
__device__ __forceinline__ void mx_encode(const uint32_t (&x)[N], uint32_t s, uint32_t (&w)[N * MxFormat<FMT>::BITS > 32 ? 2 : 1], const uint32_t* t = nullptr) {
    if constexpr (RM == MX_SR) {
        uint32_t y[N];
#pragma unroll
        for (int e = 0; e < N; ++e) y[e] = mx_sr_round<FMT>(x[e], s, t[e]);
        mx_encode<FMT, N>(y, 127u, w);
        return;
    }
    const float scale = mx_scale_operand(s);
    if constexpr (FMT == MX_FP4_E2M1) {
        uint32_t r = 0;
        mx_static_for<0, N / 2>([&](auto j) {
            constexpr int J = decltype(j)::value;
            const uint32_t a = mx_is_nan(x[2 * J]) ? 0u : x[2 * J], b = mx_is_nan(x[2 * J + 1]) ? 0u : x[2 * J + 1];
            r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, __uint_as_float(a), __uint_as_float(b), scale, J);
        });
        w[0] = r;
    } else {
        mx_static_for<0, N / 4>([&](auto j) {
            constexpr int J = decltype(j)::value;
            s16x2 r {0, 0};
            r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, __uint_as_float(x[4 * J]), __uint_as_float(x[4 * J + 1]), scale, false);
            r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, __uint_as_float(x[4 * J + 2]), __uint_as_float(x[4 * J + 3]), scale, true);
            const uint32_t notnan = (mx_is_nan(x[4 * J]) ? 0u : 0x1u) | (mx_is_nan(x[4 * J + 1]) ? 0u : 0x100u) | (mx_is_nan(x[4 * J + 2]) ? 0u : 0x10000u) |
                                    (mx_is_nan(x[4 * J + 3]) ? 0u : 0x1000000u);
            w[J] = mx_fp8_saturate(__builtin_bit_cast(uint32_t, r), notnan);
        });
    }
}

// elements 2 J and 2 J + 1 of the codes in w (element 0 lowest) under the scale operand, as float32
template <int FMT, int J, int WORDS>
__device__ __forceinline__ f32x2 mx_decode_pair(const uint32_t (&w)[WORDS], float scale) {
    if constexpr (FMT == MX_FP4_E2M1) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[J / 4], scale, J % 4);
    else return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[J / 2], scale, (J & 1) != 0);
}

// the same as two bfloat16 in a dword: RNE_bf16 of the float32 value (the instruction's own rounding is that one)
template <int FMT, int J, int WORDS>
__device__ __forceinline__ uint32_t mx_decode_pair_bf16(const uint32_t (&w)[WORDS], float scale) {
    if constexpr (FMT == MX_FP4_E2M1) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[J / 4], scale, J % 4));
    else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[J / 2], scale, (J & 1) != 0));
}

template <int DT_IN, int FMT>
struct MxQuantTile {
    static constexpr int EPV = InVec<DT_IN>::EPV;
    static constexpr int BITS = MxFormat<FMT>::BITS;
    static constexpr int OB = EPV * BITS / 8;                       // code bytes per input vector: 2, 4, 4, 8
    static constexpr int LPB = kMxBlock / EPV;                      // lanes per block
    static constexpr int BPR = 64 / LPB;                            // blocks per row
    static constexpr int NV = (16 / OB) > 4 ? 16 / OB : 4;          // rows: 16 code bytes per lane, at least 4 loads in flight
    static constexpr int TILE_ELEMS = NV * 64 * EPV;                // 2048 (1024 for float32 -> FP8)
    static constexpr int OUT_BYTES = NV * 64 * OB;
    static constexpr int NB = NV * BPR;                             // blocks, and scale bytes, per tile: 64 (32 for float32 -> FP8)
    static_assert((NV * OB) % 16 == 0 && NB % 16 == 0, "16-byte stores of the staged codes and scales");
};

template <int DT_IN>
__device__ __forceinline__ void mx_unpack_bits(const u32x4& raw, uint32_t (&x)[InVec<DT_IN>::EPV]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (DT_IN == DT_F32) {
            x[e] = raw[e];
        } else {
            x[2 * e] = raw[e] << 16;                                // low half = lower index
            x[2 * e + 1] = raw[e] & 0xffff0000u;
        }
    }
}

// The tile's NV rows in `raw` (grouped_load: elements at or past numel are quiet NaNs) -> its codes and scale bytes, staged through the wave's LDS
// slices and stored.  Shared by the single kernel, the batch (kernels_mx_batch.hip) and the fused reduce (mx_reduce_kernels.hpp).  RM = MX_SR: keys
// are mx_sr_keys of the global index of the tile's first element.
template <int DT_IN, int FMT, int RM = MX_RN>
__device__ __forceinline__ void mx_quantize_rows(const u32x4 (&raw)[MxQuantTile<DT_IN, FMT>::NV], uint8_t* __restrict__ codes, uint8_t* __restrict__ scales,
                                                 int64_t numel, int64_t nblocks, int64_t tile, bool full, int lane, uint8_t* stage, uint8_t* stage_scales,
                                                 [[maybe_unused]] const MxSrKeys& keys = {}) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int EPV = T::EPV, OB = T::OB, NV = T::NV, LPB = T::LPB, BPR = T::BPR, NB = T::NB;
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        uint32_t x[EPV];
        mx_unpack_bits<DT_IN>(raw[r], x);
        uint32_t key = mx_abs_key(x[0]);
#pragma unroll
        for (int e = 1; e < EPV; ++e) {
            const uint32_t k = mx_abs_key(x[e]);
            key = k > key ? k : key;
        }
        const uint32_t s = RM == MX_SR ? mx_sr_scale_byte<FMT>(mx_block_max<LPB>(key)) : mx_scale_byte<FMT>(mx_block_max<LPB>(key));
        if (lane % LPB == 0) stage_scales[r * BPR + lane / LPB] = static_cast<uint8_t>(s);
        uint32_t w[OB > 4 ? 2 : 1];
        if constexpr (RM == MX_SR) {
            uint32_t t[EPV];
#pragma unroll
            for (int e = 0; e < EPV; ++e) t[e] = mx_sr_threshold(keys, static_cast<uint32_t>((r * 64 + lane) * EPV + e));
            mx_encode<FMT, EPV, MX_SR>(x, s, w, t);
        } else {
            mx_encode<FMT, EPV>(x, s, w);
        }
        uint8_t* dst = stage + (r * 64 + lane) * OB;
        if constexpr (OB == 2) *reinterpret_cast<uint16_t*>(dst) = static_cast<uint16_t>(w[0]);
        else if constexpr (OB == 4) *reinterpret_cast<uint32_t*>(dst) = w[0];
        else *reinterpret_cast<u32x2*>(dst) = u32x2 {w[0], w[1]};
    }
    wave_lds_sync();

    uint8_t* o = codes + tile * T::OUT_BYTES;
    uint8_t* osc = scales + tile * NB;
    if (full) {
#pragma unroll
        for (int j = 0; j < NV * OB / 16; ++j) st<ST_WT>(reinterpret_cast<u32x4*>(o) + j * 64 + lane, reinterpret_cast<const u32x4*>(stage)[j * 64 + lane]);
        if (lane < NB / 16) st<ST_WT>(reinterpret_cast<u32x4*>(osc) + lane, reinterpret_cast<const u32x4*>(stage_scales)[lane]);
    } else {
        const int64_t left = (numel * T::BITS + 7) / 8 - tile * T::OUT_BYTES;   // code bytes of the tensor from the tile's first on (< OUT_BYTES)
        for (int b = lane; b < left; b += 64) o[b] = stage[b];
        const int64_t blocks_left = nblocks - tile * NB;
        for (int b = lane; b < NB && b < blocks_left; b += 64) osc[b] = stage_scales[b];
    }
}

// one wave's tile of one tensor (tile * TILE_ELEMS < numel): load, then mx_quantize_rows
template <int DT_IN, int FMT, int RM = MX_RN>
__device__ __forceinline__ void mx_quantize_tile(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel,
                                                 int64_t nblocks, int64_t tile, int lane, uint8_t* stage, uint8_t* stage_scales, uint64_t seed = 0,
                                                 uint64_t index_base = 0) {
    using T = MxQuantTile<DT_IN, FMT>;
    const int64_t e0 = tile * T::TILE_ELEMS;
    const bool full = e0 + T::TILE_ELEMS <= numel;                  // wave-uniform
    u32x4 raw[T::NV];
    grouped_load<DT_IN, T::NV>(in, numel, e0 / T::EPV, lane, full, raw);
    if constexpr (RM == MX_SR)
        mx_quantize_rows<DT_IN, FMT, MX_SR>(raw, codes, scales, numel, nblocks, tile, full, lane, stage, stage_scales,
                                            mx_sr_keys(seed, index_base + static_cast<uint64_t>(e0)));
    else mx_quantize_rows<DT_IN, FMT>(raw, codes, scales, numel, nblocks, tile, full, lane, stage, stage_scales);
}

template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::OUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    if (tile * T::TILE_ELEMS >= numel) return;
    mx_quantize_tile<DT_IN, FMT>(in, codes, scales, numel, nblocks, tile, lane, s_codes[wave], s_scales[wave]);
}

// The same launch with stochastic rounding: element i has global index index_base + i (seed and base by value: capturable).
template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_sr_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks, uint64_t seed,
                      uint64_t index_base) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::OUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    if (tile * T::TILE_ELEMS >= numel) return;
    mx_quantize_tile<DT_IN, FMT, MX_SR>(in, codes, scales, numel, nblocks, tile, lane, s_codes[wave], s_scales[wave], seed, index_base);
}

// element i of a float32 / bfloat16 tensor as float32 bits
template <int DT>
__device__ __forceinline__ uint32_t mx_load_bits(const void* in, int64_t i) {
    if constexpr (DT == DT_F32) return static_cast<const uint32_t*>(in)[i];
    else return static_cast<uint32_t>(static_cast<const uint16_t*>(in)[i]) << 16;
}

// Guarded form for buffers that are not 16-byte aligned: a thread per block, element by element, through the same steps -- the same bytes.
template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_guarded_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; b < nblocks; b += stride) {
        const int64_t i0 = b * kMxBlock;
        const int n = numel - i0 < kMxBlock ? static_cast<int>(numel - i0) : kMxBlock;
        uint32_t key = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t k = mx_abs_key(mx_load_bits<DT_IN>(in, i0 + j));
            key = k > key ? k : key;
        }
        const uint32_t s = mx_scale_byte<FMT>(key);
        scales[b] = static_cast<uint8_t>(s);
        for (int j = 0; j < n; j += 4) {
            uint32_t x[4], w[1];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = j + e < n ? mx_load_bits<DT_IN>(in, i0 + j + e) : 0u;
            mx_encode<FMT, 4>(x, s, w);
            if constexpr (FMT == MX_FP4_E2M1) {
                codes[(i0 + j) / 2] = static_cast<uint8_t>(w[0]);
                if (j + 2 < n) codes[(i0 + j) / 2 + 1] = static_cast<uint8_t>(w[0] >> 8);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < n) codes[i0 + j + e] = static_cast<uint8_t>(w[0] >> (8 * e));
            }
        }
    }
}

// The guarded form with stochastic rounding: the same loop, the headroom scale byte and the hash words from the block's own keys.
template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_sr_guarded_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks,
                              uint64_t seed, uint64_t index_base) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; b < nblocks; b += stride) {
        const int64_t i0 = b * kMxBlock;
        const int n = numel - i0 < kMxBlock ? static_cast<int>(numel - i0) : kMxBlock;
        uint32_t key = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t k = mx_abs_key(mx_load_bits<DT_IN>(in, i0 + j));
            key = k > key ? k : key;
        }
        const uint32_t s = mx_sr_scale_byte<FMT>(key);
        const MxSrKeys keys = mx_sr_keys(seed, index_base + static_cast<uint64_t>(i0));
        scales[b] = static_cast<uint8_t>(s);
        for (int j = 0; j < n; j += 4) {
            uint32_t x[4], t[4], w[1];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = j + e < n ? mx_load_bits<DT_IN>(in, i0 + j + e) : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = mx_sr_threshold(keys, static_cast<uint32_t>(j + e));
            mx_encode<FMT, 4, MX_SR>(x, s, w, t);
            if constexpr (FMT == MX_FP4_E2M1) {
                codes[(i0 + j) / 2] = static_cast<uint8_t>(w[0]);
                if (j + 2 < n) codes[(i0 + j) / 2 + 1] = static_cast<uint8_t>(w[0] >> 8);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < n) codes[i0 + j + e] = static_cast<uint8_t>(w[0] >> (8 * e));
            }
        }
    }
}

template <int FMT, int DT_OUT>
struct MxDequantTile {
    static constexpr int BITS = MxFormat<FMT>::BITS;
    static constexpr int PACK = 8 / BITS;
    static constexpr int EPV = DT_OUT == DT_F32 ? 4 : 8;           // elements per 16-byte output vector
    static constexpr int IB = EPV * BITS / 8;                       // code bytes per output vector: 2, 4, 4, 8
    static constexpr int NIN = 2;                                   // 16-byte input rows per lane
    static constexpr int TILE_BYTES = NIN * 64 * 16;
    static constexpr int TILE_ELEMS = TILE_BYTES * PACK;            // 4096 (FP4), 2048 (FP8)
    static constexpr int OV = NIN * 16 / IB;                        // output vectors per lane
    static constexpr int NB = TILE_ELEMS / kMxBlock;                // blocks, and scale bytes, per tile: 128, 64
};

// out[i] (op)= d, one element (the end of a ragged tile, and the guarded kernel)
template <int DT_OUT, int OP>
__device__ __forceinline__ void mx_store_one(void* out, int64_t i, float d) {
    if constexpr (DT_OUT == DT_F32) {
        float* o = static_cast<float*>(out);
        o[i] = OP == OP_ADD ? __fadd_rn(d, o[i]) : d;
    } else {
        uint16_t* o = static_cast<uint16_t*>(out);
        o[i] = static_cast<uint16_t>(f32_to_bf16_bits(OP == OP_ADD ? __fadd_rn(d, bf16_bits_to_f32(o[i])) : d));
    }
}

// one wave's tile of one tensor (tile * TILE_ELEMS < numel).  Shared by the single kernel and the batch (kernels_mx_batch.hip).
template <int FMT, int DT_OUT, int OP>
__device__ __forceinline__ void mx_dequantize_tile(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, void* __restrict__ out, int64_t numel,
                                                   int64_t nblocks, int64_t tile, int lane, uint8_t* stage, uint8_t* stage_scales) {
    using T = MxDequantTile<FMT, DT_OUT>;
    constexpr int EPV = T::EPV, IB = T::IB, NB = T::NB, WORDS = IB > 4 ? 2 : 1;
    const int64_t e0 = tile * T::TILE_ELEMS;
    const bool full = e0 + T::TILE_ELEMS <= numel;                  // wave-uniform
    const int64_t b0 = tile * T::TILE_BYTES, nbytes = (numel * T::BITS + 7) / 8;

    u32x4 raw[T::NIN];
#pragma unroll
    for (int k = 0; k < T::NIN; ++k) {
        const int64_t off = b0 + (k * 64 + lane) * 16;
        if (full) {
            raw[k] = ld<true>(reinterpret_cast<const u32x4*>(codes + off));
        } else {
            raw[k] = u32x4 {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (off + j < nbytes) raw[k][j >> 2] |= static_cast<uint32_t>(codes[off + j]) << ((j & 3) * 8);
        }
    }
    if (full) {                                                     // the tile's scale bytes, once
        if (lane < NB / 4) reinterpret_cast<uint32_t*>(stage_scales)[lane] = ld<true>(reinterpret_cast<const uint32_t*>(scales + tile * NB) + lane);
    } else {
        for (int j = lane; j < NB; j += 64)
            if (tile * NB + j < nblocks) stage_scales[j] = scales[tile * NB + j];
    }
#pragma unroll
    for (int k = 0; k < T::NIN; ++k) reinterpret_cast<u32x4*>(stage)[k * 64 + lane] = raw[k];
    wave_lds_sync();

    u32x4* out16 = reinterpret_cast<u32x4*>(static_cast<uint8_t*>(out) + e0 * (DT_OUT == DT_F32 ? 4 : 2));
#pragma unroll
    for (int k = 0; k < T::OV; ++k) {
        const int c = k * 64 + lane;                                // output vector of the tile
        const int ce = c * EPV;                                     // its first element, relative to e0
        if (!full && e0 + ce >= numel) continue;
        const bool whole = full || e0 + ce + EPV <= numel;          // otherwise the tensor ends inside this vector
        const float scale = mx_scale_operand(stage_scales[ce / kMxBlock]);
        uint32_t w[WORDS];
        staged_words<IB>(stage + c * IB, w);
        if constexpr (DT_OUT == DT_BF16 && OP == OP_SET) {
            u32x4 r;
            mx_static_for<0, 4>([&](auto j) { r[decltype(j)::value] = mx_decode_pair_bf16<FMT, decltype(j)::value>(w, scale); });
            if (whole) {
                st<ST_WT>(out16 + c, r);
            } else {
#pragma unroll
                for (int e = 0; e < EPV; ++e)
                    if (e0 + ce + e < numel) static_cast<uint16_t*>(out)[e0 + ce + e] = static_cast<uint16_t>(r[e >> 1] >> ((e & 1) * 16));
            }
        } else {
            float f[EPV];
            mx_static_for<0, EPV / 2>([&](auto j) {
                constexpr int J = decltype(j)::value;
                const f32x2 p = mx_decode_pair<FMT, J>(w, scale);
                f[2 * J] = p[0];
                f[2 * J + 1] = p[1];
            });
            if (whole) {
                u32x4 r;
                u32x4 old {};
                if constexpr (OP == OP_ADD) old = ld<false>(out16 + c);
                if constexpr (DT_OUT == DT_F32) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = __float_as_uint(OP == OP_ADD ? __fadd_rn(f[e], __uint_as_float(old[e])) : f[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        r[e] = f32x2_to_bf16x2_bits(__fadd_rn(f[2 * e], __uint_as_float(old[e] << 16)), __fadd_rn(f[2 * e + 1], __uint_as_float(old[e] & 0xffff0000u)));
                }
                st<ST_WT>(out16 + c, r);
            } else {
#pragma unroll
                for (int e = 0; e < EPV; ++e)
                    if (e0 + ce + e < numel) mx_store_one<DT_OUT, OP>(out, e0 + ce + e, f[e]);
            }
        }
    }
}

template <int FMT, int DT_OUT, int OP>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_mx_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, void* __restrict__ out, int64_t numel, int64_t nblocks) {
    using T = MxDequantTile<FMT, DT_OUT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::TILE_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    if (tile * T::TILE_ELEMS >= numel) return;
    mx_dequantize_tile<FMT, DT_OUT, OP>(codes, scales, out, numel, nblocks, tile, lane, s_codes[wave], s_scales[wave]);
}

// Guarded form for buffers that are not 16-byte aligned: element by element, the same bytes.
template <int FMT, int DT_OUT, int OP>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_mx_guarded_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, void* __restrict__ out, int64_t numel) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; i < numel; i += stride) {
        uint32_t w[1];
        if constexpr (FMT == MX_FP4_E2M1) w[0] = (codes[i >> 1] >> ((i & 1) * 4)) & 0xfu;
        else w[0] = codes[i];
        mx_store_one<DT_OUT, OP>(out, i, mx_decode_pair<FMT, 0>(w, mx_scale_operand(scales[i / kMxBlock]))[0]);
    }
}

}  // namespace pq
