// MXFP6 for gfx950: 32 elements of FP6 E2M3 or E3M2 under one E8M0 scale byte, the codes a dense string of 6-bit fields (a block is 24 bytes).  The
// definition is in include/piquant_hip.h (piquant_hip_quantize_mx); this file is the two streaming kernels, their guarded forms and the conversion
// helpers they share.  The gfx950 FP6 conversions take a whole block from ONE lane and return (or take) its 6 dwords, so the tile is not the FP4 / FP8
// tile of mx_kernels.hpp (a block spread over 8 or 4 lanes of a row): here a wave owns 2048 elements = 64 blocks, one block per lane, and the rows
// of coalesced 16-byte accesses are transposed through the wave's own LDS slice on the way in (quantize) or out (dequantize).
//
// Quantize: ONE streaming launch that reads the input once -- no scan, no atomics, no grid barrier, no block barrier.
//   loads     8 (float32) or 4 (bfloat16) rows of 64 16-byte nt loads, all issued before the first use; grouped_load fills a ragged tile with quiet NaNs
//   transpose vector v = r * 64 + lane of the tile belongs to block v / 8 (v / 4); a block's bytes are contiguous in the slice and blocks are 144 (80)
//             bytes apart: the 16 pad bytes make the lane stride 36 (20) banks, so the 16 lanes of one ds_read_b128 phase start at 16 different
//             multiples of 4 banks -- the read-back of 128 (64) bytes per lane does not serialise.  A float32 vector is stored as its two even
//             elements and, 64 bytes on, its two odd ones: v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 INTERLEAVES its operands (field 2 j is element j of
//             the first, field 2 j + 1 element j of the second; tools/probe_mx_fp6_cvt.hip), so the lane reads the first operand from the block's
//             first 64 bytes and the second from the next 64 with no register shuffling.  v_cvt_scalef32_pk32_{fp6,bf6}_bf16 takes the 16 packed
//             dwords in order.
//   amax      in the lane, on the integer keys: the unsigned maximum of the words without their sign bits (v_pk_max_u16 on the packed bfloat16
//             halves).  Only when that is above the infinity pattern does the lane hold a NaN: then the NaNs are replaced by +0 -- the conversions
//             encode a NaN as the largest magnitude of its sign, the definition says code 0 -- and the maximum is taken again without them.
//   scale     s = max(E(amax) - emax, 0), integer arithmetic on the exponent field; the scale operand is the float with bits s << 23
//   codes     one conversion per block.  Saturation (also of an infinity), ties to even, denormal inputs and s = 0 agree with the definition as
//             they are (the probe); nothing but the NaN replacement is added.
//   stores    the 64 x 24 code bytes and the 64 scale bytes go back into the slice and leave as 96 + 4 16-byte write-through stores.
// Dequantize, the mirror image: the tile's 1536 code bytes are 96 16-byte nt loads staged in the slice, lane l reads its 24 bytes and loads its scale
// byte, converts once (v_cvt_scalef32_pk32_f32_{fp6,bf6}; v_cvt_scalef32_pk32_bf16_{fp6,bf6} for a bfloat16 SET: every code under every scale byte,
// s = 0 and s = 0xFF -> NaN included, agrees with the definition) and writes its 128 (64) bytes back at the padded stride; the rows of 16-byte vectors
// are read out of that, an ADD's `out` -- loaded in row layout before anything else -- is added with __fadd_rn (bfloat16 rounded once, from the
// float32 sum), and the rows leave as write-through stores.
#pragma once

#include "mx_kernels.hpp"

namespace pq {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef __bf16 bf16x32 __attribute__((ext_vector_type(32)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

constexpr int kMx6TileElems = 2048;                                 // 64 blocks, one per lane
constexpr int kMx6BlockBytes = 24;
constexpr int kMx6TileBytes = 64 * kMx6BlockBytes;                  // 1536

template <int FMT>
struct Mx6Format {
    static_assert(FMT == MX_FP6_E2M3 || FMT == MX_FP6_E3M2, "the FP6 formats");
    static constexpr int EMAX = FMT == MX_FP6_E2M3 ? 2 : 4;
};

// The slice of a wave: 64 blocks of BLOCK_BYTES float bytes, STRIDE apart.  The codes (1536 bytes) and scale bytes (64, behind them) share it.
template <int BLOCK_BYTES>
struct Mx6Slice {
    static_assert(BLOCK_BYTES == 128 || BLOCK_BYTES == 64, "32 float32 or 32 bfloat16");
    static constexpr int STRIDE = BLOCK_BYTES + 16;
    static constexpr int BYTES = 64 * STRIDE;                       // 9216 / 5120
    static constexpr int SCALES_AT = kMx6TileBytes;
    static_assert(SCALES_AT + 64 <= BYTES, "codes and scale bytes fit the slice");
};

// The number of words the 32 elements of a block are held in: float32 bits, or bfloat16 pairs (the lower index in the low half).
template <int DT>
constexpr int kMx6Words = DT == DT_F32 ? 32 : 16;

// The block in w -> its scale byte s and its 6 dwords c (the definition's string).  float32: w[j] is element 2 j and w[16 + j] element 2 j + 1,
// j = 0 .. 15 (the two operands of 2xpk16); bfloat16: w[j] holds elements 2 j and 2 j + 1.  NaNs in w are replaced by +0.
template <int FMT, int DT_IN>
__device__ __forceinline__ void mx6_encode(uint32_t (&w)[kMx6Words<DT_IN>], uint32_t& s, u32x6& c) {
    constexpr int EMAX = Mx6Format<FMT>::EMAX;
    if constexpr (DT_IN == DT_F32) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const uint32_t k = w[i] & 0x7fffffffu;
            m = k > m ? k : m;
        }
        if (m > 0x7f800000u) {                                      // a NaN in the block: rare (and the filling of a ragged tile)
            m = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                if (mx_is_nan(w[i])) w[i] = 0u;
                const uint32_t k = w[i] & 0x7fffffffu;
                m = k > m ? k : m;
            }
        }
        const int e = static_cast<int>(m >> 23) - EMAX;
        s = static_cast<uint32_t>(e > 0 ? e : 0);
        f32x16 a, b;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            a[j] = __uint_as_float(w[j]);
            b[j] = __uint_as_float(w[16 + j]);
        }
        if constexpr (FMT == MX_FP6_E2M3) c = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, mx_scale_operand(s));
        else c = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, mx_scale_operand(s));
    } else {
        u16x2 m2 {0, 0};
#pragma unroll
        for (int i = 0; i < 16; ++i) m2 = __builtin_elementwise_max(m2, __builtin_bit_cast(u16x2, w[i] & 0x7fff7fffu));
        uint32_t m = m2[0] > m2[1] ? m2[0] : m2[1];
        if (m > 0x7f80u) {
            m = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if ((w[i] & 0x7fffu) > 0x7f80u) w[i] &= 0xffff0000u;
                if ((w[i] & 0x7fff0000u) > 0x7f800000u) w[i] &= 0x0000ffffu;
                const uint32_t lo = w[i] & 0x7fffu, hi = (w[i] >> 16) & 0x7fffu;
                m = lo > m ? lo : m;
                m = hi > m ? hi : m;
            }
        }
        const int e = static_cast<int>(m >> 7) - EMAX;              // the exponent field of a bfloat16 key
        s = static_cast<uint32_t>(e > 0 ? e : 0);
        u32x16 p;
#pragma unroll
        for (int j = 0; j < 16; ++j) p[j] = w[j];
        if constexpr (FMT == MX_FP6_E2M3) c = __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(bf16x32, p), mx_scale_operand(s));
        else c = __builtin_amdgcn_cvt_scalef32_pk32_bf6_bf16(__builtin_bit_cast(bf16x32, p), mx_scale_operand(s));
    }
}

// The same with stochastic rounding (keys: mx_sr_keys of the global index of the block's first element): the scale byte with headroom, every element
// rounded in the scaled domain (mx_sr_round; bfloat16 widened first, which is exact) and the float32 conversion under the scale operand 1.0 for both
// input types -- v_cvt_scalef32_sr_pk32_* draws ONE random word for its 32 elements and cannot follow the definition.
template <int FMT, int DT_IN>
__device__ __forceinline__ void mx6_encode_sr(const uint32_t (&w)[kMx6Words<DT_IN>], const MxSrKeys& keys, uint32_t& s, u32x6& c) {
    auto elem = [&](int i) {                                        // the float32 bits of element i, a NaN replaced by +0
        uint32_t x;
        if constexpr (DT_IN == DT_F32) x = w[(i & 1) * 16 + (i >> 1)];
        else x = i & 1 ? w[i >> 1] & 0xffff0000u : w[i >> 1] << 16;
        return mx_is_nan(x) ? 0u : x;
    };
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const uint32_t k = elem(i) & 0x7fffffffu;
        m = k > m ? k : m;
    }
    s = mx_sr_scale_byte<FMT>(m);
    f32x16 a, b;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        a[j] = __uint_as_float(mx_sr_round<FMT>(elem(2 * j), s, mx_sr_threshold(keys, 2 * j)));
        b[j] = __uint_as_float(mx_sr_round<FMT>(elem(2 * j + 1), s, mx_sr_threshold(keys, 2 * j + 1)));
    }
    if constexpr (FMT == MX_FP6_E2M3) c = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, mx_scale_operand(127u));
    else c = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, mx_scale_operand(127u));
}

// the block's 32 values in order, as float32
template <int FMT>
__device__ __forceinline__ f32x32 mx6_decode_f32(const u32x6& c, float scale) {
    if constexpr (FMT == MX_FP6_E2M3) return __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(c, scale);
    else return __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(c, scale);
}

// the same as 16 bfloat16 pairs (every value is a bfloat16 number: nothing is rounded)
template <int FMT>
__device__ __forceinline__ u32x16 mx6_decode_bf16(const u32x6& c, float scale) {
    if constexpr (FMT == MX_FP6_E2M3) return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, scale));
    else return __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_bf6(c, scale));
}

template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_fp6_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks) {
    constexpr int EPV = InVec<DT_IN>::EPV, NV = kMx6TileElems / (64 * EPV), N = kMx6Words<DT_IN>;
    using S = Mx6Slice<N * 4>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[WAVES][S::BYTES];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t e0 = tile * kMx6TileElems;
    if (e0 >= numel) return;
    const bool full = e0 + kMx6TileElems <= numel;                  // wave-uniform
    uint8_t* stage = s_stage[wave];

    u32x4 raw[NV];
    grouped_load<DT_IN, NV>(in, numel, e0 / EPV, lane, full, raw);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        const int v = r * 64 + lane;
        if constexpr (DT_IN == DT_F32) {
            uint8_t* dst = stage + (v >> 3) * S::STRIDE + (v & 7) * 8;
            *reinterpret_cast<u32x2*>(dst) = u32x2 {raw[r][0], raw[r][2]};
            *reinterpret_cast<u32x2*>(dst + 64) = u32x2 {raw[r][1], raw[r][3]};
        } else {
            *reinterpret_cast<u32x4*>(stage + (v >> 2) * S::STRIDE + (v & 3) * 16) = raw[r];
        }
    }
    wave_lds_sync();

    uint32_t w[N];
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        const u32x4 t = *reinterpret_cast<const u32x4*>(stage + lane * S::STRIDE + k * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[4 * k + e] = t[e];
    }
    uint32_t s;
    u32x6 c;
    mx6_encode<FMT, DT_IN>(w, s, c);
    wave_lds_sync();                                                // every lane has read its block: the slice is free for the codes

#pragma unroll
    for (int k = 0; k < 3; ++k) reinterpret_cast<u32x2*>(stage + lane * kMx6BlockBytes)[k] = u32x2 {c[2 * k], c[2 * k + 1]};
    stage[S::SCALES_AT + lane] = static_cast<uint8_t>(s);
    wave_lds_sync();

    uint8_t* o = codes + tile * kMx6TileBytes;
    uint8_t* osc = scales + tile * 64;
    if (full) {
        st<ST_WT>(reinterpret_cast<u32x4*>(o) + lane, reinterpret_cast<const u32x4*>(stage)[lane]);
        if (lane < 32) st<ST_WT>(reinterpret_cast<u32x4*>(o) + 64 + lane, reinterpret_cast<const u32x4*>(stage)[64 + lane]);
        if (lane < 4) st<ST_WT>(reinterpret_cast<u32x4*>(osc) + lane, reinterpret_cast<const u32x4*>(stage + S::SCALES_AT)[lane]);
    } else {
        const int64_t left = (numel * 6 + 7) / 8 - tile * kMx6TileBytes;   // code bytes of the tensor from the tile's first on (<= 1536)
        for (int b = lane; b < left && b < kMx6TileBytes; b += 64) o[b] = stage[b];
        if (tile * 64 + lane < nblocks) osc[lane] = stage[S::SCALES_AT + lane];
    }
}

// Guarded form for buffers that are not 16-byte aligned: a thread per block, element loads and byte stores, through mx6_encode -- the same bytes.
template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_fp6_guarded_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; b < nblocks; b += stride) {
        const int64_t i0 = b * kMxBlock;
        const int n = numel - i0 < kMxBlock ? static_cast<int>(numel - i0) : kMxBlock;
        uint32_t w[kMx6Words<DT_IN>];
#pragma unroll
        for (int j = 0; j < 16; ++j) {                              // elements at or past numel: quiet NaNs, as grouped_load has them
            if constexpr (DT_IN == DT_F32) {
                w[j] = 2 * j < n ? static_cast<const uint32_t*>(in)[i0 + 2 * j] : 0x7fc00000u;
                w[16 + j] = 2 * j + 1 < n ? static_cast<const uint32_t*>(in)[i0 + 2 * j + 1] : 0x7fc00000u;
            } else {
                const uint32_t lo = 2 * j < n ? static_cast<const uint16_t*>(in)[i0 + 2 * j] : 0x7fc0u;
                const uint32_t hi = 2 * j + 1 < n ? static_cast<const uint16_t*>(in)[i0 + 2 * j + 1] : 0x7fc0u;
                w[j] = lo | (hi << 16);
            }
        }
        uint32_t s;
        u32x6 c;
        mx6_encode<FMT, DT_IN>(w, s, c);
        scales[b] = static_cast<uint8_t>(s);
        const int nbytes = (n * 6 + 7) / 8;
#pragma unroll
        for (int k = 0; k < kMx6BlockBytes; ++k)
            if (k < nbytes) codes[b * kMx6BlockBytes + k] = static_cast<uint8_t>(c[k >> 2] >> ((k & 3) * 8));
    }
}

// The same tile with stochastic rounding: element i of the tensor at the global index index_base + i (seed and base by value: capturable).
template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_fp6_sr_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks,
                          uint64_t seed, uint64_t index_base) {
    constexpr int EPV = InVec<DT_IN>::EPV, NV = kMx6TileElems / (64 * EPV), N = kMx6Words<DT_IN>;
    using S = Mx6Slice<N * 4>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[WAVES][S::BYTES];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t e0 = tile * kMx6TileElems;
    if (e0 >= numel) return;
    const bool full = e0 + kMx6TileElems <= numel;                  // wave-uniform
    uint8_t* stage = s_stage[wave];

    u32x4 raw[NV];
    grouped_load<DT_IN, NV>(in, numel, e0 / EPV, lane, full, raw);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        const int v = r * 64 + lane;
        if constexpr (DT_IN == DT_F32) {
            uint8_t* dst = stage + (v >> 3) * S::STRIDE + (v & 7) * 8;
            *reinterpret_cast<u32x2*>(dst) = u32x2 {raw[r][0], raw[r][2]};
            *reinterpret_cast<u32x2*>(dst + 64) = u32x2 {raw[r][1], raw[r][3]};
        } else {
            *reinterpret_cast<u32x4*>(stage + (v >> 2) * S::STRIDE + (v & 3) * 16) = raw[r];
        }
    }
    wave_lds_sync();

    uint32_t w[N];
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        const u32x4 t = *reinterpret_cast<const u32x4*>(stage + lane * S::STRIDE + k * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[4 * k + e] = t[e];
    }
    uint32_t s;
    u32x6 c;
    mx6_encode_sr<FMT, DT_IN>(w, mx_sr_keys(seed, index_base + static_cast<uint64_t>(e0 + lane * kMxBlock)), s, c);
    wave_lds_sync();                                                // every lane has read its block: the slice is free for the codes

#pragma unroll
    for (int k = 0; k < 3; ++k) reinterpret_cast<u32x2*>(stage + lane * kMx6BlockBytes)[k] = u32x2 {c[2 * k], c[2 * k + 1]};
    stage[S::SCALES_AT + lane] = static_cast<uint8_t>(s);
    wave_lds_sync();

    uint8_t* o = codes + tile * kMx6TileBytes;
    uint8_t* osc = scales + tile * 64;
    if (full) {
        st<ST_WT>(reinterpret_cast<u32x4*>(o) + lane, reinterpret_cast<const u32x4*>(stage)[lane]);
        if (lane < 32) st<ST_WT>(reinterpret_cast<u32x4*>(o) + 64 + lane, reinterpret_cast<const u32x4*>(stage)[64 + lane]);
        if (lane < 4) st<ST_WT>(reinterpret_cast<u32x4*>(osc) + lane, reinterpret_cast<const u32x4*>(stage + S::SCALES_AT)[lane]);
    } else {
        const int64_t left = (numel * 6 + 7) / 8 - tile * kMx6TileBytes;   // code bytes of the tensor from the tile's first on (<= 1536)
        for (int b = lane; b < left && b < kMx6TileBytes; b += 64) o[b] = stage[b];
        if (tile * 64 + lane < nblocks) osc[lane] = stage[S::SCALES_AT + lane];
    }
}

// Its guarded form: the same loop through mx6_encode_sr.
template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_fp6_sr_guarded_kernel(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks,
                                  uint64_t seed, uint64_t index_base) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; b < nblocks; b += stride) {
        const int64_t i0 = b * kMxBlock;
        const int n = numel - i0 < kMxBlock ? static_cast<int>(numel - i0) : kMxBlock;
        uint32_t w[kMx6Words<DT_IN>];
#pragma unroll
        for (int j = 0; j < 16; ++j) {                              // elements at or past numel: quiet NaNs, as grouped_load has them
            if constexpr (DT_IN == DT_F32) {
                w[j] = 2 * j < n ? static_cast<const uint32_t*>(in)[i0 + 2 * j] : 0x7fc00000u;
                w[16 + j] = 2 * j + 1 < n ? static_cast<const uint32_t*>(in)[i0 + 2 * j + 1] : 0x7fc00000u;
            } else {
                const uint32_t lo = 2 * j < n ? static_cast<const uint16_t*>(in)[i0 + 2 * j] : 0x7fc0u;
                const uint32_t hi = 2 * j + 1 < n ? static_cast<const uint16_t*>(in)[i0 + 2 * j + 1] : 0x7fc0u;
                w[j] = lo | (hi << 16);
            }
        }
        uint32_t s;
        u32x6 c;
        mx6_encode_sr<FMT, DT_IN>(w, mx_sr_keys(seed, index_base + static_cast<uint64_t>(i0)), s, c);
        scales[b] = static_cast<uint8_t>(s);
        const int nbytes = (n * 6 + 7) / 8;
#pragma unroll
        for (int k = 0; k < kMx6BlockBytes; ++k)
            if (k < nbytes) codes[b * kMx6BlockBytes + k] = static_cast<uint8_t>(c[k >> 2] >> ((k & 3) * 8));
    }
}

// What the dequantize stages per block: float32 values, except for a bfloat16 SET (the conversion's own bfloat16 pairs).
template <int DT_OUT, int OP>
constexpr bool kMx6StageF32 = DT_OUT == DT_F32 || OP == OP_ADD;

template <int FMT, int DT_OUT, int OP>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_mx_fp6_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, void* __restrict__ out, int64_t numel, int64_t nblocks) {
    constexpr bool F32 = kMx6StageF32<DT_OUT, OP>;
    using S = Mx6Slice<F32 ? 128 : 64>;
    constexpr int EPV = DT_OUT == DT_F32 ? 4 : 8, NV = kMx6TileElems / (64 * EPV);
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[WAVES][S::BYTES];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t e0 = tile * kMx6TileElems;
    if (e0 >= numel) return;
    const bool full = e0 + kMx6TileElems <= numel;                  // wave-uniform
    const int64_t b0 = tile * kMx6TileBytes, nbytes = (numel * 6 + 7) / 8;
    uint8_t* stage = s_stage[wave];

    u32x4 old[NV];
    if constexpr (OP == OP_ADD) grouped_load<DT_OUT, NV>(out, numel, e0 / EPV, lane, full, old);

    u32x4 raw[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t off = b0 + (k * 64 + lane) * 16;
        raw[k] = u32x4 {0u, 0u, 0u, 0u};
        if (k == 1 && lane >= 32) continue;                         // 96 vectors a tile
        if (full) {
            raw[k] = ld<true>(reinterpret_cast<const u32x4*>(codes + off));
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (off + j < nbytes) raw[k][j >> 2] |= static_cast<uint32_t>(codes[off + j]) << ((j & 3) * 8);
        }
    }
    const uint32_t sb = tile * 64 + lane < nblocks ? scales[tile * 64 + lane] : 0u;
    reinterpret_cast<u32x4*>(stage)[lane] = raw[0];
    if (lane < 32) reinterpret_cast<u32x4*>(stage)[64 + lane] = raw[1];
    wave_lds_sync();

    u32x6 c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u32x2 t = reinterpret_cast<const u32x2*>(stage + lane * kMx6BlockBytes)[k];
        c[2 * k] = t[0];
        c[2 * k + 1] = t[1];
    }
    wave_lds_sync();                                                // every lane has read its codes: the slice is free for the values

    const float scale = mx_scale_operand(sb);
    if constexpr (F32) {
        const f32x32 f = mx6_decode_f32<FMT>(c, scale);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            *reinterpret_cast<u32x4*>(stage + lane * S::STRIDE + k * 16) =
                u32x4 {__float_as_uint(f[4 * k]), __float_as_uint(f[4 * k + 1]), __float_as_uint(f[4 * k + 2]), __float_as_uint(f[4 * k + 3])};
    } else {
        const u32x16 p = mx6_decode_bf16<FMT>(c, scale);
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x4*>(stage + lane * S::STRIDE + k * 16) = u32x4 {p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]};
    }
    wave_lds_sync();

    u32x4* out16 = reinterpret_cast<u32x4*>(static_cast<uint8_t*>(out) + e0 * (DT_OUT == DT_F32 ? 4 : 2));
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        const int v = r * 64 + lane;                                // output vector of the tile
        const int ce = v * EPV;                                     // its first element, relative to e0
        if (!full && e0 + ce >= numel) continue;
        u32x4 res;
        if constexpr (DT_OUT == DT_F32) {
            res = *reinterpret_cast<const u32x4*>(stage + (v >> 3) * S::STRIDE + (v & 7) * 16);
            if constexpr (OP == OP_ADD) {
#pragma unroll
                for (int e = 0; e < 4; ++e) res[e] = __float_as_uint(__fadd_rn(__uint_as_float(res[e]), __uint_as_float(old[r][e])));
            }
        } else if constexpr (OP == OP_SET) {
            res = *reinterpret_cast<const u32x4*>(stage + (v >> 2) * S::STRIDE + (v & 3) * 16);
        } else {
            const uint8_t* src = stage + (v >> 2) * S::STRIDE + (v & 3) * 32;
            const u32x4 lo = *reinterpret_cast<const u32x4*>(src), hi = *reinterpret_cast<const u32x4*>(src + 16);
            const uint32_t f[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                res[e] = f32x2_to_bf16x2_bits(__fadd_rn(__uint_as_float(f[2 * e]), __uint_as_float(old[r][e] << 16)),
                                              __fadd_rn(__uint_as_float(f[2 * e + 1]), __uint_as_float(old[r][e] & 0xffff0000u)));
        }
        if (full || e0 + ce + EPV <= numel) {
            st<ST_WT>(out16 + v, res);
        } else {                                                    // the tensor ends inside this vector
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                if (e0 + ce + e >= numel) continue;
                if constexpr (DT_OUT == DT_F32) static_cast<uint32_t*>(out)[e0 + ce + e] = res[e];
                else static_cast<uint16_t*>(out)[e0 + ce + e] = static_cast<uint16_t>(res[e >> 1] >> ((e & 1) * 16));
            }
        }
    }
}

// Guarded form for buffers that are not 16-byte aligned: a thread per block, byte loads and element stores, through the same conversions.
template <int FMT, int DT_OUT, int OP>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_mx_fp6_guarded_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, void* __restrict__ out, int64_t numel,
                                 int64_t nblocks) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; b < nblocks; b += stride) {
        const int64_t i0 = b * kMxBlock;
        const int n = numel - i0 < kMxBlock ? static_cast<int>(numel - i0) : kMxBlock;
        const int nbytes = (n * 6 + 7) / 8;
        u32x6 c {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kMx6BlockBytes; ++k)
            if (k < nbytes) c[k >> 2] |= static_cast<uint32_t>(codes[b * kMx6BlockBytes + k]) << ((k & 3) * 8);
        const float scale = mx_scale_operand(scales[b]);
        if constexpr (kMx6StageF32<DT_OUT, OP>) {
            const f32x32 f = mx6_decode_f32<FMT>(c, scale);
#pragma unroll
            for (int j = 0; j < kMxBlock; ++j)
                if (j < n) mx_store_one<DT_OUT, OP>(out, i0 + j, f[j]);
        } else {
            const u32x16 p = mx6_decode_bf16<FMT>(c, scale);
#pragma unroll
            for (int j = 0; j < kMxBlock; ++j)
                if (j < n) static_cast<uint16_t*>(out)[i0 + j] = static_cast<uint16_t>(p[j >> 1] >> ((j & 1) * 16));
        }
    }
}

}  // namespace pq
