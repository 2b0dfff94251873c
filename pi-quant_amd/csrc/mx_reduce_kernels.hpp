// The MX wire's kernels: what makes a quantized collective over MX records a handful of launches (include/piquant_hip.h has the definitions).
//   reduce_quantize_mx_kernel   (codes, scales) = quantize_mx(acc + sum_i dequantize_mx(term_i)): every ring hop and the mesh owner's step
//   dequantize_sum_mx_kernel    out (op)= sum_i dequantize_mx(term_i): the reduce-scatter owner's step
//   quantize_mx_batch_kernel / dequantize_mx_batch_kernel   the single kernels' tiles (mx_kernels.hpp) over up to 16 tensors
// Each is ONE streaming launch: no scan, no atomics, no grid or block barrier, no scratch; the waves of a block never wait for one another
// (wave_lds_sync on the wave's own LDS slice is the only synchronisation).
//
// Fused reduce: MxQuantTile's geometry, so that the sum goes through mx_quantize_rows as it is.  A wave owns NV rows of 64 16-byte acc vectors; a
// tile's share of one term is CONTIGUOUS -- OUT_BYTES = 1024 or 2048 code bytes (one or two coalesced 16-byte nt loads per lane) and NB = 32 or 64
// scale bytes (one dword for the first 8 or 16 lanes).  A term is parked in the wave's LDS slice, every lane reads back the OB code bytes of its
// own vector of each row and its block's scale byte, decodes with v_cvt_scalef32_pk_f32_{fp4,fp8} (s << 23 as the scale operand: s = 0, s = 0xFF
// and NaN codes come out as the definition has them) and adds with __fadd_rn into the resident rows; a bfloat16 accumulator rounds each pair of
// sums to bfloat16 and widens it again, which is what makes the result the composition's (dequantize_mx ADD term by term, then quantize_mx).
// The term loop is pipelined over ONE slice: the loads of term t + 1 are issued as soon as term t is parked, in front of its decode, and wait in
// registers; a second slice would double the LDS of a block (4.3 -> 8.6 KiB for the widest tile) to save one wave_lds_sync per term, which costs
// nothing while the wave waits for the next term's bytes anyway.  The same slice then stages the output.
// A ragged last tile reads its missing acc elements as quiet NaNs and its missing term bytes as 0: the NaN survives the sum and encodes as in
// quantize_mx; the stores stop at the tensor's last code byte and last scale byte.
//
// Dequantize-sum: MxDequantTile's geometry -- 2 KiB of codes per wave and term, every lane ends with the codes of its own OV 16-byte output
// vectors.  The running sum of those vectors stays in registers over the term loop (64 VGPRs for FP4 -> float32, the widest): out is read once
// (ADD) or never (SET) and written once.  The first term of a bfloat16 SET is rounded once (the conversion to bfloat16 itself, as dequantize_mx SET
// does it), the next is added to the rounded value.
#pragma once

#include "mx_kernels.hpp"

namespace pq {

constexpr int kMxMaxTerms = 16;
struct MxTerms {
    const uint8_t* codes[kMxMaxTerms];
    const uint8_t* scales[kMxMaxTerms];
    int count;
};

// the kernels' term table from a launch's term[] and count (launch.hpp: MxReduceLaunch, MxDequantSumLaunch, MxReduceEfLaunch); host side
template <class Launch>
inline MxTerms mx_terms_of(const Launch& l, const char* what, int min_count) {
    static_assert(kMxMaxInputs == kMxMaxTerms, "host and device term limits");
    if (l.count < min_count || l.count > kMxMaxTerms) panic("%s: %d terms, %d to %d per launch", what, l.count, min_count, kMxMaxTerms);
    MxTerms terms {};
    for (int i = 0; i < l.count; ++i) {
        terms.codes[i] = static_cast<const uint8_t*>(l.term[i].codes);
        terms.scales[i] = l.term[i].scales;
    }
    terms.count = l.count;
    return terms;
}

template <int DT_ACC, int FMT>
using MxQuantRows = u32x4[MxQuantTile<DT_ACC, FMT>::NV];    // the resident rows of a fused reduce's tile
template <int FMT, int DT_OUT>
using MxSumRows = u32x4[MxDequantTile<FMT, DT_OUT>::OV];    // the running sum of a dequantize-sum's output vectors

// ---- fused reduce + quantize --------------------------------------------------------------------------------------------------------------------

// a full tile's share of one term, loaded a term ahead: N16 16-byte vectors of codes per lane and, for lane < NB / 4, four scale bytes
template <int DT_ACC, int FMT>
struct MxReduceTermLoad {
    using T = MxQuantTile<DT_ACC, FMT>;
    static constexpr int N16 = T::OUT_BYTES / 1024;
    u32x4 v[N16];
    uint32_t sc;

    __device__ __forceinline__ void load(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, int64_t tile, int lane) {
        const u32x4* c = reinterpret_cast<const u32x4*>(codes + tile * T::OUT_BYTES);
#pragma unroll
        for (int j = 0; j < N16; ++j) v[j] = ld<true>(c + j * 64 + lane);
        sc = 0u;
        if (lane < T::NB / 4) sc = ld<true>(reinterpret_cast<const uint32_t*>(scales + tile * T::NB) + lane);
    }

    __device__ __forceinline__ void park(uint8_t* stage, uint8_t* stage_scales, int lane) const {
#pragma unroll
        for (int j = 0; j < N16; ++j) reinterpret_cast<u32x4*>(stage)[j * 64 + lane] = v[j];
        if (lane < T::NB / 4) reinterpret_cast<uint32_t*>(stage_scales)[lane] = sc;
    }
};

// the tile the tensor ends in, straight from memory: byte loads up to the tensor's last code byte and last scale byte, zeros behind them
template <class T>
__device__ __forceinline__ void mx_park_term_partial(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, int64_t tile, int64_t bytes_left,
                                                     int64_t blocks_left, uint8_t* stage, uint8_t* stage_scales, int lane) {
    const uint8_t* c = codes + tile * T::OUT_BYTES;
    for (int b = lane; b < T::OUT_BYTES; b += 64) stage[b] = b < bytes_left ? c[b] : 0;
    if (lane < T::NB) stage_scales[lane] = lane < blocks_left ? scales[tile * T::NB + lane] : 0;
}

// raw[r] = rn(raw[r] + the parked term's values of the lane's vector of row r), in the accumulator's type: the arithmetic of dequantize_mx ADD
template <int DT_ACC, int FMT>
__device__ __forceinline__ void mx_add_term(MxQuantRows<DT_ACC, FMT>& raw, const uint8_t* stage, const uint8_t* stage_scales, int lane) {
    using T = MxQuantTile<DT_ACC, FMT>;
    constexpr int EPV = T::EPV, OB = T::OB, NV = T::NV;
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        const float scale = mx_scale_operand(stage_scales[r * T::BPR + lane / T::LPB]);
        uint32_t w[OB > 4 ? 2 : 1];
        staged_words<OB>(stage + (r * 64 + lane) * OB, w);
        mx_static_for<0, EPV / 2>([&](auto j) {
            constexpr int J = decltype(j)::value;
            const f32x2 p = mx_decode_pair<FMT, J>(w, scale);
            if constexpr (DT_ACC == DT_F32) {
                raw[r][2 * J] = __float_as_uint(__fadd_rn(p[0], __uint_as_float(raw[r][2 * J])));
                raw[r][2 * J + 1] = __float_as_uint(__fadd_rn(p[1], __uint_as_float(raw[r][2 * J + 1])));
            } else {
                raw[r][J] = f32x2_to_bf16x2_bits(__fadd_rn(p[0], __uint_as_float(raw[r][J] << 16)), __fadd_rn(p[1], __uint_as_float(raw[r][J] & 0xffff0000u)));
            }
        });
    }
}

template <int DT_ACC, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_mx_kernel(const void* __restrict__ acc, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks, MxTerms terms) {
    using T = MxQuantTile<DT_ACC, FMT>;
    using L = MxReduceTermLoad<DT_ACC, FMT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::OUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t e0 = tile * T::TILE_ELEMS;
    if (e0 >= numel) return;
    const bool full = e0 + T::TILE_ELEMS <= numel;                  // wave-uniform
    uint8_t* stage = s_codes[wave];
    uint8_t* stage_scales = s_scales[wave];

    u32x4 raw[T::NV];
    L next;
    if (full && terms.count > 0) next.load(terms.codes[0], terms.scales[0], tile, lane);
    grouped_load<DT_ACC, T::NV>(acc, numel, e0 / T::EPV, lane, full, raw);
    for (int i = 0; i < terms.count; ++i) {
        if (full) {
            const L cur = next;
            cur.park(stage, stage_scales, lane);
            if (i + 1 < terms.count) next.load(terms.codes[i + 1], terms.scales[i + 1], tile, lane);   // in flight under this term's decode
        } else {
            mx_park_term_partial<T>(terms.codes[i], terms.scales[i], tile, (numel * T::BITS + 7) / 8 - tile * T::OUT_BYTES, nblocks - tile * T::NB, stage,
                                    stage_scales, lane);
        }
        wave_lds_sync();
        mx_add_term<DT_ACC, FMT>(raw, stage, stage_scales, lane);
        wave_lds_sync();                                            // every lane has read the term: the slice is free for the next one, or for the output
    }
    mx_quantize_rows<DT_ACC, FMT>(raw, codes, scales, numel, nblocks, tile, full, lane, stage, stage_scales);
}

// element i of term t as float32: the guarded kernels' decode (dequantize_mx_guarded_kernel's)
template <int FMT>
__device__ __forceinline__ float mx_term_value(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, int64_t i) {
    uint32_t w[1];
    if constexpr (FMT == MX_FP4_E2M1) w[0] = (codes[i >> 1] >> ((i & 1) * 4)) & 0xfu;
    else w[0] = codes[i];
    return mx_decode_pair<FMT, 0>(w, mx_scale_operand(scales[i / kMxBlock]))[0];
}

// element i of acc + the terms, added in order and rounded to the accumulator's type after each, as float32 bits
template <int DT_ACC, int FMT>
__device__ __forceinline__ uint32_t mx_guarded_sum(const void* __restrict__ acc, const MxTerms& terms, int64_t i) {
    uint32_t x = mx_load_bits<DT_ACC>(acc, i);
    for (int t = 0; t < terms.count; ++t) {
        const float s = __fadd_rn(mx_term_value<FMT>(terms.codes[t], terms.scales[t], i), __uint_as_float(x));
        if constexpr (DT_ACC == DT_F32) x = __float_as_uint(s);
        else x = f32_to_bf16_bits(s) << 16;
    }
    return x;
}

// Guarded form for buffers that are not 16-byte aligned: a thread per block, element by element, through the same steps -- the same bytes.  The sum
// is formed twice (for the block's maximum, then for the codes) instead of being kept: 32 live sums a thread would spill.
template <int DT_ACC, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_mx_guarded_kernel(const void* __restrict__ acc, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks,
                                  MxTerms terms) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; b < nblocks; b += stride) {
        const int64_t i0 = b * kMxBlock;
        const int n = numel - i0 < kMxBlock ? static_cast<int>(numel - i0) : kMxBlock;
        uint32_t key = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t k = mx_abs_key(mx_guarded_sum<DT_ACC, FMT>(acc, terms, i0 + j));
            key = k > key ? k : key;
        }
        const uint32_t s = mx_scale_byte<FMT>(key);
        scales[b] = static_cast<uint8_t>(s);
        for (int j = 0; j < n; j += 4) {
            uint32_t x[4], w[1];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = j + e < n ? mx_guarded_sum<DT_ACC, FMT>(acc, terms, i0 + j + e) : 0u;
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

// ---- dequantize-sum -----------------------------------------------------------------------------------------------------------------------------

// a full tile's share of one term, loaded a term ahead: two 16-byte vectors of codes per lane and, for lane < NB / 4, four scale bytes
template <int FMT, int DT_OUT>
struct MxSumTermLoad {
    using T = MxDequantTile<FMT, DT_OUT>;
    u32x4 v[T::NIN];
    uint32_t sc;

    __device__ __forceinline__ void load(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, int64_t tile, int lane) {
        const u32x4* c = reinterpret_cast<const u32x4*>(codes + tile * T::TILE_BYTES);
#pragma unroll
        for (int k = 0; k < T::NIN; ++k) v[k] = ld<true>(c + k * 64 + lane);
        sc = 0u;
        if (lane < T::NB / 4) sc = ld<true>(reinterpret_cast<const uint32_t*>(scales + tile * T::NB) + lane);
    }

    __device__ __forceinline__ void park(uint8_t* stage, uint8_t* stage_scales, int lane) const {
#pragma unroll
        for (int k = 0; k < T::NIN; ++k) reinterpret_cast<u32x4*>(stage)[k * 64 + lane] = v[k];
        if (lane < T::NB / 4) reinterpret_cast<uint32_t*>(stage_scales)[lane] = sc;
    }
};

// sum[k] (one 16-byte output vector: float32 bits, or bfloat16 pairs) takes the parked term's values of the lane's vector k: stored (SET: the first
// term of a SET, bfloat16 rounded by the conversion itself) or added and rounded to the output type.  A ragged tile's vectors past the tensor's end
// hold whatever the zero fill decodes to and are never stored.
template <int FMT, int DT_OUT, bool SET>
__device__ __forceinline__ void mx_sum_term(MxSumRows<FMT, DT_OUT>& sum, const uint8_t* stage, const uint8_t* stage_scales, int lane) {
    using T = MxDequantTile<FMT, DT_OUT>;
    constexpr int EPV = T::EPV, IB = T::IB, WORDS = IB > 4 ? 2 : 1;
#pragma unroll
    for (int k = 0; k < T::OV; ++k) {
        const int c = k * 64 + lane;
        const float scale = mx_scale_operand(stage_scales[c * EPV / kMxBlock]);
        uint32_t w[WORDS];
        staged_words<IB>(stage + c * IB, w);
        mx_static_for<0, EPV / 2>([&](auto j) {
            constexpr int J = decltype(j)::value;
            if constexpr (DT_OUT == DT_BF16 && SET) {
                sum[k][J] = mx_decode_pair_bf16<FMT, J>(w, scale);
            } else {
                const f32x2 p = mx_decode_pair<FMT, J>(w, scale);
                if constexpr (DT_OUT == DT_F32) {
                    sum[k][2 * J] = __float_as_uint(SET ? p[0] : __fadd_rn(p[0], __uint_as_float(sum[k][2 * J])));
                    sum[k][2 * J + 1] = __float_as_uint(SET ? p[1] : __fadd_rn(p[1], __uint_as_float(sum[k][2 * J + 1])));
                } else {
                    sum[k][J] = f32x2_to_bf16x2_bits(__fadd_rn(p[0], __uint_as_float(sum[k][J] << 16)), __fadd_rn(p[1], __uint_as_float(sum[k][J] & 0xffff0000u)));
                }
            }
        });
    }
}

template <int FMT, int DT_OUT, int OP>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_sum_mx_kernel(void* __restrict__ out, int64_t numel, int64_t nblocks, MxTerms terms) {
    using T = MxDequantTile<FMT, DT_OUT>;
    using L = MxSumTermLoad<FMT, DT_OUT>;
    constexpr int EPV = T::EPV, OV = T::OV, NB = T::NB, ESIZE = DT_OUT == DT_F32 ? 4 : 2, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::TILE_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t e0 = tile * T::TILE_ELEMS;
    if (e0 >= numel) return;
    const bool full = e0 + T::TILE_ELEMS <= numel;                  // wave-uniform
    uint8_t* stage = s_codes[wave];
    uint8_t* stage_scales = s_scales[wave];
    const int64_t bytes_left = (numel * T::BITS + 7) / 8 - tile * T::TILE_BYTES, blocks_left = nblocks - tile * NB;

    L next;
    if (full) next.load(terms.codes[0], terms.scales[0], tile, lane);
    u32x4* out16 = reinterpret_cast<u32x4*>(static_cast<uint8_t*>(out) + e0 * ESIZE);
    u32x4 sum[OV];
    if constexpr (OP == OP_ADD) {                                   // out, once; a vector the tensor ends in element by element, zeros behind the end
#pragma unroll
        for (int k = 0; k < OV; ++k) {
            const int64_t i = e0 + static_cast<int64_t>(k * 64 + lane) * EPV;
            if (full || i + EPV <= numel) {
                sum[k] = ld<true>(out16 + k * 64 + lane);
            } else {
                sum[k] = u32x4 {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < EPV; ++e) {
                    if (i + e >= numel) continue;
                    if constexpr (DT_OUT == DT_F32) sum[k][e] = static_cast<const uint32_t*>(out)[i + e];
                    else sum[k][e >> 1] |= static_cast<uint32_t>(static_cast<const uint16_t*>(out)[i + e]) << ((e & 1) * 16);
                }
            }
        }
    }
    for (int i = 0; i < terms.count; ++i) {
        if (full) {
            const L cur = next;
            cur.park(stage, stage_scales, lane);
            if (i + 1 < terms.count) next.load(terms.codes[i + 1], terms.scales[i + 1], tile, lane);   // in flight under this term's decode
        } else {
            const uint8_t* c = terms.codes[i] + tile * T::TILE_BYTES;
            for (int b = lane; b < T::TILE_BYTES; b += 64) stage[b] = b < bytes_left ? c[b] : 0;
            for (int b = lane; b < NB; b += 64) stage_scales[b] = b < blocks_left ? terms.scales[i][tile * NB + b] : 0;
        }
        wave_lds_sync();
        if (OP == OP_SET && i == 0) mx_sum_term<FMT, DT_OUT, true>(sum, stage, stage_scales, lane);
        else mx_sum_term<FMT, DT_OUT, false>(sum, stage, stage_scales, lane);
        wave_lds_sync();                                            // every lane has read the term: the slice is free for the next one
    }
#pragma unroll
    for (int k = 0; k < OV; ++k) {
        const int64_t i = e0 + static_cast<int64_t>(k * 64 + lane) * EPV;
        if (full || i + EPV <= numel) {
            st<ST_WT>(out16 + k * 64 + lane, sum[k]);
        } else {
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                if (i + e >= numel) continue;
                if constexpr (DT_OUT == DT_F32) static_cast<uint32_t*>(out)[i + e] = sum[k][e];
                else static_cast<uint16_t*>(out)[i + e] = static_cast<uint16_t>(sum[k][e >> 1] >> ((e & 1) * 16));
            }
        }
    }
}

// ---- batches: the single kernels' tiles over up to kMxBatchMax tensors ---------------------------------------------------------------------------
// Tensor t owns the waves [chunk_begin[t], chunk_begin[t + 1]) of the grid (a chunk is one tile); the host fills the prefix table and every wave
// finds its tensor by a wave-uniform search of at most 15 compares (grouped_batch_tensor).  Member t's bytes are those of the single kernel on it.
constexpr int kMxBatchMax = 16;
struct MxQuantBatchArgs {
    const void* in[kMxBatchMax];
    uint8_t* codes[kMxBatchMax];
    uint8_t* scales[kMxBatchMax];
    int64_t numel[kMxBatchMax];
    int64_t chunk_begin[kMxBatchMax + 1];
    int count;
};
struct MxDequantBatchArgs {
    const uint8_t* codes[kMxBatchMax];
    const uint8_t* scales[kMxBatchMax];
    void* out[kMxBatchMax];
    int64_t numel[kMxBatchMax];
    int64_t chunk_begin[kMxBatchMax + 1];
    int count;
};

template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_batch_kernel(MxQuantBatchArgs a) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::OUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    mx_quantize_tile<DT_IN, FMT>(a.in[t], a.codes[t], a.scales[t], numel, (numel + kMxBlock - 1) / kMxBlock, c - a.chunk_begin[t], lane, s_codes[wave],
                                 s_scales[wave]);
}

// The batch with stochastic rounding: one seed, member t's elements at the global indices index_base[t] + i -- the bytes of quantize_mx_sr_kernel on it.
struct MxSrBatchArgs {
    uint64_t seed;
    uint64_t index_base[kMxBatchMax];
};

template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_sr_batch_kernel(MxQuantBatchArgs a, MxSrBatchArgs sr) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::OUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    mx_quantize_tile<DT_IN, FMT, MX_SR>(a.in[t], a.codes[t], a.scales[t], numel, (numel + kMxBlock - 1) / kMxBlock, c - a.chunk_begin[t], lane, s_codes[wave],
                                        s_scales[wave], sr.seed, sr.index_base[t]);
}

template <int FMT, int DT_OUT, int OP>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_mx_batch_kernel(MxDequantBatchArgs a) {
    using T = MxDequantTile<FMT, DT_OUT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::TILE_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    mx_dequantize_tile<FMT, DT_OUT, OP>(a.codes[t], a.scales[t], a.out[t], numel, (numel + kMxBlock - 1) / kMxBlock, c - a.chunk_begin[t], lane, s_codes[wave],
                                        s_scales[wave]);
}

}  // namespace pq
