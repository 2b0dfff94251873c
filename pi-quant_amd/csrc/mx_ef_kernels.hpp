// Error feedback on the MX wire (include/piquant_hip.h, piquant_hip_quantize_mx_ef): y = rn_f32(widen(x) + R), (codes, scales) = quantize_mx(y),
// R <- rn_f32(y - dequantize_mx(codes, scales)), in ONE streaming launch -- no scan, no atomics, no grid or block barrier, no scratch.  The residual
// R is float32 whatever the tensor's type, and so is y: a bfloat16 tensor is only ever widened.
//
// Geometry: MxQuantTile's, per input type.  A wave owns NV rows of 64 16-byte x vectors; a block is 8 lanes of a float32 row or 4 of a bfloat16 row,
// so mx_block_max's DPP steps and the staging of codes and scale bytes (mx_quantize_row, mx_store_staged) are the plain quantize's.  A lane-row is
// EPV = 4 or 8 elements, which are RV = 1 or 2 16-byte vectors of the residual: a bfloat16 lane loads and stores the two vectors of its own eight
// elements (32 contiguous bytes; the two instructions of a row cover the same 2 KiB of the residual, each every other 16 bytes).  The other form --
// the float32 tile over 8-byte x loads -- would keep one residual vector a lane, but the fused reduce must round its running sum to bfloat16 after
// every term, pair by pair, on the packed rows that MxReduceTermLoad and mx_add_term work on: this form takes both as they are.
// Every x load and every residual load of the tile (nt, 16 bytes) is issued before the first use.
// Per row: y = x + R (__fadd_rn); integer amax on y's bits, scale byte, mx_encode (mx_quantize_row); the codes, STILL IN REGISTERS, decoded with
// mx_decode_pair under the same scale operand -- the decode agrees with the definition for every code under every scale byte (the
// probe table), so the value is dequantize_mx's without an LDS round trip or a second pass; R' = y - d with a __fsub_rn of its own (no contraction,
// no reassociation: the unit is built with -ffp-contract=off besides); R' leaves as 16-byte write-through stores.
// A ragged last tile reads its missing x elements as quiet NaNs (grouped_load) and its missing residual elements as 0: y is a NaN there, changes no
// amax, encodes to nibble 0 in FP4 and is never stored -- codes, scale bytes and residual stop at the tensor's end.
//
// Fused reduce (piquant_hip_reduce_quantize_mx_ef): reduce_quantize_mx_kernel's term loop (MxReduceTermLoad, mx_add_term: the sum rounded to the
// accumulator's type after each term) in front of the same rows body; the sum and the residual stay in registers, one launch for 0 .. 16 terms.
// Batch: the tile body behind grouped_batch_tensor's prefix search.  Guarded: a thread per block, element by element through the same mx_encode /
// mx_decode_pair -- the same bytes -- for buffers that are not 16-byte aligned; the single call is its count == 0.
#pragma once

#include "mx_reduce_kernels.hpp"

namespace pq {

// The two halves of mx_quantize_rows (mx_kernels.hpp), restated here because the codes must stay with the caller between them.  mx_quantize_rows
// itself is left whole: cut into these two, the bfloat16 instances of the plain kernels compiled to other schedules and register counts.

// The lane's vector of row r of a tile (x: its EPV elements as float32 bits) -> the block's scale byte, parked by the lane that starts the block
// and returned, and the lane's codes in w, parked at the vector's place of the wave's LDS slice.
template <int DT_IN, int FMT>
__device__ __forceinline__ uint32_t mx_quantize_row(const uint32_t (&x)[MxQuantTile<DT_IN, FMT>::EPV], int r, int lane, uint8_t* stage, uint8_t* stage_scales,
                                                    uint32_t (&w)[MxQuantTile<DT_IN, FMT>::OB > 4 ? 2 : 1]) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int EPV = T::EPV, OB = T::OB, LPB = T::LPB, BPR = T::BPR;
    uint32_t key = mx_abs_key(x[0]);
#pragma unroll
    for (int e = 1; e < EPV; ++e) {
        const uint32_t k = mx_abs_key(x[e]);
        key = k > key ? k : key;
    }
    const uint32_t s = mx_scale_byte<FMT>(mx_block_max<LPB>(key));
    if (lane % LPB == 0) stage_scales[r * BPR + lane / LPB] = static_cast<uint8_t>(s);
    mx_encode<FMT, EPV>(x, s, w);
    uint8_t* dst = stage + (r * 64 + lane) * OB;
    if constexpr (OB == 2) *reinterpret_cast<uint16_t*>(dst) = static_cast<uint16_t>(w[0]);
    else if constexpr (OB == 4) *reinterpret_cast<uint32_t*>(dst) = w[0];
    else *reinterpret_cast<u32x2*>(dst) = u32x2 {w[0], w[1]};
    return s;
}

// The tile's parked codes and scale bytes to memory: 16-byte-per-lane write-through stores, or byte by byte up to the tensor's last code byte and
// last scale byte in the tile the tensor ends in.
template <class T>
__device__ __forceinline__ void mx_store_staged(uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks, int64_t tile, bool full,
                                                int lane, const uint8_t* stage, const uint8_t* stage_scales) {
    constexpr int OB = T::OB, NV = T::NV, NB = T::NB;
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

// the residual of a tile's rows: RV 16-byte vectors per lane-row
template <int DT_IN, int FMT>
using MxEfResidualRows = u32x4[MxQuantTile<DT_IN, FMT>::NV][InVec<DT_IN>::EPV / 4];

// Load only (all issued before the first use); elements at or past numel read as 0 -- their x is a quiet NaN, so what they hold decides nothing.
template <int DT_IN, int FMT>
__device__ __forceinline__ void mx_ef_load_residual(const float* residual, int64_t numel, int64_t e0, int lane, bool full, MxEfResidualRows<DT_IN, FMT>& res) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int RV = T::EPV / 4;
    const u32x4* r16 = reinterpret_cast<const u32x4*>(residual);
#pragma unroll
    for (int r = 0; r < T::NV; ++r) {
#pragma unroll
        for (int k = 0; k < RV; ++k) {
            const int64_t vec = e0 / 4 + (r * 64 + lane) * RV + k;
            if (full || (vec + 1) * 4 <= numel) {
                res[r][k] = ld<true>(r16 + vec);
            } else {
                res[r][k] = u32x4 {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 4; ++e)   // unrolled: constant register indices
                    if (vec * 4 + e < numel) res[r][k][e] = reinterpret_cast<const uint32_t*>(residual)[vec * 4 + e];
            }
        }
    }
}

// The tile's rows in `raw` (x, or the fused reduce's sum, in the tensor's type) and their residual in `res` -> codes, scale bytes and the new
// residual.  The wave's LDS slices as in mx_quantize_rows.
template <int DT_IN, int FMT>
__device__ __forceinline__ void mx_ef_rows(const u32x4 (&raw)[MxQuantTile<DT_IN, FMT>::NV], const MxEfResidualRows<DT_IN, FMT>& res, float* residual,
                                           uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks, int64_t tile, bool full,
                                           int lane, uint8_t* stage, uint8_t* stage_scales) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int EPV = T::EPV, OB = T::OB, NV = T::NV, RV = EPV / 4;
    const int64_t v0 = tile * (T::TILE_ELEMS / 4);                  // the tile's first residual vector
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        uint32_t y[EPV];
        mx_unpack_bits<DT_IN>(raw[r], y);
#pragma unroll
        for (int e = 0; e < EPV; ++e) y[e] = __float_as_uint(__fadd_rn(__uint_as_float(y[e]), __uint_as_float(res[r][e / 4][e % 4])));
        uint32_t w[OB > 4 ? 2 : 1];
        const float scale = mx_scale_operand(mx_quantize_row<DT_IN, FMT>(y, r, lane, stage, stage_scales, w));
        u32x4 o[RV];
        mx_static_for<0, EPV / 2>([&](auto j) {
            constexpr int J = decltype(j)::value;
            const f32x2 d = mx_decode_pair<FMT, J>(w, scale);
            o[J / 2][(2 * J) % 4] = __float_as_uint(__fsub_rn(__uint_as_float(y[2 * J]), d[0]));
            o[J / 2][(2 * J) % 4 + 1] = __float_as_uint(__fsub_rn(__uint_as_float(y[2 * J + 1]), d[1]));
        });
#pragma unroll
        for (int k = 0; k < RV; ++k) grouped_store_vector<DT_F32>(residual, numel, v0 + (r * 64 + lane) * RV + k, full, o[k]);
    }
    mx_store_staged<T>(codes, scales, numel, nblocks, tile, full, lane, stage, stage_scales);
}

// one wave's tile of one (tensor, residual) pair (tile * TILE_ELEMS < numel)
template <int DT_IN, int FMT>
__device__ __forceinline__ void mx_ef_tile(const void* __restrict__ in, float* residual, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel,
                                           int64_t nblocks, int64_t tile, int lane, uint8_t* stage, uint8_t* stage_scales) {
    using T = MxQuantTile<DT_IN, FMT>;
    const int64_t e0 = tile * T::TILE_ELEMS;
    const bool full = e0 + T::TILE_ELEMS <= numel;                  // wave-uniform
    u32x4 raw[T::NV];
    MxEfResidualRows<DT_IN, FMT> res;
    grouped_load<DT_IN, T::NV>(in, numel, e0 / T::EPV, lane, full, raw);
    mx_ef_load_residual<DT_IN, FMT>(residual, numel, e0, lane, full, res);
    mx_ef_rows<DT_IN, FMT>(raw, res, residual, codes, scales, numel, nblocks, tile, full, lane, stage, stage_scales);
}

template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_ef_kernel(const void* __restrict__ in, float* residual, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel, int64_t nblocks) {
    using T = MxQuantTile<DT_IN, FMT>;
    constexpr int WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[WAVES][T::OUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_scales[WAVES][T::NB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    if (tile * T::TILE_ELEMS >= numel) return;
    mx_ef_tile<DT_IN, FMT>(in, residual, codes, scales, numel, nblocks, tile, lane, s_codes[wave], s_scales[wave]);
}

// Up to kMxBatchMax independent (tensor, residual) pairs in ONE launch, found through the prefix table of quantize_mx_batch_kernel.
struct MxEfBatchArgs {
    const void* in[kMxBatchMax];
    float* residual[kMxBatchMax];
    uint8_t* codes[kMxBatchMax];
    uint8_t* scales[kMxBatchMax];
    int64_t numel[kMxBatchMax];
    int64_t chunk_begin[kMxBatchMax + 1];
    int count;
};

template <int DT_IN, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_mx_ef_batch_kernel(MxEfBatchArgs a) {
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
    mx_ef_tile<DT_IN, FMT>(a.in[t], a.residual[t], a.codes[t], a.scales[t], numel, (numel + kMxBlock - 1) / kMxBlock, c - a.chunk_begin[t], lane, s_codes[wave],
                           s_scales[wave]);
}

// The fused reduce: the residual's loads go out with the accumulator's and the first term's, the term loop is reduce_quantize_mx_kernel's.
template <int DT_ACC, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_mx_ef_kernel(const void* __restrict__ acc, float* residual, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel,
                             int64_t nblocks, MxTerms terms) {
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
    MxEfResidualRows<DT_ACC, FMT> res;
    L next;
    if (full && terms.count > 0) next.load(terms.codes[0], terms.scales[0], tile, lane);
    grouped_load<DT_ACC, T::NV>(acc, numel, e0 / T::EPV, lane, full, raw);
    mx_ef_load_residual<DT_ACC, FMT>(residual, numel, e0, lane, full, res);
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
    mx_ef_rows<DT_ACC, FMT>(raw, res, residual, codes, scales, numel, nblocks, tile, full, lane, stage, stage_scales);
}

// Guarded form of the single call (terms.count == 0) and of the reduce, for buffers that are not 16-byte aligned: a thread per block, element by
// element, through the same steps -- the same bytes.  y is formed twice (for the block's maximum, then for the codes), as reduce_quantize_mx_guarded_kernel
// forms its sum: a block's residual is read twice and written once, by its own thread, each element behind its last read.
template <int DT_ACC, int FMT>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_mx_ef_guarded_kernel(const void* __restrict__ acc, float* residual, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t numel,
                                     int64_t nblocks, MxTerms terms) {
    auto y_of = [&](int64_t i) { return __float_as_uint(__fadd_rn(__uint_as_float(mx_guarded_sum<DT_ACC, FMT>(acc, terms, i)), residual[i])); };
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; b < nblocks; b += stride) {
        const int64_t i0 = b * kMxBlock;
        const int n = numel - i0 < kMxBlock ? static_cast<int>(numel - i0) : kMxBlock;
        uint32_t key = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t k = mx_abs_key(y_of(i0 + j));
            key = k > key ? k : key;
        }
        const uint32_t s = mx_scale_byte<FMT>(key);
        scales[b] = static_cast<uint8_t>(s);
        for (int j = 0; j < n; j += 4) {
            uint32_t y[4], w[1];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = j + e < n ? y_of(i0 + j + e) : 0u;
            mx_encode<FMT, 4>(y, s, w);
            const f32x2 d01 = mx_decode_pair<FMT, 0>(w, mx_scale_operand(s)), d23 = mx_decode_pair<FMT, 1>(w, mx_scale_operand(s));
            const float d[4] = {d01[0], d01[1], d23[0], d23[1]};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < n) residual[i0 + j + e] = __fsub_rn(__uint_as_float(y[e]), d[e]);
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

}  // namespace pq
