// Error feedback in the rotated domain (include/piquant_hip.h, piquant_hip_quantize_grouped_rotated_ef / piquant_hip_reduce_quantize_grouped_rotated_ef;
// DESIGN.md 4d).  The residual is a float32 record of ROTATED values: the rotation is orthogonal, linear and the same on every step for one seed,
// so what a step loses is fed to the next one without ever leaving the rotated domain -- one rotation a call, as in the kernels without a residual.
//   quantize   Y = the float32 forward rotation of the widened tensor; y = rn(Y + R); (q, scales, zero points) = quantize_grouped(y), computed
//              parameters; R <- rn(y - d), d the float32 SET dequantize of q.  Bit for bit quantize_grouped_ef(hadamard_grouped(widen(x)), R).
//   reduce     Y = rotate(widen(acc)) + d(term_0) + ... in order, one separately rounded float32 add per term; then as above: the residual is
//              added BEHIND the terms.  acc is only read.
// Both sit on the float32 row layout of GroupedQuantTile and are assembled from the helpers of grouped_rot_kernels.hpp (load, rotation, term loop)
// and of grouped_kernels.hpp (the chunk body with KEEP, the residual store).  The residual's rows are 16-byte loads issued in front of the
// butterflies -- memory work the VALU-bound rotation hides -- where a lane holds at most eight rows; the sixteen-row tiles (every uint2 tile,
// G = 4096) load them behind the butterflies instead, four rows at a time (grouped_rot_ef_add_batched): all sixteen in flight do not fit.  One launch each: no scan, no atomics, no
// grid barrier, no LDS memory traffic for the butterflies; waves never wait for one another.
#pragma once

#include "grouped_rot_kernels.hpp"

namespace pq {

// whether the residual's rows are in flight across the butterflies (NV rows a lane)
template <int NV>
struct GroupedRotEfEarly {
    static constexpr bool value = NV <= 8;
};

// one wave's chunk of a tensor of type DT on the float32 tile, loads only: float32 rows into raw, bfloat16 rows packed into t (widened later, so
// that the residual's loads can be issued behind these without a wait between them)
template <int DT, int NV>
__device__ __forceinline__ void grouped_rot_ef_load(const void* in, int64_t numel, int64_t v0, int lane, bool full, u32x4 (&raw)[NV], u32x2 (&t)[NV]) {
    if constexpr (DT == DT_F32) grouped_load<DT_F32, NV>(in, numel, v0, lane, full, raw);
    else grouped_load_bf16x4<NV>(in, numel, v0, lane, full, t);
}

// raw[r] = rn(raw[r] + R[r]) for the sixteen-row tiles: the residual's rows loaded and added B at a time, so that they never hold more than B rows
// of registers (elements at or past numel: quiet NaNs, as grouped_load reads them)
template <int NV, int B>
__device__ __forceinline__ void grouped_rot_ef_add_batched(u32x4 (&raw)[NV], const float* residual, int64_t numel, int64_t v0, int lane, bool full) {
    static_assert(NV % B == 0, "whole batches");
#pragma unroll
    for (int b0 = 0; b0 < NV; b0 += B) {
        u32x4 res[B];
        grouped_load<DT_F32, B>(residual, numel, v0 + b0 * 64, lane, full, res);
#pragma unroll
        for (int j = 0; j < B; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) raw[b0 + j][e] = __float_as_uint(__fadd_rn(__uint_as_float(raw[b0 + j][e]), __uint_as_float(res[j][e])));
        }
    }
}

constexpr int kGroupedRotEfBatchRows = 4;

// One wave's chunk (NG groups of the float32 tile from group g0 on) of one (tensor, residual) pair: the body of the single-tensor kernel and of the
// batch kernel; the wave's LDS slices as in grouped_quantize_chunk with KEEP.
template <int DT_IN, int BITS, int MODE, int G>
__device__ __forceinline__ void grouped_rot_ef_chunk(const void* __restrict__ in, float* residual, uint8_t* __restrict__ out, int64_t numel,
                                                     float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo,
                                                     uint32_t rot_hi, const QuantParams& p0, int64_t g0, int lane, uint8_t* stage, float* s_a, float* s_b,
                                                     float* s_c) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG;
    constexpr bool EARLY = GroupedRotEfEarly<NV>::value;
    const int64_t v0 = g0 * T::V;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform

    u32x4 raw[NV];
    [[maybe_unused]] u32x4 res[EARLY ? NV : 1];
    [[maybe_unused]] u32x2 t[NV];
    if constexpr (EARLY) {
        grouped_rot_ef_load<DT_IN, NV>(in, numel, v0, lane, full, raw, t);
        grouped_load<DT_F32, NV>(residual, numel, v0, lane, full, res);
        if constexpr (DT_IN != DT_F32) grouped_widen_bf16x4<NV>(t, raw);
    } else {
        grouped_rot_load<DT_IN, NV>(in, numel, v0, lane, full, raw, t);
    }
    grouped_rotate_chunk<BITS, G, false>(raw, numel, g0, full, lane, rot_lo, rot_hi);
    if constexpr (EARLY) grouped_add_residual<DT_F32, NV>(raw, res);
    else grouped_rot_ef_add_batched<NV, kGroupedRotEfBatchRows>(raw, residual, numel, v0, lane, full);
    grouped_quantize_chunk<DT_F32, BITS, MODE, G, false, NV, true>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a, s_b, s_c);
    grouped_residual_store<DT_F32, BITS, G>(raw, residual, numel, v0, full, lane, stage, s_c, s_b);
}

template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_rotated_ef_kernel(const void* __restrict__ in, float* residual, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                   uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi, QuantParams p0) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];   // {min, max}, then {1/scale, zero point, scale} of the chunk's groups

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    grouped_rot_ef_chunk<DT_IN, BITS, MODE, G>(in, residual, out, numel, scales, zero_points, ngroups, rot_lo, rot_hi, p0, g0, lane, s_out[wave], s_a[wave],
                                               s_b[wave], s_c[wave]);
}

// Batch: up to kGroupedBatchMax independent (tensor, residual) pairs in ONE launch, found through the prefix table of quantize_grouped_batch_kernel
// (unit: the chunk of the float32 tile, G * NG elements).  The residuals of the table are float32, whatever the tensors' type.
template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_rotated_ef_batch_kernel(GroupedEfBatchArgs a, uint32_t rot_lo, uint32_t rot_hi, QuantParams p0) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    grouped_rot_ef_chunk<DT_IN, BITS, MODE, G>(a.in[t], static_cast<float*>(a.residual[t]), a.out[t], numel, a.scales[t], a.zero_points[t],
                                               (numel + G - 1) / G, rot_lo, rot_hi, p0, (c - a.chunk_begin[t]) * NG, lane, s_out[wave], s_a[wave],
                                               s_b[wave], s_c[wave]);
}

// The term loop is reduce_quantize_grouped_rotated_kernel's: the first term's loads in front of the accumulator's, term i + 1 in flight while term
// i is added.
template <int DT_ACC, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_grouped_rotated_ef_kernel(const void* __restrict__ acc, float* residual, uint8_t* __restrict__ out, int64_t numel,
                                          float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi,
                                          QuantParams p0, GroupedTerms terms) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    using L = GroupedTermLoad<DT_F32, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64, PACK = 8 / BITS;
    constexpr bool EARLY = GroupedRotEfEarly<NV>::value;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];   // a term's {scale, bias}; then {min, max}, then {1/scale, zero point, scale}
    __shared__ int32_t s_z[WAVES][NG];                                 // a term's zero point

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    const int64_t v0 = g0 * T::V;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform
    const int64_t gj = g0 + lane;
    const bool has_group = lane < NG && gj < ngroups;
    uint8_t* stage = s_out[wave];
    const int count = terms.count;

    u32x4 raw[NV];
    [[maybe_unused]] u32x4 res[EARLY ? NV : 1];
    [[maybe_unused]] u32x2 t[NV];
    L next;
    if (full && count > 0) next.load(terms.in[0], terms.scales[0], terms.zero_points[0], v0, gj, has_group, lane);
    if constexpr (EARLY) {
        grouped_rot_ef_load<DT_ACC, NV>(acc, numel, v0, lane, full, raw, t);
        grouped_load<DT_F32, NV>(residual, numel, v0, lane, full, res);
        if constexpr (DT_ACC != DT_F32) grouped_widen_bf16x4<NV>(t, raw);
    } else {
        grouped_rot_load<DT_ACC, NV>(acc, numel, v0, lane, full, raw, t);
    }
    grouped_rotate_chunk<BITS, G, false>(raw, numel, g0, full, lane, rot_lo, rot_hi);
    for (int i = 0; i < count; ++i) {
        if (full) {
            const L cur = next;
            grouped_park_term(cur, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            if (i + 1 < count) next.load(terms.in[i + 1], terms.scales[i + 1], terms.zero_points[i + 1], v0, gj, has_group, lane);
        } else {
            grouped_park_term_partial<T>(terms, i, v0, (numel + PACK - 1) / PACK - v0 * T::OB, gj, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
        }
        wave_lds_sync();
        grouped_add_term<DT_F32, DT_F32, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
        wave_lds_sync();
    }
    if constexpr (EARLY) grouped_add_residual<DT_F32, NV>(raw, res);
    else grouped_rot_ef_add_batched<NV, kGroupedRotEfBatchRows>(raw, residual, numel, v0, lane, full);
    grouped_quantize_chunk<DT_F32, BITS, MODE, G, false, NV, true>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a[wave], s_b[wave],
                                                                   s_c[wave]);
    grouped_residual_store<DT_F32, BITS, G>(raw, residual, numel, v0, full, lane, stage, s_c[wave], s_b[wave]);
}

// The guarded form of both calls (terms.count == 0: the quantize), for buffers that are not 16-byte aligned: one wave per group, the group's
// widened values in the block's LDS, rotated there (a whole group only), the terms and then the residual added element by element -- a lane adds
// into the elements it holds --, then the element-by-element tail of grouped_ef_guarded in float32.  The same bytes.  Correct, not fast.
template <int DT_ACC, int BITS, int MODE>
__global__ void __launch_bounds__(kGroupedRotGuardedBlock)
reduce_quantize_grouped_rotated_ef_scalar_kernel(const void* __restrict__ acc, float* residual, uint8_t* __restrict__ out, int64_t numel, int64_t group_size,
                                                 float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo,
                                                 uint32_t rot_hi, float threshold, uint32_t seed_lo, uint32_t seed_hi, uint64_t index_base, GroupedTerms terms) {
    constexpr int PACK = 8 / BITS, QMAX = (1 << BITS) - 1, FORM = DequantForm<BITS, DT_F32>::value;
    __shared__ float buf[kGroupedMaxG];
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t b = g * group_size;
        const int len = static_cast<int>(b + group_size < numel ? group_size : numel - b);
        for (int o = lane; o < len; o += 64) buf[o] = InVec<DT_ACC>::load_scalar(acc, b + o);
        if (len == group_size) grouped_rot_guarded<false>(buf, len, lane, rot_lo, rot_hi);
        for (int i = 0; i < terms.count; ++i) {
            const GroupedRotGuardedTerm<BITS> term(terms, i, g);
            for (int o = lane; o < len; o += 64) buf[o] = __fadd_rn(term(b + o), buf[o]);
        }
        for (int o = lane; o < len; o += 64) buf[o] = __fadd_rn(buf[o], residual[b + o]);
        wave_lds_sync();
        QuantParams p;
        DequantParams d;
        grouped_guarded_params<BITS>([&](int o) { return buf[o]; }, len, lane, false, scales, zero_points, g, threshold, seed_lo, seed_hi, index_base, p, d);
        uint8_t* og = out + b / PACK;   // a group starts on a whole packed byte
        for (int by = lane; by * PACK < len; by += 64) {
            uint32_t word = 0;
            for (int k = 0; k < PACK; ++k) {
                const int o = by * PACK + k;
                if (o >= len) break;
                const float y = buf[o];
                const uint32_t q = quant_one<MODE, QMAX>(y, p, static_cast<uint64_t>(b + o));
                word |= q << (k * BITS);
                residual[b + o] = residual_one<DT_F32>(y, dequant_one<FORM>(q, d));
            }
            og[by] = static_cast<uint8_t>(word);
        }
        wave_lds_sync();
    }
}

}  // namespace pq
