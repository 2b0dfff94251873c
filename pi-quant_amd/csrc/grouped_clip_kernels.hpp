// Per-group clip search for group-wise quantization, in ONE launch that reads the tensor once (include/piquant_hip.h,
// piquant_hip_quantize_grouped_clipped, has the definition; DESIGN.md, "Per-group clip search").
//
// A searched group -- full, hi > lo -- tries `steps` ranges: candidate k shrinks both extremes towards zero, lo_k = fl32(lo r_k),
// hi_k = fl32(hi r_k) with r_k = 1 - k / 16 (exact), takes the ordinary f64 epilogue on (lo_k, hi_k) and is judged by the float32 sum of squared
// errors of the NEAREST round trip through it, whatever the call's rounding mode.  The smallest error wins, ties and NaNs keep the smaller k;
// the group is then quantized once, in the call's mode, with the winner: an ordinary group with other parameters, which every dequantizer takes.
//
// The kernel is quantize_grouped_kernel's wave-owns-a-chunk tile (grouped_kernels.hpp) with a candidate loop between the min / max reduction and the
// quantize pass.  Per candidate: lane j < NG runs the epilogue of group j and parks {1/scale, zero point, scale}; every lane quantizes and
// dequantizes its resident rows and squares the errors; the errors are summed in the order of the ADJACENT-PAIR TREE over the group's elements --
// in the lane (EPV contiguous elements), then an xor butterfly over the group's LPG contiguous lanes (the min / max reduction's lane exchange),
// then, for a group of RPG > 1 rows, the rows in adjacent pairs.  Rows are folded LAST: a row is 64 EPV contiguous elements, so the tree's lower
// levels lie inside it -- the min / max fold may combine a lane's rows first, a float sum may not.  The order is what makes the choice reproducible
// bit for bit by a model that knows nothing of lanes (tests/clip_model.py).  Lane j keeps the best {error, k, scale, zero point} of its group.
// The candidate loop's trip count is a kernel argument: the instances are quantize_grouped's.  (One candidate is quantize_grouped itself: the host
// forwards steps == 1 to it, capi_grouped.cpp.)
//
// Every product, difference and sum of the error is rounded on its own (__fmul_rn / __fsub_rn / __fadd_rn, and the unit compiles with contraction off).
// The candidate passes take the long step (clip_quant_nearest): the short step's bound holds for the unclipped range only with the candidate's own,
// larger 1 / scale, and the long step is right everywhere.  The final pass takes the short step under quantize_grouped's rule, with the winner's
// 1 / scale.
#pragma once

#include "grouped_kernels.hpp"

namespace pq {

constexpr int kGroupedClipMaxSteps = 12;

// the nearest step of the pair's position-independent quantize (with_round_mode, grouped_dispatch.hpp)
template <int DT_IN, int BITS>
struct ClipNearestMode {
    static constexpr int value = (DT_IN == DT_F32 && BITS == 2) ? RM_NEAREST_I64 : RM_NEAREST_FAST;
};

// sum over aligned runs of LPG lanes (a power of two <= 64) in adjacent pairs: lane l with l ^ 1, the pairs with the pairs 2 lanes away, ...
template <int LPG>
__device__ __forceinline__ float segment_sum(float v) {
    if constexpr (LPG > 1) v = __fadd_rn(v, xor_lane<1>(v));
    if constexpr (LPG > 2) v = __fadd_rn(v, xor_lane<2>(v));
    if constexpr (LPG > 4) v = __fadd_rn(v, xor_lane<4>(v));
    if constexpr (LPG > 8) v = __fadd_rn(v, xor_lane<8>(v));
    if constexpr (LPG > 16) v = __fadd_rn(v, xor_lane<16>(v));
    if constexpr (LPG > 32) v = __fadd_rn(v, xor_lane<32>(v));
    return v;
}

// s[0 .. N) summed in adjacent pairs (N a power of two), in place
template <int N>
__device__ __forceinline__ float pair_tree_sum(float (&s)[N]) {
    static_assert((N & (N - 1)) == 0, "a power of two");
#pragma unroll
    for (int n = N; n > 1; n >>= 1) {
#pragma unroll
        for (int j = 0; j < n / 2; ++j) s[j] = __fadd_rn(s[2 * j], s[2 * j + 1]);
    }
    return s[0];
}

// The nearest quantize of a candidate pass.  The generic step (fp32 -> uint2: std::round, then int64 arithmetic) is written without its 64-bit
// branch: the zero point lies in [0, qmax] here, so clamp(int64(r) + zp, 0, qmax) == int(med(r, -zp, qmax - zp)) + zp for every integral r below
// 2^63, and everything else -- r >= 2^63, a NaN -- is the reference's INT64_MIN + zp, which clamps to 0 (r < -2^63 clamps to 0 either way).
template <int DT_IN, int BITS>
__device__ __forceinline__ uint32_t clip_quant_nearest(float x, const QuantParams& p) {
    constexpr int QMAX = (1 << BITS) - 1;
    if constexpr (ClipNearestMode<DT_IN, BITS>::value == RM_NEAREST_I64) {
        const float r = roundf(__fmul_rn(x, p.inv_scale));
        const float zpf = static_cast<float>(p.zp32);
        const float t = __builtin_fminf(__builtin_fmaxf(r, -zpf), static_cast<float>(QMAX) - zpf);
        return r < 9223372036854775808.0f ? static_cast<uint32_t>(static_cast<int32_t>(t) + p.zp32) : 0u;
    } else {
        return quant_one<RM_NEAREST_FAST, QMAX>(x, p, 0);
    }
}

// fl32((x - d)^2) for d = the float32 dequantize of the nearest quantize of x; +0 for a NaN x.  With 0 <= zp <= qmax the pair's float32
// dequantize form is float(int32(q) - zp) * scale for every width (uint2's int64 form computes the same small integer).
template <int DT_IN, int BITS>
__device__ __forceinline__ float clip_error_one(float x, const QuantParams& p, const DequantParams& d) {
    const uint32_t q = clip_quant_nearest<DT_IN, BITS>(x, p);
    const float e = __fsub_rn(x, dequant_one<DQ_SUBMUL>(q, d));
    return x != x ? 0.0f : __fmul_rn(e, e);
}

template <int DT_IN, int BITS>
__device__ __forceinline__ float clip_error_vec(const u32x4& raw, const QuantParams& p, const DequantParams& d) {
    constexpr int EPV = InVec<DT_IN>::EPV;
    float v[EPV], s[EPV];
    InVec<DT_IN>::unpack(raw, v);
#pragma unroll
    for (int e = 0; e < EPV; ++e) s[e] = clip_error_one<DT_IN, BITS>(v[e], p, d);
    return pair_tree_sum<EPV>(s);
}

// Candidate k of the range [lo, hi]: the epilogue on the shrunk extremes.  False for a candidate that is skipped (not hi_k > lo_k); k = 0 is
// quantize_grouped's pair whatever the range is.
template <int BITS>
__device__ __forceinline__ bool clip_candidate(float lo, float hi, int k, float& scale, int64_t& zp) {
    const float r = __fsub_rn(1.0f, __fmul_rn(static_cast<float>(k), 0.0625f));   // exact
    const float lo_k = __fmul_rn(lo, r), hi_k = __fmul_rn(hi, r);
    quant_params_epilogue(float_to_key(lo_k), float_to_key(-hi_k), BITS, scale, zp);   // 0 <= zp <= 2^BITS - 1
    return k == 0 || hi_k > lo_k;
}

// the QuantParams / DequantParams of one (scale, zero point): 1 / scale as the host forms it for quantize_uniform
__device__ __forceinline__ void clip_params(float inv, int32_t zp, float scale, QuantParams& p, DequantParams& d) {
    p = QuantParams {};
    p.inv_scale = inv;
    p.zp32 = zp;
    p.zp64 = zp;
    d = DequantParams {};
    d.scale = scale;
    d.zp32 = zp;
    d.zp64 = zp;
}

// The chunk whose NV rows are in `raw` (grouped_load: elements at or past numel are quiet NaNs, which add +0 to every error): min / max, the
// candidate loop, the winners' parameters and choices written, then quantize_grouped's quantize pass and staged stores.  The wave's LDS slices:
// stage (OUT_BYTES bytes) and s_a, s_b, s_c, s_e (NG floats each).
template <int DT_IN, int BITS, int MODE, int G, int NV_ = GroupedQuantTile<DT_IN, BITS, G>::NV>
__device__ __forceinline__ void grouped_clip_chunk(u32x4 (&raw)[NV_], uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                                   uint8_t* __restrict__ zero_points, uint8_t* __restrict__ choices, int64_t ngroups, int steps,
                                                   const QuantParams& p0, int64_t g0, bool full, int lane, uint8_t* stage, float* s_a, float* s_b,
                                                   float* s_c, float* s_e) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int EPV = T::EPV, OB = T::OB, NV = T::NV, RPG = T::RPG, SETS = T::SETS, LPG = T::LPG, GPR = T::GPR, NG = T::NG;
    constexpr int WORDS = OB > 4 ? 2 : 1, PACK = 8 / BITS;
    const int64_t v0 = g0 * T::V;                                   // first input vector of the chunk
    const int64_t gj = g0 + lane;                                   // lane j < NG: group j of the chunk
    const bool has_group = lane < NG && gj < ngroups;

    {   // the groups' {min, max}, as quantize_grouped finds them (the fold may combine a lane's rows first)
        float lo[SETS], hi[SETS];
#pragma unroll
        for (int s = 0; s < SETS; ++s) {
            lo[s] = 3.402823466e+38f;
            hi[s] = -3.402823466e+38f;
        }
#pragma unroll
        for (int r = 0; r < NV; ++r) minmax_vec<DT_IN>(raw[r], lo[r / RPG], hi[r / RPG]);
#pragma unroll
        for (int s = 0; s < SETS; ++s) {
            segment_minmax<LPG>(lo[s], hi[s]);
            if (lane % LPG == 0) {
                s_a[s * GPR + lane / LPG] = lo[s];
                s_b[s * GPR + lane / LPG] = hi[s];
            }
        }
    }
    wave_lds_sync();
    float glo = 0.0f, ghi = 0.0f;
    if (has_group) {
        glo = s_a[lane];
        ghi = s_b[lane];
    }
    wave_lds_sync();                                                // s_a / s_b are the candidates' from here on
    const bool searched = has_group && ghi > glo && (gj + 1) * G <= numel;   // not a degenerate group, not the ragged last one

    float best_e = 0.0f, best_scale = 1.0f, best_inv = 1.0f;
    int32_t best_zp = 0, best = 0;
#pragma unroll 1
    for (int k = 0; k < steps; ++k) {                               // wave-uniform
        bool ok = false;
        float scale = 1.0f, inv = 1.0f;
        int64_t zp = 0;
        if (has_group && (k == 0 || searched)) {
            ok = clip_candidate<BITS>(glo, ghi, k, scale, zp);
            inv = __fdiv_rn(1.0f, scale);
            s_a[lane] = inv;
            s_b[lane] = __int_as_float(static_cast<int32_t>(zp));
            s_c[lane] = scale;
        }
        wave_lds_sync();
        float err[SETS];
#pragma unroll
        for (int s = 0; s < SETS; ++s) {
            const int slot = s * GPR + lane / LPG;
            QuantParams p;
            DequantParams d;
            clip_params(s_a[slot], __float_as_int(s_b[slot]), s_c[slot], p, d);
            float rows[RPG];
#pragma unroll
            for (int i = 0; i < RPG; ++i) rows[i] = segment_sum<LPG>(clip_error_vec<DT_IN, BITS>(raw[s * RPG + i], p, d));   // lanes first ...
            err[s] = pair_tree_sum<RPG>(rows);                                                                                // ... then rows
        }
#pragma unroll
        for (int s = 0; s < SETS; ++s)
            if (lane % LPG == 0) s_e[s * GPR + lane / LPG] = err[s];
        wave_lds_sync();
        if (ok) {
            const float e = s_e[lane];
            if (k == 0 || e < best_e) {                             // strict: a NaN never wins, a tie keeps the smaller k
                best_e = e;
                best = k;
                best_scale = scale;
                best_inv = inv;
                best_zp = static_cast<int32_t>(zp);
            }
        }
    }

    bool bounded = true;
    if (has_group) {
        st<ST_WT>(scales + gj, best_scale);
        st<ST_WT>(zero_points + gj, static_cast<uint8_t>(best_zp));
        if (choices != nullptr) st<ST_WT>(choices + gj, static_cast<uint8_t>(best));
        // the short step's bound (quant_kernels.hpp, BoundedStep) on the group's UNCLIPPED extremes with the winner's 1 / scale
        bounded = __fmul_rn(__builtin_fmaxf(__builtin_fabsf(glo), __builtin_fabsf(ghi)), best_inv) < 1.0e9f;
        s_a[lane] = best_inv;
        s_b[lane] = __int_as_float(best_zp);
    }
    wave_lds_sync();
    const bool short_step = full && __all(bounded ? 1 : 0) != 0;   // wave-uniform

    // from here on grouped_quantize_chunk's second half, on the parked winners
    [[maybe_unused]] ElementKeys keys {};
    if constexpr (MODE == RM_STOCH_ELEM) keys = element_keys_for(p0, p0.index_base + static_cast<uint64_t>(v0 + lane) * EPV);
    QuantParams p[SETS];
    BoundedStep bstep[SETS];
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
        const int slot = s * GPR + lane / LPG;
        p[s] = p0;
        p[s].dyn = nullptr;
        p[s].inv_scale = s_a[slot];
        p[s].zp32 = __float_as_int(s_b[slot]);
        p[s].zp64 = p[s].zp32;
        bstep[s] = bounded_step_for<BITS>(p[s].zp32);
    }
    uint32_t w[NV][WORDS];
    if (short_step) {
#pragma unroll
        for (int r = 0; r < NV; ++r)
            quantize_vec_short<DT_IN, BITS, MODE>(raw[r], p[r / RPG], keys, static_cast<uint64_t>(v0 + r * 64 + lane) * EPV, bstep[r / RPG], w[r]);
    } else {
#pragma unroll
        for (int r = 0; r < NV; ++r) quantize_vec<DT_IN, BITS, MODE>(raw[r], p[r / RPG], keys, static_cast<uint64_t>(v0 + r * 64 + lane) * EPV, w[r]);
    }
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        uint8_t* dst = stage + (r * 64 + lane) * OB;
        if constexpr (OB == 1) *dst = static_cast<uint8_t>(w[r][0]);
        else if constexpr (OB == 2) *reinterpret_cast<uint16_t*>(dst) = static_cast<uint16_t>(w[r][0]);
        else if constexpr (OB == 4) *reinterpret_cast<uint32_t*>(dst) = w[r][0];
        else *reinterpret_cast<u32x2*>(dst) = u32x2 {w[r][0], w[r][1]};
    }
    wave_lds_sync();
    uint8_t* o = out + v0 * OB;
    if (full) {
        if constexpr (T::LANE_OUT_BYTES >= 16) {
#pragma unroll
            for (int j = 0; j < T::LANE_OUT_BYTES / 16; ++j)
                st<ST_WT>(reinterpret_cast<u32x4*>(o) + j * 64 + lane, reinterpret_cast<const u32x4*>(stage)[j * 64 + lane]);
        } else if constexpr (T::LANE_OUT_BYTES == 8) {
            st<ST_WT>(reinterpret_cast<u32x2*>(o) + lane, reinterpret_cast<const u32x2*>(stage)[lane]);
        } else {
            st<ST_WT>(reinterpret_cast<uint32_t*>(o) + lane, reinterpret_cast<const uint32_t*>(stage)[lane]);
        }
    } else {
        const int64_t left = (numel + PACK - 1) / PACK - v0 * OB;   // bytes of the tensor from the chunk's first byte on (< OUT_BYTES)
        for (int b = lane; b < left; b += 64) o[b] = stage[b];
    }
}

template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_clipped_kernel(const void* __restrict__ in, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                uint8_t* __restrict__ zero_points, int64_t ngroups, uint8_t* __restrict__ choices, int steps, QuantParams p0) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG], s_e[WAVES][NG];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform

    u32x4 raw[NV];
    grouped_load<DT_IN, NV>(in, numel, g0 * T::V, lane, full, raw);
    grouped_clip_chunk<DT_IN, BITS, MODE, G>(raw, out, numel, scales, zero_points, choices, ngroups, steps, p0, g0, full, lane, s_out[wave], s_a[wave],
                                             s_b[wave], s_c[wave], s_e[wave]);
}

// Batch: quantize_grouped_batch_kernel's table with the members' choices (an entry may be NULL)
struct GroupedClipBatchArgs {
    const void* in[kGroupedBatchMax];
    uint8_t* out[kGroupedBatchMax];
    float* scales[kGroupedBatchMax];
    uint8_t* zero_points[kGroupedBatchMax];
    uint8_t* choices[kGroupedBatchMax];
    int64_t numel[kGroupedBatchMax];
    int64_t chunk_begin[kGroupedBatchMax + 1];
    int count;
};

template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_clipped_batch_kernel(GroupedClipBatchArgs a, int steps, QuantParams p0) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG], s_e[WAVES][NG];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    const int64_t ngroups = (numel + G - 1) / G;
    const int64_t g0 = (c - a.chunk_begin[t]) * NG;
    const bool full = (g0 + NG) * G <= numel;

    u32x4 raw[NV];
    grouped_load<DT_IN, NV>(a.in[t], numel, g0 * T::V, lane, full, raw);
    grouped_clip_chunk<DT_IN, BITS, MODE, G>(raw, a.out[t], numel, a.scales[t], a.zero_points[t], a.choices[t], ngroups, steps, p0, g0, full, lane,
                                             s_out[wave], s_a[wave], s_b[wave], s_c[wave], s_e[wave]);
}

// The guarded kernel, for buffers that are not 16-byte aligned: one wave per group, element by element, the same bytes.  Correct, not fast.
// The same tree: a lane takes four contiguous elements of every run of 256, the wave's butterfly sums a run, the runs are summed in adjacent
// pairs.  A lane or a run past the group's end adds +0, which changes no sum of squares (x + 0 == x for every x >= +0, infinities and NaNs too).
template <int DT_IN, int BITS, int MODE>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_clipped_scalar_kernel(const void* __restrict__ in, uint8_t* __restrict__ out, int64_t numel, int64_t group_size, float* __restrict__ scales,
                                       uint8_t* __restrict__ zero_points, int64_t ngroups, uint8_t* __restrict__ choices, int steps, QuantParams p0) {
    constexpr int PACK = 8 / BITS, QMAX = (1 << BITS) - 1, RUN = 256, RUNS = kGroupedMaxG / RUN;
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kGroupedBlock / 64);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the group loop is wave-uniform
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * (kGroupedBlock / 64) + wave; g < ngroups; g += waves) {
        const int64_t b = g * group_size, e = b + group_size < numel ? b + group_size : numel;
        const int len = static_cast<int>(e - b);
        float lo = 3.402823466e+38f, hi = -3.402823466e+38f;   // the scan's identities (minmax_kernels.hpp)
        for (int o0 = 0; o0 < len; o0 += 64) {
            if (o0 + lane < len) {
                const float x = quieted(InVec<DT_IN>::load_scalar(in, b + o0 + lane));
                lo = __builtin_fminf(lo, x);
                hi = __builtin_fmaxf(hi, x);
            }
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        const bool searched = hi > lo && len == group_size;
        float best_e = 0.0f, best_scale = 1.0f;
        int64_t best_zp = 0;
        int best = 0;
#pragma unroll 1
        for (int k = 0; k < steps; ++k) {
            if (k != 0 && !searched) break;
            float scale;
            int64_t zp;
            const bool ok = clip_candidate<BITS>(lo, hi, k, scale, zp);
            QuantParams p;
            DequantParams d;
            clip_params(__fdiv_rn(1.0f, scale), static_cast<int32_t>(zp), scale, p, d);
            float runs[RUNS];
#pragma unroll
            for (int r = 0; r < RUNS; ++r) {
                float s[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = r * RUN + lane * 4 + i;
                    s[i] = o < len ? clip_error_one<DT_IN, BITS>(InVec<DT_IN>::load_scalar(in, b + o), p, d) : 0.0f;
                }
                runs[r] = segment_sum<64>(pair_tree_sum<4>(s));
            }
            const float err = pair_tree_sum<RUNS>(runs);
            if (ok && (k == 0 || err < best_e)) {
                best_e = err;
                best = k;
                best_scale = scale;
                best_zp = zp;
            }
        }
        if (lane == 0) {
            scales[g] = best_scale;
            zero_points[g] = static_cast<uint8_t>(best_zp);
            if (choices != nullptr) choices[g] = static_cast<uint8_t>(best);
        }
        QuantParams p = p0;
        p.dyn = nullptr;
        p.inv_scale = __fdiv_rn(1.0f, best_scale);
        p.zp64 = best_zp;
        p.zp32 = static_cast<int32_t>(best_zp);
        for (int64_t by = b / PACK + lane; by < (e + PACK - 1) / PACK; by += 64) {
            uint32_t acc = 0;
            for (int i = 0; i < PACK; ++i) {
                const int64_t idx = by * PACK + i;
                if (idx >= numel) break;
                acc |= quant_one<MODE, QMAX>(InVec<DT_IN>::load_scalar(in, idx), p, static_cast<uint64_t>(idx)) << (i * BITS);
            }
            out[by] = static_cast<uint8_t>(acc);
        }
    }
}

}  // namespace pq
