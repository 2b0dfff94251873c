// Group-wise quantization for gfx950: one (scale, zero point) per run of G contiguous elements, G a power of two in [32, 4096].
//
// Semantics (include/piquant_hip.h, piquant_hip_quantize_grouped): group g covers [g G, min((g + 1) G, numel)); its parameters are what
// piquant_hip_compute_quant_params_device writes for that slice alone (NaNs ignored, a group of nothing but NaNs gets (1.0, qmax >> 1), the
// f64 epilogue of minmax_kernels.hpp), and its bytes are piquant_hip_quantize_uniform of the slice with them -- the position-independent form.
// Because G >= 32 is a power of two, every group starts on a whole packed byte and on a 16-byte input boundary, so the output is exactly the
// per-group outputs laid end to end.
//
// Quantize: ONE streaming launch, no scan, no atomics, no grid barrier.  A wave owns a "chunk" of NG whole groups = NV rows of 64 consecutive
// 16-byte input vectors (row r, lane l: vector r * 64 + l of the chunk, one coalesced 1 KiB load per row).  A group is V = G / EPV vectors:
//   V <= 64   a group is LPG = V consecutive lanes of one row; the row holds 64 / V groups.  min / max: a segmented xor reduction of log2(V)
//             steps (DPP quad permutes for 1 and 2, ds_swizzle for 4 .. 16 -- no LDS memory traffic -- and ds_bpermute for 32)
//   V > 64    a group is RPG = V / 64 rows: every lane folds its RPG vectors, then the whole wave reduces (six steps)
// The lane that starts a group parks the group's {min, max} in the wave's LDS slice; lane j < NG then runs the f64 epilogue for group j of the
// chunk (one epilogue per group, not per lane), writes scales[g] / zero_points[g] (contiguous runs) and parks {1/scale, zp} for the lanes that
// quantize.  Quantization and packing are the uniform kernels' (quantize_vec / quantize_vec_short), with the parameters in VGPRs instead of
// SGPRs; the packed bytes go through the wave's LDS slice so that every lane writes 16 contiguous bytes with a write-through store.
// The wave's last chunk may be partial (the tensor ends inside it): its missing elements are read as quiet NaNs -- which the fold ignores and
// which quantize to 0, the bits a ragged quantize_uniform tail leaves empty -- and its stores are cut at the tensor's last packed byte.
//
// Fused reduce + quantize (reduce_quantize_grouped_kernel): the quantize tile with up to 16 packed terms added into the resident rows first,
// each term's chunk staged through the wave's LDS slice and dequantized with its own group parameters -- the bytes of grouped dequantize ADD per
// term followed by quantize.  Batches (quantize_grouped_batch_kernel, dequantize_grouped_batch_kernel): up to 16 tensors in one launch, a wave
// finding its tensor in a prefix table of chunk counts, then running the single kernel's body.
//
// Dequantize: a wave owns NIN KiB of packed input (16 bytes per lane and row), staged through LDS and read back as the packed bytes of one
// 16-byte output vector per lane and step, so that loads and stores are both coalesced 16-byte accesses; the group parameters of the chunk are
// loaded once into LDS and every output vector picks its group's.
//
// The helpers the kernels are made of, each rule stated on the one that owns it:
//   grouped_batch_tensor          a wave's tensor in a batch's prefix table (all five batch kernels, grouped_requant_kernels.hpp's included)
//   staged_words                  the packed bytes of one vector out of the wave's LDS slice, as dwords
//   grouped_dequantize_row        staged_words + dequant_one over a lane-row: the read-back of a staged term and of the chunk's own output
//   grouped_load / _bf16x4        a chunk's rows from memory, quiet NaNs behind the tensor's end; grouped_widen_bf16x4 widens the packed rows
//   grouped_quantize_chunk        parameters, quantization and staged stores of one chunk (KEEP / REQUANT: the chunk stays readable)
//   GroupedTermLoad, grouped_park_term / grouped_park_term_partial, grouped_term_dequant_params, grouped_add_term
//                                 a term of the fused reduce kernels: loaded a term ahead, staged (full chunk / partial chunk), gathered, added
//   grouped_set_term              the first term of a dequantize-sum SET (dequantize_sum_grouped_kernel, at the end): stored, not added
//   grouped_guarded_params        the group prologue of the four guarded quantizing kernels
//   grouped_add_residual, residual_one, grouped_parked_dequant_params, grouped_store_vector, grouped_residual_store
//                                 the error-feedback steps around the chunk body; grouped_ef_chunk is the whole tile for both residual types
// A kernel's code depends on how these are cut, not only on what they say: the notes "by reference", "G is not used" and "written out" on some of
// them record forms that were tried and compiled to other code (profiles/EXPERIMENTS.md, "Shared helpers for the grouped kernels").
#pragma once

#include "dequant_kernels.hpp"
#include "fused_kernels.hpp"
#include "minmax_kernels.hpp"
#include "quant_kernels.hpp"

#include <type_traits>

namespace pq {

constexpr int kGroupedBlock = 256;   // four waves; waves never wait for one another (LDS slices are per wave)

// lane l's value against lane l ^ OFF's: DPP quad permutes (VALU), ds_swizzle in bitmask mode inside 32 lanes (LDS pipe, no memory), ds_bpermute for 32
template <int OFF>
__device__ __forceinline__ float xor_lane(float v) {
    const int i = __builtin_bit_cast(int, v);
    int r;
    if constexpr (OFF == 1) r = __builtin_amdgcn_update_dpp(i, i, 0xb1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
    else if constexpr (OFF == 2) r = __builtin_amdgcn_update_dpp(i, i, 0x4e, 0xf, 0xf, false); // quad_perm [2,3,0,1]
    else if constexpr (OFF < 32) r = __builtin_amdgcn_ds_swizzle(i, 0x1f | (OFF << 10));       // and 0x1f, or 0, xor OFF
    else r = __shfl_xor(i, 32);
    return __builtin_bit_cast(float, r);
}

// min / max over aligned runs of LPG lanes (LPG a power of two <= 64): every lane of a run ends with the run's result
template <int LPG>
__device__ __forceinline__ void segment_minmax(float& lo, float& hi) {
    if constexpr (LPG > 1) { lo = __builtin_fminf(lo, xor_lane<1>(lo)); hi = __builtin_fmaxf(hi, xor_lane<1>(hi)); }
    if constexpr (LPG > 2) { lo = __builtin_fminf(lo, xor_lane<2>(lo)); hi = __builtin_fmaxf(hi, xor_lane<2>(hi)); }
    if constexpr (LPG > 4) { lo = __builtin_fminf(lo, xor_lane<4>(lo)); hi = __builtin_fmaxf(hi, xor_lane<4>(hi)); }
    if constexpr (LPG > 8) { lo = __builtin_fminf(lo, xor_lane<8>(lo)); hi = __builtin_fmaxf(hi, xor_lane<8>(hi)); }
    if constexpr (LPG > 16) { lo = __builtin_fminf(lo, xor_lane<16>(lo)); hi = __builtin_fmaxf(hi, xor_lane<16>(hi)); }
    if constexpr (LPG > 32) { lo = __builtin_fminf(lo, xor_lane<32>(lo)); hi = __builtin_fmaxf(hi, xor_lane<32>(hi)); }
}

// same-wave LDS writes visible to the wave's later reads (DS operations of one wave execute in order; this keeps the compiler from reordering)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Batches: the chunks of tensor t are [chunk_begin[t], chunk_begin[t + 1]) of the grid's waves.  The tensor of wave c of the grid from that prefix
// table (wave-uniform, <= 15 compares); false for a wave behind the batch's last chunk.  The wave's chunk inside its tensor is c - a.chunk_begin[t].
// Args is the kernel's argument table, by reference: handed the table and the count as values, or left to return t, the search loop compiled to a
// different scalar prologue in every batch kernel (profiles/EXPERIMENTS.md).
template <class Args>
__device__ __forceinline__ bool grouped_batch_tensor(const Args& a, int64_t c, int& t) {
    if (c >= a.chunk_begin[a.count]) return false;
    t = 0;
    while (t + 1 < a.count && c >= a.chunk_begin[t + 1]) ++t;
    return true;
}

// The NB = 1, 2, 4 or 8 packed bytes at `src` (NB-aligned, in the wave's LDS slice) as dwords: one LDS read of exactly that width.
template <int NB>
__device__ __forceinline__ void staged_words(const uint8_t* src, uint32_t (&w)[NB > 4 ? 2 : 1]) {
    static_assert(NB == 1 || NB == 2 || NB == 4 || NB == 8, "the packed bytes of one 16-byte vector");
    if constexpr (NB == 1) w[0] = *src;
    else if constexpr (NB == 2) w[0] = *reinterpret_cast<const uint16_t*>(src);
    else if constexpr (NB == 4) w[0] = *reinterpret_cast<const uint32_t*>(src);
    else {
        const u32x2 t = *reinterpret_cast<const u32x2*>(src);
        w[0] = t[0];
        w[1] = t[1];
    }
}

// f = the lane's vector of row r of a chunk of the tile of type DT (InVec<DT>::EPV elements, OB = EPV * BITS / 8 packed bytes at vector r * 64 + lane
// of `stage`), dequantized with p in FORM -- the tile's own pair unless the accumulator has another type.  The one read-back of the wave's LDS
// slice: a term's staged chunk (grouped_add_term) and the chunk's own packed output (grouped_residual_store, grouped_requant_store).  G is not used:
// it keeps one instance per tile, as there was -- with one shared by all group sizes a quantize-dequantize kernel came out scheduled differently.
template <int DT, int BITS, int G, int FORM = DequantForm<BITS, DT>::value>
__device__ __forceinline__ void grouped_dequantize_row(const uint8_t* stage, int r, int lane, const DequantParams& p, float (&f)[InVec<DT>::EPV]) {
    constexpr int EPV = InVec<DT>::EPV, OB = EPV * BITS / 8;
    uint32_t w[OB > 4 ? 2 : 1];
    staged_words<OB>(stage + (r * 64 + lane) * OB, w);
#pragma unroll
    for (int e = 0; e < EPV; ++e) f[e] = dequant_one<FORM>((w[(e * BITS) >> 5] >> ((e * BITS) & 31)) & ((1u << BITS) - 1u), p);
}

template <int DT_IN, int BITS, int G>
struct GroupedQuantTile {
    static constexpr int EPV = InVec<DT_IN>::EPV;
    static constexpr int OB = EPV * BITS / 8;                       // packed bytes per input vector
    static constexpr int V = G / EPV;                               // vectors per group
    static constexpr int LPG = V < 64 ? V : 64;                     // lanes per group (per row)
    static constexpr int RPG = V < 64 ? 1 : V / 64;                 // rows per group
    static constexpr int NV_WANT = (16 / OB) > 4 ? 16 / OB : 4;     // rows for 16 output bytes per lane (at least 4 loads in flight)
    static constexpr int NV = RPG > (V < NV_WANT ? V : NV_WANT) ? RPG : (V < NV_WANT ? V : NV_WANT);   // rows per lane (<= V: at most 64 groups)
    static constexpr int SETS = NV / RPG;                           // groups per lane
    static constexpr int GPR = 64 / LPG;                            // groups per row
    static constexpr int NG = SETS * GPR;                           // groups per chunk
    static constexpr int CHUNK_ELEMS = NV * 64 * EPV;
    static constexpr int OUT_BYTES = NV * 64 * OB;
    static constexpr int LANE_OUT_BYTES = NV * OB;
    static_assert(NG >= 1 && NG <= 64 && NG * G == CHUNK_ELEMS, "a chunk is 1..64 whole groups");
    static_assert(LANE_OUT_BYTES % 16 == 0 || LANE_OUT_BYTES == 8 || LANE_OUT_BYTES == 4, "store shapes of the staged output");
};

// one wave's chunk of `in` as NV rows of 16-byte vectors; elements at or past numel read as quiet NaNs
template <int DT_IN, int NV>
__device__ __forceinline__ void grouped_load(const void* in, int64_t numel, int64_t v0, int lane, bool full, u32x4 (&raw)[NV]) {
    constexpr int EPV = InVec<DT_IN>::EPV;
    const u32x4* in16 = static_cast<const u32x4*>(in);
    if (full) {
#pragma unroll
        for (int r = 0; r < NV; ++r) raw[r] = ld<true>(in16 + v0 + r * 64 + lane);
        return;
    }
    constexpr uint32_t QNAN = DT_IN == DT_F32 ? 0x7fc00000u : 0x7fc07fc0u;
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        const int64_t vec = v0 + r * 64 + lane;
        if ((vec + 1) * EPV <= numel) {
            raw[r] = ld<true>(in16 + vec);
        } else {
            raw[r] = u32x4 {QNAN, QNAN, QNAN, QNAN};
#pragma unroll
            for (int e = 0; e < EPV; ++e) {   // unrolled: constant register indices
                const int64_t i = vec * EPV + e;
                if (i >= numel) continue;
                if constexpr (DT_IN == DT_F32) raw[r][e] = static_cast<const uint32_t*>(in)[i];
                else raw[r][e >> 1] = (raw[r][e >> 1] & ((e & 1) ? 0x0000ffffu : 0xffff0000u)) |
                                      (static_cast<uint32_t>(static_cast<const uint16_t*>(in)[i]) << ((e & 1) * 16));
            }
        }
    }
}

// The rows of a tensor of type DT on the tile of type DT_TILE.  DT == DT_TILE: the tile's own 16-byte vectors (grouped_load).  A bfloat16 tensor on
// the float32 tile (error feedback with a float32 residual): a lane-row is four elements, which are 8 bytes of the tensor (one global_load_dwordx2,
// 512 contiguous bytes per wave-row), kept PACKED (u32x2: two bfloat16 a dword) until grouped_widen_bf16x4.
template <int DT, int DT_TILE>
using GroupedRow = std::conditional_t<DT == DT_TILE, u32x4, u32x2>;

// one wave's chunk of the bfloat16 tensor `in` as NV rows of four elements, still packed (8 bytes a lane-row); elements at or past numel read as
// quiet NaNs.  Load only: nothing here uses what it loads, so that the residual's loads can be issued behind these without a wait between them.
template <int NV>
__device__ __forceinline__ void grouped_load_bf16x4(const void* in, int64_t numel, int64_t v0, int lane, bool full, u32x2 (&t)[NV]) {
    const u32x2* in8 = static_cast<const u32x2*>(in);
    if (full) {
#pragma unroll
        for (int r = 0; r < NV; ++r) t[r] = ld<true>(in8 + v0 + r * 64 + lane);
        return;
    }
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        const int64_t vec = v0 + r * 64 + lane;
        if ((vec + 1) * 4 <= numel) {
            t[r] = ld<true>(in8 + vec);
        } else {
            t[r] = u32x2 {0x7fc07fc0u, 0x7fc07fc0u};
#pragma unroll
            for (int e = 0; e < 4; ++e) {   // unrolled: constant register indices
                const int64_t i = vec * 4 + e;
                if (i >= numel) continue;
                t[r][e >> 1] = (t[r][e >> 1] & ((e & 1) ? 0x0000ffffu : 0xffff0000u)) |
                               (static_cast<uint32_t>(static_cast<const uint16_t*>(in)[i]) << ((e & 1) * 16));
            }
        }
    }
}

// the packed rows widened to float32 bits: raw[r][e] = bits << 16.  Loading and widening are two steps on purpose: a load that widened in place
// would put a use between the tensor's loads and the residual's.
template <int NV>
__device__ __forceinline__ void grouped_widen_bf16x4(const u32x2 (&t)[NV], u32x4 (&raw)[NV]) {
#pragma unroll
    for (int r = 0; r < NV; ++r) raw[r] = u32x4 {t[r][0] << 16, t[r][0] & 0xffff0000u, t[r][1] << 16, t[r][1] & 0xffff0000u};
}

// Quantize of one chunk whose NV rows are in `raw` (grouped_load: elements at or past numel are quiet NaNs): parameters, quantization, staged
// stores.  GIVEN: scales / zero_points are inputs ("quantize with these per-group parameters", no reduction); otherwise they are written.
// p0 carries what is per call (threshold, seed, index base); its inv_scale / zero point are replaced per group.  The wave's LDS
// slices (stage: OUT_BYTES bytes; s_a, s_b: NG floats each).  KEEP (the error-feedback kernels): the chunk stays readable after the call --
// `stage` holds its packed bytes, s_a / s_b the groups' {1/scale, zero point} and s_scale (NG floats) their scales; nothing else changes.
// REQUANT (the fake-quantization kernels, with KEEP): the packed bytes stay in `stage` and never go to memory (`out` is not used), computed
// parameters are written only when `scales` is not NULL, and given-or-computed is the wave-uniform runtime flag `given_rt` instead of GIVEN.
// The default leaves every other instantiation as it was (their `given` below is a compile-time constant).
template <int DT_IN, int BITS, int MODE, int G, bool GIVEN, int NV_ = GroupedQuantTile<DT_IN, BITS, G>::NV, bool KEEP = false, bool REQUANT = false>
__device__ __forceinline__ void grouped_quantize_chunk(u32x4 (&raw)[NV_], uint8_t* __restrict__ out, int64_t numel,
                                                       float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, const QuantParams& p0,
                                                       int64_t g0, bool full, int lane, uint8_t* stage, float* s_a, float* s_b,
                                                       float* s_scale = nullptr, bool given_rt = false) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int EPV = T::EPV, OB = T::OB, NV = T::NV, RPG = T::RPG, SETS = T::SETS, LPG = T::LPG, GPR = T::GPR, NG = T::NG;
    constexpr int WORDS = OB > 4 ? 2 : 1, PACK = 8 / BITS;
    const int64_t v0 = g0 * T::V;                                   // first input vector of the chunk

    const int64_t gj = g0 + lane;                                   // lane j < NG: group j of the chunk
    bool bounded = true;
    const bool given = REQUANT ? given_rt : GIVEN;
    if (given) {
        if (lane < NG && gj < ngroups) {
            const float scale = scales[gj];
            s_a[lane] = __fdiv_rn(1.0f, scale);                     // as the host forms 1 / scale for quantize_uniform
            s_b[lane] = __int_as_float(static_cast<int32_t>(zero_points[gj]));
            if constexpr (KEEP) s_scale[lane] = scale;
        }
        bounded = false;                                            // no data range known: the long step everywhere
    } else {
        float lo[SETS], hi[SETS];
#pragma unroll
        for (int s = 0; s < SETS; ++s) {
            lo[s] = 3.402823466e+38f;                               // the scan's identities (minmax_kernels.hpp)
            hi[s] = -3.402823466e+38f;
        }
#pragma unroll
        for (int r = 0; r < NV; ++r) minmax_vec<DT_IN>(raw[r], lo[r / RPG], hi[r / RPG]);   // every element quieted first: a signaling NaN poisons nothing
#pragma unroll
        for (int s = 0; s < SETS; ++s) {
            segment_minmax<LPG>(lo[s], hi[s]);
            if (lane % LPG == 0) {
                s_a[s * GPR + lane / LPG] = lo[s];
                s_b[s * GPR + lane / LPG] = hi[s];
            }
        }
        wave_lds_sync();
        if (lane < NG && gj < ngroups) {
            const float glo = s_a[lane], ghi = s_b[lane];
            float scale;
            int64_t zp;
            quant_params_epilogue(float_to_key(glo), float_to_key(-ghi), BITS, scale, zp);   // 0 <= zp <= 2^BITS - 1
            const float inv = __fdiv_rn(1.0f, scale);
            if (!REQUANT || scales != nullptr) {
                st<ST_WT>(scales + gj, scale);
                st<ST_WT>(zero_points + gj, static_cast<uint8_t>(zp));
            }
            // the short step needs |x / scale| far below 2^31 for every element: |x| <= max(|min|, |max|) (quant_kernels.hpp, BoundedStep)
            bounded = __fmul_rn(__builtin_fmaxf(__builtin_fabsf(glo), __builtin_fabsf(ghi)), inv) < 1.0e9f;
            s_a[lane] = inv;
            s_b[lane] = __int_as_float(static_cast<int32_t>(zp));
            if constexpr (KEEP) s_scale[lane] = scale;
        }
    }
    wave_lds_sync();
    const bool short_step = full && __all(bounded ? 1 : 0) != 0;   // wave-uniform

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

    // stage the chunk's packed bytes, then lane-contiguous write-through stores
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        uint8_t* dst = stage + (r * 64 + lane) * OB;
        if constexpr (OB == 1) *dst = static_cast<uint8_t>(w[r][0]);
        else if constexpr (OB == 2) *reinterpret_cast<uint16_t*>(dst) = static_cast<uint16_t>(w[r][0]);
        else if constexpr (OB == 4) *reinterpret_cast<uint32_t*>(dst) = w[r][0];
        else *reinterpret_cast<u32x2*>(dst) = u32x2 {w[r][0], w[r][1]};
    }
    wave_lds_sync();
    if constexpr (REQUANT) return;
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

template <int DT_IN, int BITS, int MODE, int G, bool GIVEN>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_kernel(const void* __restrict__ in, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales, uint8_t* __restrict__ zero_points,
                        int64_t ngroups, QuantParams p0) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];   // {min, max} of the chunk's groups, then {1/scale, zero point}

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform

    u32x4 raw[NV];
    grouped_load<DT_IN, NV>(in, numel, g0 * T::V, lane, full, raw);
    grouped_quantize_chunk<DT_IN, BITS, MODE, G, GIVEN>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, s_out[wave], s_a[wave], s_b[wave]);
}

// Batch: up to kGroupedBatchMax independent tensors in ONE launch.  A wave finds its tensor and its chunk (grouped_batch_tensor) and then runs exactly
// the single-tensor kernel's body.  The four argument tables (this one, GroupedDequantBatchArgs, GroupedEfBatchArgs, GroupedRequantBatchArgs) stay
// four plain structs: their member types differ, and one template or a shared base would change the kernels' mangled names or the kernarg layout.
constexpr int kGroupedBatchMax = 16;
struct GroupedQuantBatchArgs {
    const void* in[kGroupedBatchMax];
    uint8_t* out[kGroupedBatchMax];
    float* scales[kGroupedBatchMax];
    uint8_t* zero_points[kGroupedBatchMax];
    int64_t numel[kGroupedBatchMax];
    int64_t chunk_begin[kGroupedBatchMax + 1];
    int count;
};

template <int DT_IN, int BITS, int MODE, int G, bool GIVEN>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_batch_kernel(GroupedQuantBatchArgs a, QuantParams p0) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];

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
    grouped_quantize_chunk<DT_IN, BITS, MODE, G, GIVEN>(raw, a.out[t], numel, a.scales[t], a.zero_points[t], ngroups, p0, g0, full, lane, s_out[wave],
                                                        s_a[wave], s_b[wave]);
}

// Fused reduce + quantize: out, scales, zero_points = quantize_grouped(acc + dequantize_grouped(in_0) + ... + dequantize_grouped(in_{k-1})), the terms
// added in order with the running sum rounded to the accumulator's type after each one -- the bytes of k grouped dequantize ADD calls into acc
// followed by quantize_grouped(acc), without the sum ever leaving the registers.  The terms are packed tensors of the same numel and group size,
// each with its own per-group parameters (same G as the output groups).  A term's chunk is NV * 64 * OB contiguous bytes: staged through the
// wave's LDS slice with coalesced 16-byte loads (the next term's in flight while the current one is added), read back as the OB packed bytes of
// each of the lane's NV input vectors; lane j < NG loads group j's {scale, zero point}.
constexpr int kGroupedReduceMaxTerms = 16;
struct GroupedTerms {
    const uint8_t* in[kGroupedReduceMaxTerms];
    const float* scales[kGroupedReduceMaxTerms];
    const uint8_t* zero_points[kGroupedReduceMaxTerms];
    int count;
};

template <int DT_IN, int BITS, int G>
struct GroupedTermLoad {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    static constexpr int LOB = T::LANE_OUT_BYTES;
    static constexpr int N16 = LOB >= 16 ? LOB / 16 : 1;   // 16-byte loads per lane (one 8- or 4-byte load below 16)
    u32x4 v[N16];
    float scale, bias;
    int32_t zp;

    // full chunk: the lane's share of the chunk's packed bytes (coalesced) and, for lane j < NG, group j's parameters
    __device__ __forceinline__ void load(const uint8_t* __restrict__ q, const float* __restrict__ sc, const uint8_t* __restrict__ zps, int64_t v0, int64_t gj,
                                         bool has_group, int lane) {
        const uint8_t* c = q + v0 * T::OB;
        if constexpr (LOB >= 16) {
#pragma unroll
            for (int j = 0; j < N16; ++j) v[j] = ld<true>(reinterpret_cast<const u32x4*>(c) + j * 64 + lane);
        } else if constexpr (LOB == 8) {
            const u32x2 t = ld<true>(reinterpret_cast<const u32x2*>(c) + lane);
            v[0] = u32x4 {t[0], t[1], 0u, 0u};
        } else {
            v[0] = u32x4 {ld<true>(reinterpret_cast<const uint32_t*>(c) + lane), 0u, 0u, 0u};
        }
        params(sc, zps, gj, has_group);
    }

    __device__ __forceinline__ void params(const float* __restrict__ sc, const uint8_t* __restrict__ zps, int64_t gj, bool has_group) {
        if (has_group) {
            scale = sc[gj];
            zp = zps[gj];
        }
    }

    __device__ __forceinline__ void park(uint8_t* stage, int lane) const {
        if constexpr (LOB >= 16) {
#pragma unroll
            for (int j = 0; j < N16; ++j) reinterpret_cast<u32x4*>(stage)[j * 64 + lane] = v[j];
        } else if constexpr (LOB == 8) {
            reinterpret_cast<u32x2*>(stage)[lane] = u32x2 {v[0][0], v[0][1]};
        } else {
            reinterpret_cast<uint32_t*>(stage)[lane] = v[0][0];
        }
    }
};

// Staging a term: its chunk's packed bytes into `stage` and, from lane j < NG, group j's {scale, bias, zero point} into the wave's LDS slices, where
// grouped_add_term finds them.  A full chunk comes out of the registers of a GroupedTermLoad (loaded a term ahead) ...
template <class L>
__device__ __forceinline__ void grouped_park_term(const L& t, uint8_t* stage, float* s_scale, float* s_bias, int32_t* s_zp, bool has_group, int lane) {
    t.park(stage, lane);
    if (has_group) {
        s_scale[lane] = t.scale;
        s_bias[lane] = __fmul_rn(-static_cast<float>(t.zp), t.scale);   // as resolved(DequantParams) forms it
        s_zp[lane] = t.zp;
    }
}

// ... and a chunk the tensor ends in (at vector v0 of term i, `left` bytes before the tensor's last packed byte) straight from memory: byte loads
// up to that byte, zeros behind it -- they meet the quiet NaNs of the accumulator's missing elements, which stay NaN.  T: the tile.  The terms
// come as the kernel's argument by reference: handed the term's three pointers as values, the scalar loads of the two parameter pointers moved in
// front of the byte loop in every reduce kernel.
template <class T, class Terms>
__device__ __forceinline__ void grouped_park_term_partial(const Terms& terms, int i, int64_t v0, int64_t left, int64_t gj, uint8_t* stage, float* s_scale,
                                                          float* s_bias, int32_t* s_zp, bool has_group, int lane) {
    const uint8_t* c = terms.in[i] + v0 * T::OB;
    for (int b = lane; b < T::OUT_BYTES; b += 64) stage[b] = b < left ? c[b] : 0;
    if (has_group) {
        const float scale = terms.scales[i][gj];
        const int32_t zp = terms.zero_points[i][gj];
        s_scale[lane] = scale;
        s_bias[lane] = __fmul_rn(-static_cast<float>(zp), scale);
        s_zp[lane] = zp;
    }
}

// the dequantize parameters of the lane's SETS groups (tile T) from a parked term's {scale, bias, zero point} (grouped_park_term)
template <class T>
__device__ __forceinline__ void grouped_term_dequant_params(DequantParams (&p)[T::SETS], const float* s_scale, const float* s_bias, const int32_t* s_zp,
                                                            int lane) {
#pragma unroll
    for (int s = 0; s < T::SETS; ++s) {
        const int slot = s * T::GPR + lane / T::LPG;
        p[s] = DequantParams {};
        p[s].scale = s_scale[slot];
        p[s].bias = s_bias[slot];
        p[s].zp32 = s_zp[slot];
        p[s].zp64 = p[s].zp32;
    }
}

// x[r] = rn(x[r] + the dequantized packed bytes of vector r of the lane) in the accumulator's type DT_ACC, group parameters per set: the arithmetic
// of a grouped dequantize ADD, in the pair's form uint -> DT_ACC, on the geometry of the tile of type DT_TILE.  A bfloat16 accumulator, on its own
// tile (eight elements a row) or packed on the float32 tile (four), adds in float32 and rounds each pair of sums back with the pairwise conversion.
template <int DT_ACC, int DT_TILE, int BITS, int G, int NV_ = GroupedQuantTile<DT_TILE, BITS, G>::NV>
__device__ __forceinline__ void grouped_add_term(GroupedRow<DT_ACC, DT_TILE> (&x)[NV_], const uint8_t* stage, const float* s_scale, const float* s_bias,
                                                 const int32_t* s_zp, int lane) {
    using T = GroupedQuantTile<DT_TILE, BITS, G>;
    constexpr int EPV = T::EPV, NV = T::NV, RPG = T::RPG, SETS = T::SETS;
    static_assert(DT_ACC == DT_TILE || (DT_ACC == DT_BF16 && DT_TILE == DT_F32), "the accumulator on its own tile, or bfloat16 packed on the float32 tile");
    DequantParams p[SETS];
    grouped_term_dequant_params<T>(p, s_scale, s_bias, s_zp, lane);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        float f[EPV];
        grouped_dequantize_row<DT_TILE, BITS, G, DequantForm<BITS, DT_ACC>::value>(stage, r, lane, p[r / RPG], f);
        if constexpr (DT_ACC == DT_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[r][e] = __float_as_uint(__fadd_rn(f[e], __uint_as_float(x[r][e])));
        } else {
#pragma unroll
            for (int h = 0; h < EPV / 2; ++h)
                x[r][h] = f32x2_to_bf16x2_bits(__fadd_rn(f[2 * h], __uint_as_float(x[r][h] << 16)),
                                               __fadd_rn(f[2 * h + 1], __uint_as_float(x[r][h] & 0xffff0000u)));
        }
    }
}

template <int DT_ACC, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_grouped_kernel(const void* __restrict__ acc, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                               uint8_t* __restrict__ zero_points, int64_t ngroups, QuantParams p0, GroupedTerms terms) {
    using T = GroupedQuantTile<DT_ACC, BITS, G>;
    using L = GroupedTermLoad<DT_ACC, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64, PACK = 8 / BITS;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];
    __shared__ int32_t s_z[WAVES][NG];

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

    u32x4 raw[NV];
    L next;
    if (full && terms.count > 0) next.load(terms.in[0], terms.scales[0], terms.zero_points[0], v0, gj, has_group, lane);
    grouped_load<DT_ACC, NV>(acc, numel, v0, lane, full, raw);
    for (int i = 0; i < terms.count; ++i) {
        if (full) {
            const L cur = next;
            grouped_park_term(cur, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            if (i + 1 < terms.count) next.load(terms.in[i + 1], terms.scales[i + 1], terms.zero_points[i + 1], v0, gj, has_group, lane);
        } else {
            grouped_park_term_partial<T>(terms, i, v0, (numel + PACK - 1) / PACK - v0 * T::OB, gj, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
        }
        wave_lds_sync();
        grouped_add_term<DT_ACC, DT_ACC, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
        wave_lds_sync();
    }
    grouped_quantize_chunk<DT_ACC, BITS, MODE, G, false>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a[wave], s_b[wave]);
}

// ---- The guarded kernels, for buffers that are not 16-byte aligned: one wave per group, element by element, the same bytes.  Correct, not fast.

// What every guarded quantizing kernel does first for its group of `len` elements (<= 4096: 32-bit offsets inside the group; x_of(o) is element
// o of what is quantized): the group's parameters -- read where they are given, else min / max with every element quieted, the wave reduction,
// the f64 epilogue and, from lane 0 and unless `scales` is NULL, the write -- then the group's QuantParams (what is per call comes as the four
// scalars) and DequantParams.  The min / max rounds have wave-uniform trip counts: a lane past the group's end sits the round out.  Every lane's
// loads of the group are complete behind the wave reduction, so a kernel may overwrite what x_of reads.
template <int BITS, class X>
__device__ __forceinline__ void grouped_guarded_params(X&& x_of, int len, int lane, bool given, float* scales, uint8_t* zero_points, int64_t g, float threshold,
                                                       uint32_t seed_lo, uint32_t seed_hi, uint64_t index_base, QuantParams& p, DequantParams& d) {
    float scale;
    int64_t zp;
    if (given) {
        scale = scales[g];
        zp = zero_points[g];
    } else {
        float lo = 3.402823466e+38f, hi = -3.402823466e+38f;   // the scan's identities (minmax_kernels.hpp)
        for (int o0 = 0; o0 < len; o0 += 64) {
            if (o0 + lane < len) {
                const float x = quieted(x_of(o0 + lane));
                lo = __builtin_fminf(lo, x);
                hi = __builtin_fmaxf(hi, x);
            }
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        quant_params_epilogue(float_to_key(lo), float_to_key(-hi), BITS, scale, zp);
        if (lane == 0 && scales != nullptr) {
            scales[g] = scale;
            zero_points[g] = static_cast<uint8_t>(zp);
        }
    }
    p = QuantParams {};
    p.threshold = threshold;
    p.seed_lo = seed_lo;
    p.seed_hi = seed_hi;
    p.index_base = index_base;
    p.inv_scale = __fdiv_rn(1.0f, scale);   // as the host forms 1 / scale for quantize_uniform
    p.zp64 = zp;
    p.zp32 = static_cast<int32_t>(zp);
    d = DequantParams {};
    d.scale = scale;
    d.zp32 = p.zp32;
    d.zp64 = zp;
    d.bias = __fmul_rn(-static_cast<float>(d.zp32), scale);   // as resolved(DequantParams) forms it
}

template <int DT_IN, int BITS, int MODE, bool GIVEN>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_scalar_kernel(const void* __restrict__ in, uint8_t* __restrict__ out, int64_t numel, int64_t group_size, float* __restrict__ scales,
                               uint8_t* __restrict__ zero_points, int64_t ngroups, QuantParams p0) {
    constexpr int PACK = 8 / BITS, QMAX = (1 << BITS) - 1;
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kGroupedBlock / 64);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the group loop is wave-uniform
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * (kGroupedBlock / 64) + wave; g < ngroups; g += waves) {
        const int64_t b = g * group_size, e = b + group_size < numel ? b + group_size : numel;
        QuantParams p;
        DequantParams d;   // not used: nothing is read back here
        grouped_guarded_params<BITS>([&](int o) { return InVec<DT_IN>::load_scalar(in, b + o); }, static_cast<int>(e - b), lane, GIVEN, scales, zero_points, g,
                                     p0.threshold, p0.seed_lo, p0.seed_hi, p0.index_base, p, d);
        for (int64_t by = b / PACK + lane; by < (e + PACK - 1) / PACK; by += 64) {
            uint32_t acc = 0;
            for (int k = 0; k < PACK; ++k) {
                const int64_t i = by * PACK + k;
                if (i >= numel) break;
                acc |= quant_one<MODE, QMAX>(InVec<DT_IN>::load_scalar(in, i), p, static_cast<uint64_t>(i)) << (k * BITS);
            }
            out[by] = static_cast<uint8_t>(acc);
        }
    }
}

template <int BITS, int DT_OUT>
struct GroupedDequantTile {
    static constexpr int PACK = 8 / BITS;
    static constexpr int EPV = DT_OUT == DT_F32 ? 4 : 8;           // elements per 16-byte output vector
    static constexpr int IB = EPV * BITS / 8;                       // packed bytes per output vector
    static constexpr int NIN = 2;                                   // 16-byte input rows per lane
    static constexpr int CHUNK_BYTES = NIN * 64 * 16;
    static constexpr int CHUNK_ELEMS = CHUNK_BYTES * PACK;
    static constexpr int OV = NIN * 16 / IB;                        // output vectors per lane
};

template <int BITS, int DT_OUT, int G>
struct GroupedDequantSlots {
    static constexpr int value = GroupedDequantTile<BITS, DT_OUT>::CHUNK_ELEMS >= G ? GroupedDequantTile<BITS, DT_OUT>::CHUNK_ELEMS / G : 1;
};

// Dequantize of the chunk that starts at element e0 (< numel); s_in / s_scale / s_bias / s_zp: the wave's LDS slices
template <int BITS, int DT_OUT, int OP, int G>
__device__ __forceinline__ void grouped_dequantize_chunk(const uint8_t* __restrict__ in, void* __restrict__ out, int64_t numel, const float* __restrict__ scales,
                                                         const uint8_t* __restrict__ zero_points, int64_t ngroups, int64_t e0, int lane, uint8_t* s_in,
                                                         float* s_scale, float* s_bias, int32_t* s_zp) {
    using T = GroupedDequantTile<BITS, DT_OUT>;
    constexpr int EPV = T::EPV, IB = T::IB, PACK = T::PACK;
    constexpr int NGD = GroupedDequantSlots<BITS, DT_OUT, G>::value;   // groups per chunk (chunk and group sizes are powers of two)
    constexpr int FORM = DequantForm<BITS, DT_OUT>::value;
    const bool full = e0 + T::CHUNK_ELEMS <= numel;                 // wave-uniform
    const int64_t b0 = e0 / PACK, nbytes = (numel + PACK - 1) / PACK;

    u32x4 raw[T::NIN];
#pragma unroll
    for (int k = 0; k < T::NIN; ++k) {
        const int64_t off = b0 + (k * 64 + lane) * 16;
        if (full) {
            raw[k] = ld<true>(reinterpret_cast<const u32x4*>(in + off));
        } else {
            raw[k] = u32x4 {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (off + j < nbytes) raw[k][j >> 2] |= static_cast<uint32_t>(in[off + j]) << ((j & 3) * 8);
        }
    }
    const int64_t gfirst = e0 / G;
    for (int j = lane; j < NGD; j += 64) {
        if (gfirst + j < ngroups) {
            const float scale = scales[gfirst + j];
            const int32_t zp = zero_points[gfirst + j];
            s_scale[j] = scale;
            s_bias[j] = __fmul_rn(-static_cast<float>(zp), scale);   // as resolved(DequantParams) forms it
            s_zp[j] = zp;
        }
    }
#pragma unroll
    for (int k = 0; k < T::NIN; ++k) reinterpret_cast<u32x4*>(s_in)[k * 64 + lane] = raw[k];
    wave_lds_sync();

    u32x4* out16 = reinterpret_cast<u32x4*>(static_cast<uint8_t*>(out) + e0 * (DT_OUT == DT_F32 ? 4 : 2));
#pragma unroll
    for (int k = 0; k < T::OV; ++k) {
        const int c = k * 64 + lane;                                // output vector of the chunk
        const int ce = c * EPV;                                     // its first element, relative to e0
        if (!full && e0 + ce >= numel) continue;
        const int slot = NGD > 1 ? ce / G : 0;
        DequantParams p {};
        p.scale = s_scale[slot];
        p.bias = s_bias[slot];
        p.zp32 = s_zp[slot];
        p.zp64 = p.zp32;
        uint32_t w[IB > 4 ? 2 : 1];
        staged_words<IB>(s_in + c * IB, w);
        float f[EPV];   // the loop is written out: through grouped_dequantize_row several instances of these kernels compiled to other code
#pragma unroll
        for (int e = 0; e < EPV; ++e) f[e] = dequant_one<FORM>((w[(e * BITS) >> 5] >> ((e * BITS) & 31)) & ((1u << BITS) - 1u), p);
        if (full || e0 + ce + EPV <= numel) {
            u32x4 r;
            u32x4 old {};
            if constexpr (OP == OP_ADD) old = ld<false>(out16 + c);
            if constexpr (DT_OUT == DT_F32) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (OP == OP_ADD) f[e] = __fadd_rn(f[e], __uint_as_float(old[e]));
                    r[e] = __float_as_uint(f[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (OP == OP_ADD) {
                        f[2 * e] = __fadd_rn(f[2 * e], __uint_as_float(old[e] << 16));
                        f[2 * e + 1] = __fadd_rn(f[2 * e + 1], __uint_as_float(old[e] & 0xffff0000u));
                    }
                    r[e] = f32x2_to_bf16x2_bits(f[2 * e], f[2 * e + 1]);
                }
            }
            st<ST_WT>(out16 + c, r);
        } else {   // the tensor ends inside this vector
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                const int64_t i = e0 + ce + e;
                if (i >= numel) continue;
                if constexpr (DT_OUT == DT_F32) {
                    float* o = static_cast<float*>(out);
                    o[i] = OP == OP_ADD ? __fadd_rn(f[e], o[i]) : f[e];
                } else {
                    uint16_t* o = static_cast<uint16_t*>(out);
                    o[i] = static_cast<uint16_t>(f32_to_bf16_bits(OP == OP_ADD ? __fadd_rn(f[e], bf16_bits_to_f32(o[i])) : f[e]));
                }
            }
        }
    }
}

template <int BITS, int DT_OUT, int OP, int G>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_grouped_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, int64_t numel, const float* __restrict__ scales,
                          const uint8_t* __restrict__ zero_points, int64_t ngroups) {
    using T = GroupedDequantTile<BITS, DT_OUT>;
    constexpr int WAVES = kGroupedBlock / 64, NGD = GroupedDequantSlots<BITS, DT_OUT, G>::value;
    __shared__ __attribute__((aligned(16))) uint8_t s_in[WAVES][T::CHUNK_BYTES];
    __shared__ float s_scale[WAVES][NGD], s_bias[WAVES][NGD];
    __shared__ int32_t s_zp[WAVES][NGD];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t e0 = chunk * T::CHUNK_ELEMS;
    if (e0 >= numel) return;
    grouped_dequantize_chunk<BITS, DT_OUT, OP, G>(in, out, numel, scales, zero_points, ngroups, e0, lane, s_in[wave], s_scale[wave], s_bias[wave], s_zp[wave]);
}

// Batch: up to kGroupedBatchMax independent tensors in ONE launch, the chunks of tensor t being [chunk_begin[t], chunk_begin[t + 1]) of the grid's
// waves (as quantize_grouped_batch_kernel)
struct GroupedDequantBatchArgs {
    const uint8_t* in[kGroupedBatchMax];
    void* out[kGroupedBatchMax];
    const float* scales[kGroupedBatchMax];
    const uint8_t* zero_points[kGroupedBatchMax];
    int64_t numel[kGroupedBatchMax];
    int64_t chunk_begin[kGroupedBatchMax + 1];
    int count;
};

template <int BITS, int DT_OUT, int OP, int G>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_grouped_batch_kernel(GroupedDequantBatchArgs a) {
    using T = GroupedDequantTile<BITS, DT_OUT>;
    constexpr int WAVES = kGroupedBlock / 64, NGD = GroupedDequantSlots<BITS, DT_OUT, G>::value;
    __shared__ __attribute__((aligned(16))) uint8_t s_in[WAVES][T::CHUNK_BYTES];
    __shared__ float s_scale[WAVES][NGD], s_bias[WAVES][NGD];
    __shared__ int32_t s_zp[WAVES][NGD];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    grouped_dequantize_chunk<BITS, DT_OUT, OP, G>(a.in[t], a.out[t], numel, a.scales[t], a.zero_points[t], (numel + G - 1) / G,
                                                  (c - a.chunk_begin[t]) * T::CHUNK_ELEMS, lane, s_in[wave], s_scale[wave], s_bias[wave], s_zp[wave]);
}

// Guarded form for buffers that are not 16-byte aligned: element by element.
template <int BITS, int DT_OUT, int OP>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_grouped_scalar_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, int64_t numel, int64_t group_size, const float* __restrict__ scales,
                                 const uint8_t* __restrict__ zero_points) {
    constexpr int FORM = DequantForm<BITS, DT_OUT>::value;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kGroupedBlock;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupedBlock + threadIdx.x; i < numel; i += stride) {
        const int64_t g = i / group_size;
        DequantParams p {};
        p.scale = scales[g];
        p.zp32 = zero_points[g];
        p.zp64 = p.zp32;
        p.bias = __fmul_rn(-static_cast<float>(p.zp32), p.scale);
        const int64_t bit = i * BITS;
        const float f = dequant_one<FORM>((in[bit >> 3] >> (bit & 7)) & ((1u << BITS) - 1u), p);
        if constexpr (DT_OUT == DT_F32) {
            float* o = static_cast<float*>(out);
            o[i] = OP == OP_ADD ? __fadd_rn(f, o[i]) : f;
        } else {
            uint16_t* o = static_cast<uint16_t*>(out);
            o[i] = static_cast<uint16_t>(f32_to_bf16_bits(OP == OP_ADD ? __fadd_rn(f, bf16_bits_to_f32(o[i])) : f));
        }
    }
}

// ---- Error feedback (piquant_hip_quantize_grouped_ef): y = x + r rounded to the tensor's type, (q, scales, zero_points) = quantize_grouped(y),
// r <- y - dequantize_grouped(q) rounded to the tensor's type, in ONE launch.  The wave loads its NV rows of x and of r (all loads issued before
// the first add), forms y in the resident rows, runs the quantize chunk body (KEEP), then reads its own packed words back from the wave's LDS
// slice, dequantizes them with its groups' parameters in the pair's own form (the value a grouped dequantize SET stores: for bf16 rounded to
// bf16 BEFORE the subtraction), subtracts with a separately rounded __fsub_rn and stores the residual rows with 16-byte write-through stores.
// No scan, no atomics, no grid barrier; waves never wait for one another.

// raw[r] = rn(raw[r] + res[r]) element by element in the tensor's type
template <int DT, int NV>
__device__ __forceinline__ void grouped_add_residual(u32x4 (&raw)[NV], const u32x4 (&res)[NV]) {
#pragma unroll
    for (int r = 0; r < NV; ++r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (DT == DT_F32) {
                raw[r][e] = __float_as_uint(__fadd_rn(__uint_as_float(raw[r][e]), __uint_as_float(res[r][e])));
            } else {
                raw[r][e] = f32x2_to_bf16x2_bits(__fadd_rn(__uint_as_float(raw[r][e] << 16), __uint_as_float(res[r][e] << 16)),
                                                 __fadd_rn(__uint_as_float(raw[r][e] & 0xffff0000u), __uint_as_float(res[r][e] & 0xffff0000u)));
            }
        }
    }
}

// y - d of one element in the tensor's type: d is what a dequantize SET stores (bf16: rounded first), the difference is rounded once more
template <int DT>
__device__ __forceinline__ float residual_one(float y, float d) {
    if constexpr (DT == DT_BF16) d = bf16_bits_to_f32(f32_to_bf16_bits(d));
    return __fsub_rn(y, d);
}

// ---- Reading a chunk back (grouped_quantize_chunk with KEEP): shared by the residual store below and the quantize-dequantize store
// (kernels_grouped_requant.hip).

// the dequantize parameters of the lane's SETS groups from what the chunk body parked: s_scale their scales, s_zp their zero points (as float bits)
template <int DT, int BITS, int G, int SETS>
__device__ __forceinline__ void grouped_parked_dequant_params(DequantParams (&p)[SETS], const float* s_scale, const float* s_zp, int lane) {
    using T = GroupedQuantTile<DT, BITS, G>;
    static_assert(SETS == T::SETS, "one entry per group of the lane");
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
        const int slot = s * T::GPR + lane / T::LPG;
        p[s] = DequantParams {};
        p[s].scale = s_scale[slot];
        p[s].zp32 = __float_as_int(s_zp[slot]);
        p[s].zp64 = p[s].zp32;
        p[s].bias = __fmul_rn(-static_cast<float>(p[s].zp32), p[s].scale);   // as resolved(DequantParams) forms it
    }
}

// vector `vec` of a tensor of type DT and numel elements <- o: one 16-byte write-through store, or element by element where the tensor ends inside
// the vector (nothing at or past numel is written).  grouped_residual_store keeps this step written out in its loop: called through here, the
// partial-chunk tail of the bfloat16 error-feedback kernels compiled to differently arranged branches, and those kernels stay instruction for
// instruction what they were.
template <int DT>
__device__ __forceinline__ void grouped_store_vector(void* __restrict__ dst, int64_t numel, int64_t vec, bool full, const u32x4& o) {
    constexpr int EPV = InVec<DT>::EPV;
    if (full || (vec + 1) * EPV <= numel) {
        st<ST_WT>(static_cast<u32x4*>(dst) + vec, o);
    } else {   // the tensor ends inside this vector, or in front of it
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            const int64_t i = vec * EPV + e;
            if (i >= numel) continue;
            if constexpr (DT == DT_F32) static_cast<uint32_t*>(dst)[i] = o[e];
            else static_cast<uint16_t*>(dst)[i] = static_cast<uint16_t>(o[e >> 1] >> ((e & 1) * 16));
        }
    }
}

// raw[r] <- y - dequantize(the chunk's packed bytes in `stage`), then the residual rows to memory (elements at or past numel are not written)
template <int DT, int BITS, int G, int NV_ = GroupedQuantTile<DT, BITS, G>::NV>
__device__ __forceinline__ void grouped_residual_store(u32x4 (&raw)[NV_], void* __restrict__ residual, int64_t numel, int64_t v0, bool full, int lane,
                                                       const uint8_t* stage, const float* s_scale, const float* s_zp) {
    using T = GroupedQuantTile<DT, BITS, G>;
    constexpr int EPV = T::EPV, NV = T::NV, RPG = T::RPG, SETS = T::SETS;
    DequantParams p[SETS];
    grouped_parked_dequant_params<DT, BITS, G>(p, s_scale, s_zp, lane);
    u32x4* r16 = static_cast<u32x4*>(residual);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        float f[EPV];
        grouped_dequantize_row<DT, BITS, G>(stage, r, lane, p[r / RPG], f);
        u32x4 o;
        if constexpr (DT == DT_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = __float_as_uint(residual_one<DT>(__uint_as_float(raw[r][e]), f[e]));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = f32x2_to_bf16x2_bits(residual_one<DT>(__uint_as_float(raw[r][e] << 16), f[2 * e]),
                                            residual_one<DT>(__uint_as_float(raw[r][e] & 0xffff0000u), f[2 * e + 1]));
        }
        const int64_t vec = v0 + r * 64 + lane;
        if (full || (vec + 1) * EPV <= numel) {
            st<ST_WT>(r16 + vec, o);
        } else {   // the tensor ends inside this vector, or in front of it
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                const int64_t i = vec * EPV + e;
                if (i >= numel) continue;
                if constexpr (DT == DT_F32) static_cast<uint32_t*>(residual)[i] = o[e];
                else static_cast<uint16_t*>(residual)[i] = static_cast<uint16_t>(o[e >> 1] >> ((e & 1) * 16));
            }
        }
    }
}

// One wave's chunk (NG groups from group g0 on) of one (tensor, residual) pair; the wave's LDS slices as in grouped_quantize_chunk plus s_c (NG
// floats).  DT_RES, the residual's type, is the pipeline's: it picks the tile, the quantize body and the dequantize form of the subtraction.  The
// tensor has that type too, or is bfloat16 beside a float32 residual: then the bytes are those of the float32 pipeline on widen(x), and x is only
// ever read.  Every load of x and of the residual is issued before the first use.
template <int DT_IN, int DT_RES, int BITS, int MODE, int G>
__device__ __forceinline__ void grouped_ef_chunk(const void* __restrict__ in, void* residual, uint8_t* __restrict__ out, int64_t numel,
                                                 float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, const QuantParams& p0,
                                                 int64_t g0, int lane, uint8_t* stage, float* s_a, float* s_b, float* s_c) {
    using T = GroupedQuantTile<DT_RES, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG;
    const int64_t v0 = g0 * T::V;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform

    u32x4 raw[NV];
    if constexpr (DT_IN == DT_RES) {
        u32x4 res[NV];
        grouped_load<DT_RES, NV>(in, numel, v0, lane, full, raw);
        grouped_load<DT_RES, NV>(residual, numel, v0, lane, full, res);
        grouped_add_residual<DT_RES, NV>(raw, res);
    } else {
        u32x2 t[NV];
        u32x4 res[NV];
        grouped_load_bf16x4<NV>(in, numel, v0, lane, full, t);
        grouped_load<DT_RES, NV>(residual, numel, v0, lane, full, res);
        grouped_widen_bf16x4<NV>(t, raw);
        grouped_add_residual<DT_RES, NV>(raw, res);
    }
    grouped_quantize_chunk<DT_RES, BITS, MODE, G, false, NV, true>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a, s_b, s_c);
    grouped_residual_store<DT_RES, BITS, G>(raw, residual, numel, v0, full, lane, stage, s_c, s_b);
}

template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_ef_kernel(const void* __restrict__ in, void* residual, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                           uint8_t* __restrict__ zero_points, int64_t ngroups, QuantParams p0) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];   // {min, max}, then {1/scale, zero point, scale} of the chunk's groups

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    grouped_ef_chunk<DT_IN, DT_IN, BITS, MODE, G>(in, residual, out, numel, scales, zero_points, ngroups, p0, g0, lane, s_out[wave], s_a[wave], s_b[wave],
                                                  s_c[wave]);
}

// Up to kGroupedBatchMax independent (tensor, residual) pairs in ONE launch, found through the prefix table of quantize_grouped_batch_kernel.
struct GroupedEfBatchArgs {
    const void* in[kGroupedBatchMax];
    void* residual[kGroupedBatchMax];
    uint8_t* out[kGroupedBatchMax];
    float* scales[kGroupedBatchMax];
    uint8_t* zero_points[kGroupedBatchMax];
    int64_t numel[kGroupedBatchMax];
    int64_t chunk_begin[kGroupedBatchMax + 1];
    int count;
};

template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_ef_batch_kernel(GroupedEfBatchArgs a, QuantParams p0) {
    using T = GroupedQuantTile<DT_IN, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    grouped_ef_chunk<DT_IN, DT_IN, BITS, MODE, G>(a.in[t], a.residual[t], a.out[t], numel, a.scales[t], a.zero_points[t], (numel + G - 1) / G, p0,
                                                  (c - a.chunk_begin[t]) * NG, lane, s_out[wave], s_a[wave], s_b[wave], s_c[wave]);
}

// ---- Error feedback on a re-quantized partial sum (piquant_hip_reduce_quantize_grouped_ef): the owner's step of a mesh all-reduce and every hop of
// a ring, compensated.  y = rn(rn(..rn(acc + d(term_0)).. + d(term_{k-1})) + residual), (q, scales, zero_points) = quantize_grouped(y),
// residual <- rn(y - d(q)), in ONE launch: the bytes of k grouped dequantize ADD calls into acc followed by quantize_grouped_ef(acc, residual).
// The tile and the term staging are reduce_quantize_grouped_kernel's, the tail is grouped_ef_chunk's.  The last term is peeled out of the loop so
// that the residual rows need not be live across it: their loads are issued right after the last term has been parked in LDS, where they fly
// during that term's dequantize and add (loading them with the acc rows lost: profiles/EXPERIMENTS.md has the comparison, DESIGN.md 4c the
// choice).  No scan, no atomics, no grid barrier; waves never wait for one another.
template <int DT_ACC, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_grouped_ef_kernel(const void* __restrict__ acc, void* residual, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                  uint8_t* __restrict__ zero_points, int64_t ngroups, QuantParams p0, GroupedTerms terms) {
    using T = GroupedQuantTile<DT_ACC, BITS, G>;
    using L = GroupedTermLoad<DT_ACC, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64, PACK = 8 / BITS;
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

    u32x4 raw[NV], res[NV];
    if (full) {
        L next;
        if (count > 0) next.load(terms.in[0], terms.scales[0], terms.zero_points[0], v0, gj, has_group, lane);
        grouped_load<DT_ACC, NV>(acc, numel, v0, lane, true, raw);
        if (count == 0) grouped_load<DT_ACC, NV>(residual, numel, v0, lane, true, res);
        for (int i = 0; i + 1 < count; ++i) {
            const L cur = next;
            grouped_park_term(cur, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            next.load(terms.in[i + 1], terms.scales[i + 1], terms.zero_points[i + 1], v0, gj, has_group, lane);
            wave_lds_sync();
            grouped_add_term<DT_ACC, DT_ACC, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
            wave_lds_sync();
        }
        if (count > 0) {   // the last term: nothing left to prefetch but the residual
            grouped_park_term(next, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            grouped_load<DT_ACC, NV>(residual, numel, v0, lane, true, res);
            wave_lds_sync();
            grouped_add_term<DT_ACC, DT_ACC, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
            wave_lds_sync();
        }
    } else {
        // the tensor ends inside this chunk: acc and residual read as quiet NaNs behind it, a term byte by byte up to its last byte (zeros behind it)
        grouped_load<DT_ACC, NV>(acc, numel, v0, lane, false, raw);
        grouped_load<DT_ACC, NV>(residual, numel, v0, lane, false, res);
        const int64_t left = (numel + PACK - 1) / PACK - v0 * T::OB;
        for (int i = 0; i < count; ++i) {
            grouped_park_term_partial<T>(terms, i, v0, left, gj, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            wave_lds_sync();
            grouped_add_term<DT_ACC, DT_ACC, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
            wave_lds_sync();
        }
    }
    grouped_add_residual<DT_ACC, NV>(raw, res);
    grouped_quantize_chunk<DT_ACC, BITS, MODE, G, false, NV, true>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a[wave], s_b[wave],
                                                                   s_c[wave]);
    grouped_residual_store<DT_ACC, BITS, G>(raw, residual, numel, v0, full, lane, stage, s_c[wave], s_b[wave]);
}

// Guarded form (grouped_guarded_params) of both error-feedback quantizes: the tensor of type DT_IN, the residual -- and with it the pipeline -- of
// type DT_RES.  y = rn(x + r) in DT_RES is formed twice, for the min / max pass and for the quantization; the residual is overwritten in between
// by nobody: its stores come behind the wave reduction.
template <int DT_IN, int DT_RES, int BITS, int MODE>
__device__ __forceinline__ void grouped_ef_guarded(const void* in, void* residual, uint8_t* out, int64_t numel, int64_t group_size, float* scales,
                                                   uint8_t* zero_points, int64_t ngroups, float threshold, uint32_t seed_lo, uint32_t seed_hi,
                                                   uint64_t index_base) {
    constexpr int PACK = 8 / BITS, QMAX = (1 << BITS) - 1, FORM = DequantForm<BITS, DT_RES>::value;
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kGroupedBlock / 64);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the group loop is wave-uniform
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * (kGroupedBlock / 64) + wave; g < ngroups; g += waves) {
        const int64_t b = g * group_size;
        const int len = static_cast<int>(b + group_size < numel ? group_size : numel - b);
        auto y_of = [&](int o) {
            const float y = __fadd_rn(InVec<DT_IN>::load_scalar(in, b + o), InVec<DT_RES>::load_scalar(residual, b + o));
            if constexpr (DT_RES == DT_BF16) return bf16_bits_to_f32(f32_to_bf16_bits(y));
            else return y;
        };
        QuantParams p;
        DequantParams d;
        grouped_guarded_params<BITS>(y_of, len, lane, false, scales, zero_points, g, threshold, seed_lo, seed_hi, index_base, p, d);
        uint8_t* og = out + b / PACK;   // a group starts on a whole packed byte
        for (int by0 = 0; by0 * PACK < len; by0 += 64) {
            const int by = by0 + lane;
            if (by * PACK >= len) continue;
            uint32_t acc = 0;
#pragma unroll
            for (int k = 0; k < PACK; ++k) {
                const int o = by * PACK + k;
                if (o >= len) continue;
                const float y = y_of(o);
                const uint32_t q = quant_one<MODE, QMAX>(y, p, static_cast<uint64_t>(b + o));
                acc |= q << (k * BITS);
                const float nr = residual_one<DT_RES>(y, dequant_one<FORM>(q, d));
                if constexpr (DT_RES == DT_F32) static_cast<float*>(residual)[b + o] = nr;
                else static_cast<uint16_t*>(residual)[b + o] = static_cast<uint16_t>(f32_to_bf16_bits(nr));
            }
            og[by] = static_cast<uint8_t>(acc);
        }
    }
}

template <int DT_IN, int BITS, int MODE>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_ef_scalar_kernel(const void* __restrict__ in, void* residual, uint8_t* __restrict__ out, int64_t numel, int64_t group_size,
                                  float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, float threshold, uint32_t seed_lo,
                                  uint32_t seed_hi, uint64_t index_base) {
    grouped_ef_guarded<DT_IN, DT_IN, BITS, MODE>(in, residual, out, numel, group_size, scales, zero_points, ngroups, threshold, seed_lo, seed_hi, index_base);
}

// ---- Error feedback with a float32 residual for a bfloat16 tensor (piquant_hip_quantize_grouped_ef_mixed): the bytes of
// quantize_grouped_ef(widen(x), residual) in the float32 pipeline, without the widened copy of x ever reaching memory.  The tile is the float32
// one, GroupedQuantTile<DT_F32, BITS, G>: a lane-row is four elements, which of x are 8 bytes (one global_load_dwordx2, 512 contiguous bytes per
// wave-row) widened into raw[r][e] = bits << 16, and of the residual one 16-byte vector.  That is the second branch of grouped_ef_chunk
// (DT_IN = bfloat16, DT_RES = float32); behind it the function goes on as for a float32 tensor: y = rn_f32(widen(x) + r), the float32 quantize
// chunk body (KEEP), r <- rn_f32(y - d) with d the float32 dequantize form.  x is never written.

template <int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_ef_f32r_kernel(const void* __restrict__ in, void* residual, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                uint8_t* __restrict__ zero_points, int64_t ngroups, QuantParams p0) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];   // {min, max}, then {1/scale, zero point, scale} of the chunk's groups

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    grouped_ef_chunk<DT_BF16, DT_F32, BITS, MODE, G>(in, residual, out, numel, scales, zero_points, ngroups, p0, g0, lane, s_out[wave], s_a[wave], s_b[wave],
                                                     s_c[wave]);
}

// up to kGroupedBatchMax independent pairs in ONE launch, found through the prefix table of quantize_grouped_batch_kernel
template <int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_ef_f32r_batch_kernel(GroupedEfBatchArgs a, QuantParams p0) {
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
    grouped_ef_chunk<DT_BF16, DT_F32, BITS, MODE, G>(a.in[t], a.residual[t], a.out[t], numel, a.scales[t], a.zero_points[t], (numel + G - 1) / G, p0,
                                                     (c - a.chunk_begin[t]) * NG, lane, s_out[wave], s_a[wave], s_b[wave], s_c[wave]);
}

// the guarded form, for buffers of any (element) alignment
template <int BITS, int MODE>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_ef_f32r_scalar_kernel(const void* __restrict__ in, void* residual, uint8_t* __restrict__ out, int64_t numel, int64_t group_size,
                                       float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, float threshold, uint32_t seed_lo,
                                       uint32_t seed_hi, uint64_t index_base) {
    grouped_ef_guarded<DT_BF16, DT_F32, BITS, MODE>(in, residual, out, numel, group_size, scales, zero_points, ngroups, threshold, seed_lo, seed_hi, index_base);
}

// ---- The two fused: error feedback on a re-quantized partial sum of a bfloat16 accumulator with a float32 residual
// (piquant_hip_reduce_quantize_grouped_ef_mixed).  reduce_quantize_grouped_ef_kernel on the float32 tile, in three places different: the
// accumulator rows stay PACKED (u32x2: two bfloat16 a dword, 2 NV registers instead of 4 NV) through the term loop -- every add rounds back to
// bfloat16 anyway --, grouped_add_term adds in the uint -> bfloat16 form, and the rows are widened once behind the last term.  The bytes are
// those of k grouped dequantize ADD calls into the bfloat16 acc followed by the mixed quantize above.  The two kernels are written out side by
// side: as one body under two thin kernels every probed instance of both compiled to other code (profiles/EXPERIMENTS.md).
template <int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_grouped_ef_f32r_kernel(const void* __restrict__ acc, void* residual, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                       uint8_t* __restrict__ zero_points, int64_t ngroups, QuantParams p0, GroupedTerms terms) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    using L = GroupedTermLoad<DT_F32, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64, PACK = 8 / BITS;
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

    u32x2 t[NV];
    u32x4 raw[NV], res[NV];
    if (full) {
        L next;
        if (count > 0) next.load(terms.in[0], terms.scales[0], terms.zero_points[0], v0, gj, has_group, lane);
        grouped_load_bf16x4<NV>(acc, numel, v0, lane, true, t);
        if (count == 0) grouped_load<DT_F32, NV>(residual, numel, v0, lane, true, res);
        for (int i = 0; i + 1 < count; ++i) {
            const L cur = next;
            grouped_park_term(cur, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            next.load(terms.in[i + 1], terms.scales[i + 1], terms.zero_points[i + 1], v0, gj, has_group, lane);
            wave_lds_sync();
            grouped_add_term<DT_BF16, DT_F32, BITS, G>(t, stage, s_a[wave], s_b[wave], s_z[wave], lane);
            wave_lds_sync();
        }
        if (count > 0) {   // the last term: nothing left to prefetch but the residual
            grouped_park_term(next, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            grouped_load<DT_F32, NV>(residual, numel, v0, lane, true, res);
            wave_lds_sync();
            grouped_add_term<DT_BF16, DT_F32, BITS, G>(t, stage, s_a[wave], s_b[wave], s_z[wave], lane);
            wave_lds_sync();
        }
    } else {
        // the tensor ends inside this chunk: acc and residual read as quiet NaNs behind it, a term byte by byte up to its last byte (zeros behind it)
        grouped_load_bf16x4<NV>(acc, numel, v0, lane, false, t);
        grouped_load<DT_F32, NV>(residual, numel, v0, lane, false, res);
        const int64_t left = (numel + PACK - 1) / PACK - v0 * T::OB;
        for (int i = 0; i < count; ++i) {
            grouped_park_term_partial<T>(terms, i, v0, left, gj, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            wave_lds_sync();
            grouped_add_term<DT_BF16, DT_F32, BITS, G>(t, stage, s_a[wave], s_b[wave], s_z[wave], lane);
            wave_lds_sync();
        }
    }
    grouped_widen_bf16x4<NV>(t, raw);
    grouped_add_residual<DT_F32, NV>(raw, res);
    grouped_quantize_chunk<DT_F32, BITS, MODE, G, false, NV, true>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a[wave], s_b[wave],
                                                                   s_c[wave]);
    grouped_residual_store<DT_F32, BITS, G>(raw, residual, numel, v0, full, lane, stage, s_c[wave], s_b[wave]);
}

// ---- Dequantize-sum (piquant_hip_dequantize_sum_grouped): out (op)= dequantize_grouped(term_0) + ... + dequantize_grouped(term_{k-1}), the bytes of
// k grouped dequantize calls into out (the first with the call's op, the others ADD: the running sum rounded to out's type after every term) in
// ONE pass over out.  The term loop of reduce_quantize_grouped_kernel on its tile -- the float rows set the chunk's size, not the packed ones --
// with a store of the rows in place of the quantize tail.

// x[r] = the dequantized packed bytes of vector r of the lane in the type DT: what a grouped dequantize SET stores (bfloat16: rounded once).  The
// first term of a SET is stored, not added to rows of +0.0: -0.0 + 0.0 is +0.0, and a NaN would take the adder's path instead of the converter's.
template <int DT, int BITS, int G, int NV_ = GroupedQuantTile<DT, BITS, G>::NV>
__device__ __forceinline__ void grouped_set_term(u32x4 (&x)[NV_], const uint8_t* stage, const float* s_scale, const float* s_bias, const int32_t* s_zp,
                                                 int lane) {
    using T = GroupedQuantTile<DT, BITS, G>;
    constexpr int EPV = T::EPV, NV = T::NV, RPG = T::RPG, SETS = T::SETS;
    DequantParams p[SETS];
    grouped_term_dequant_params<T>(p, s_scale, s_bias, s_zp, lane);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        float f[EPV];
        grouped_dequantize_row<DT, BITS, G>(stage, r, lane, p[r / RPG], f);
        if constexpr (DT == DT_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[r][e] = __float_as_uint(f[e]);
        } else {
#pragma unroll
            for (int h = 0; h < EPV / 2; ++h) x[r][h] = f32x2_to_bf16x2_bits(f[2 * h], f[2 * h + 1]);
        }
    }
}

// One wave per chunk; terms.count >= 1.  ADD loads the rows of out behind the first term's loads; SET never reads out.  Term i + 1 is in flight
// (GroupedTermLoad) while term i is added.  A chunk the tensor ends in stages its terms byte by byte (grouped_park_term_partial) and stores through
// grouped_store_vector: nothing at or past numel is read or written in any buffer.  No scan, no atomics, no grid barrier.
template <int DT_OUT, int BITS, int OP, int G>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_sum_grouped_kernel(void* __restrict__ out, int64_t numel, int64_t ngroups, GroupedTerms terms) {
    using T = GroupedQuantTile<DT_OUT, BITS, G>;
    using L = GroupedTermLoad<DT_OUT, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64, PACK = 8 / BITS;
    __shared__ __attribute__((aligned(16))) uint8_t s_in[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];   // a term's {scale, bias}
    __shared__ int32_t s_z[WAVES][NG];                 // a term's zero point

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    const int64_t v0 = g0 * T::V;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform
    const int64_t gj = g0 + lane;
    const bool has_group = lane < NG && gj < ngroups;
    uint8_t* stage = s_in[wave];
    const int count = terms.count;

    u32x4 raw[NV];
    L next;
    if (full) next.load(terms.in[0], terms.scales[0], terms.zero_points[0], v0, gj, has_group, lane);
    if constexpr (OP == OP_ADD) grouped_load<DT_OUT, NV>(out, numel, v0, lane, full, raw);
    // term i into the wave's LDS slices, term i + 1 into flight
    auto stage_term = [&](int i) {
        if (full) {
            const L cur = next;
            grouped_park_term(cur, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
            if (i + 1 < count) next.load(terms.in[i + 1], terms.scales[i + 1], terms.zero_points[i + 1], v0, gj, has_group, lane);
        } else {
            grouped_park_term_partial<T>(terms, i, v0, (numel + PACK - 1) / PACK - v0 * T::OB, gj, stage, s_a[wave], s_b[wave], s_z[wave], has_group, lane);
        }
        wave_lds_sync();
    };
    int i = 0;
    if constexpr (OP == OP_SET) {   // the first term of a SET is peeled: the loop holds the add alone
        stage_term(0);
        grouped_set_term<DT_OUT, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
        wave_lds_sync();
        i = 1;
    }
    for (; i < count; ++i) {
        stage_term(i);
        grouped_add_term<DT_OUT, DT_OUT, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
        wave_lds_sync();
    }
#pragma unroll
    for (int r = 0; r < NV; ++r) grouped_store_vector<DT_OUT>(out, numel, v0 + r * 64 + lane, full, raw[r]);
}

}  // namespace pq
