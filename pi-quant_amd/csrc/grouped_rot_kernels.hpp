// Randomized Hadamard rotation of the groups of group-wise quantization (include/piquant_hip.h, piquant_hip_hadamard_grouped).
//
// The rotation of group size G = 2^k with a 64-bit seed acts on float32 values, one FULL group at a time:
//   signs       d[j] = -1 where bit (j mod 16) of floor(element_threshold(seed, j div 16) * 2^24) is set, else +1 -- a function of the position
//               inside the group only, so every group, shard and chunk that starts on a group boundary uses the same d
//   butterflies fwht(v): for h = 1, 2, 4, .., G / 2 in this order, every pair (i, i + h) with bit h of i clear becomes (v[i] + v[i + h],
//               v[i] - v[i + h]), each a separately rounded float32 operation.  The stage order fixes every rounding.
//   constant    c_G = 2^(-k / 2): the exact power of two for even k, float32(sqrt 2) (0x3FB504F3) * 2^(-(k + 1) / 2) for odd k
//   forward     y = c_G * fwht(d * x)           inverse     x = d * (c_G * fwht(y))
// A ragged last group (numel % G != 0; a tensor shorter than G is one) is not rotated.
//
// On the tile: every kernel here sits on the FLOAT32 row layout of GroupedQuantTile (grouped_kernels.hpp) -- a lane-row is four consecutive
// elements, whatever the tensor's type: a bfloat16 tensor is loaded and stored 8 bytes a lane-row (grouped_load_bf16x4) and transformed as
// widened float32.  Position p of a group is element p % 4 of lane (p / 4) % 64 of row p / 256 of the group's rows, so stage h is
//   h = 1, 2            inside the lane's vector: plain VALU
//   h = 4 .. 128        between lanes l and l ^ (h / 4): xor_lane (DPP for 1 and 2, ds_swizzle for 4 .. 16, ds_bpermute for 32); the lane with
//                       the bit clear keeps the sum, the other one the difference partner - self, formed as partner + (-self): the same rounding
//   h = 256 .. G / 2    between rows r and r ^ (h / 256) of the registers one lane holds
// No LDS memory traffic, no block barrier; waves never wait for one another.  One launch reads the tensor once.
#pragma once

#include "grouped_kernels.hpp"

namespace pq {

constexpr int kGroupedRotGuardedBlock = 64;   // the guarded kernels: one wave a block, the group in the block's LDS

// c_G as a float32
template <int G>
struct GroupedRotScale {
    static constexpr int K = __builtin_ctz(G);
    static constexpr float value = ((K & 1) ? 0x1.6a09e6p+0f : 1.0f) / static_cast<float>(1 << ((K + 1) / 2));
};

// the sign word of positions [16 w, 16 w + 16) of a group: floor(element_threshold(seed, w) * 2^24), the counter hash before its conversion
__device__ __forceinline__ uint32_t grouped_rot_sign_word(uint32_t seed_lo, uint32_t seed_hi, uint32_t w) {
    return mix32(w ^ (mix32(seed_hi) + seed_lo)) >> 8;
}

// The rotation of the lane's share of ONE set of the float32 tile: RPG rows of four elements, the group being LPG lanes of them.
template <int G, bool INVERSE>
struct GroupedRot {
    static constexpr int V = G / 4, LPG = V < 64 ? V : 64, RPG = V < 64 ? 1 : V / 64;

    // bit e of nib[rr]: the sign of element e of the lane's vector of row rr of a set (the same for every set and every chunk)
    static __device__ __forceinline__ void signs(uint32_t (&nib)[RPG], int lane, uint32_t seed_lo, uint32_t seed_hi) {
#pragma unroll
        for (int rr = 0; rr < RPG; ++rr) {
            const uint32_t vec = static_cast<uint32_t>(rr * 64 + lane) % static_cast<uint32_t>(V);   // the vector's index in its group
            nib[rr] = (grouped_rot_sign_word(seed_lo, seed_hi, vec >> 2) >> ((vec & 3u) * 4u)) & 0xfu;
        }
    }

    static __device__ __forceinline__ void flip(float (&x)[RPG][4], const uint32_t (&nib)[RPG]) {
#pragma unroll
        for (int rr = 0; rr < RPG; ++rr) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[rr][e] = __uint_as_float(__float_as_uint(x[rr][e]) ^ ((nib[rr] << (31 - e)) & 0x80000000u));
        }
    }

    template <int OFF>
    static __device__ __forceinline__ void lane_stage(float (&x)[RPG][4], int lane) {
        if constexpr (OFF < LPG) {
            const uint32_t neg = (lane & OFF) ? 0x80000000u : 0u;
#pragma unroll
            for (int rr = 0; rr < RPG; ++rr) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float partner = xor_lane<OFF>(x[rr][e]);
                    x[rr][e] = __fadd_rn(partner, __uint_as_float(__float_as_uint(x[rr][e]) ^ neg));
                }
            }
        }
    }

    // every lane of the wave calls this together (the lane stages exchange registers)
    static __device__ __forceinline__ void run(float (&x)[RPG][4], const uint32_t (&nib)[RPG], int lane) {
        if constexpr (!INVERSE) flip(x, nib);
#pragma unroll
        for (int rr = 0; rr < RPG; ++rr) {
            const float a0 = __fadd_rn(x[rr][0], x[rr][1]), a1 = __fsub_rn(x[rr][0], x[rr][1]);
            const float a2 = __fadd_rn(x[rr][2], x[rr][3]), a3 = __fsub_rn(x[rr][2], x[rr][3]);
            x[rr][0] = __fadd_rn(a0, a2);
            x[rr][1] = __fadd_rn(a1, a3);
            x[rr][2] = __fsub_rn(a0, a2);
            x[rr][3] = __fsub_rn(a1, a3);
        }
        lane_stage<1>(x, lane);
        lane_stage<2>(x, lane);
        lane_stage<4>(x, lane);
        lane_stage<8>(x, lane);
        lane_stage<16>(x, lane);
        lane_stage<32>(x, lane);
#pragma unroll
        for (int h = 1; h < RPG; h *= 2) {
#pragma unroll
            for (int rr = 0; rr < RPG; ++rr) {
                if (rr & h) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = x[rr][e], b = x[rr + h][e];
                    x[rr][e] = __fadd_rn(a, b);
                    x[rr + h][e] = __fsub_rn(a, b);
                }
            }
        }
#pragma unroll
        for (int rr = 0; rr < RPG; ++rr) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[rr][e] = __fmul_rn(x[rr][e], GroupedRotScale<G>::value);
        }
        if constexpr (INVERSE) flip(x, nib);
    }
};

// whether the group of set s of the lane is a whole group of the tensor (T: the float32 tile); `full`: every group of the chunk is
template <class T, int G>
__device__ __forceinline__ bool grouped_rot_whole(int s, int64_t numel, int64_t g0, bool full, int lane) {
    return full || (g0 + s * T::GPR + lane / T::LPG + 1) * G <= numel;
}

// The float32 rows of one chunk (raw[r][e]: float bits; the chunk starts at group g0) rotated in place, whole groups only.
template <int BITS, int G, bool INVERSE, int NV_ = GroupedQuantTile<DT_F32, BITS, G>::NV>
__device__ __forceinline__ void grouped_rotate_chunk(u32x4 (&raw)[NV_], int64_t numel, int64_t g0, bool full, int lane, uint32_t seed_lo, uint32_t seed_hi) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    using R = GroupedRot<G, INVERSE>;
    constexpr int RPG = T::RPG, SETS = T::SETS;
    static_assert(R::RPG == RPG && R::LPG == T::LPG, "the rotation's rows are the tile's");
    uint32_t nib[RPG];
    R::signs(nib, lane, seed_lo, seed_hi);
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
        float x[RPG][4];
#pragma unroll
        for (int rr = 0; rr < RPG; ++rr) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[rr][e] = __uint_as_float(raw[s * RPG + rr][e]);
        }
        R::run(x, nib, lane);
        const bool whole = grouped_rot_whole<T, G>(s, numel, g0, full, lane);   // a select per register, not a branch around the write-back
#pragma unroll
        for (int rr = 0; rr < RPG; ++rr) {
            const u32x4 y {__float_as_uint(x[rr][0]), __float_as_uint(x[rr][1]), __float_as_uint(x[rr][2]), __float_as_uint(x[rr][3])};
            raw[s * RPG + rr] = whole ? y : raw[s * RPG + rr];
        }
    }
}

// one wave's chunk of a tensor of type DT as float32 rows (elements at or past numel: quiet NaNs); a bfloat16 tensor also leaves its packed rows in t
template <int DT, int NV>
__device__ __forceinline__ void grouped_rot_load(const void* in, int64_t numel, int64_t v0, int lane, bool full, u32x4 (&raw)[NV], u32x2 (&t)[NV]) {
    if constexpr (DT == DT_F32) {
        grouped_load<DT_F32, NV>(in, numel, v0, lane, full, raw);
    } else {
        if (full) {
            grouped_load_bf16x4<NV>(in, numel, v0, lane, true, t);
        } else {   // the tensor ends inside this chunk: a row it ends in is read element by element
#pragma unroll
            for (int r = 0; r < NV; ++r) {
                const int64_t vec = v0 + r * 64 + lane;
                if ((vec + 1) * 4 <= numel) {
                    t[r] = ld<true>(static_cast<const u32x2*>(in) + vec);
                } else {
                    uint32_t h[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[e] = vec * 4 + e < numel ? static_cast<uint32_t>(static_cast<const uint16_t*>(in)[vec * 4 + e]) : 0x7fc0u;
                    t[r] = u32x2 {h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
                }
            }
        }
        grouped_widen_bf16x4<NV>(t, raw);
    }
}

// four bfloat16 (o: two a dword) to lane-row `vec` of a bfloat16 tensor, i.e. elements [4 vec, 4 vec + 4): one 8-byte write-through store, or
// element by element where the tensor ends inside the row (nothing at or past numel is written)
__device__ __forceinline__ void grouped_rot_store_bf16x4(void* dst, int64_t numel, int64_t vec, bool full, const u32x2& o) {
    if (full || (vec + 1) * 4 <= numel) {
        st<ST_WT>(static_cast<u32x2*>(dst) + vec, o);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = vec * 4 + e;
            if (i >= numel) continue;
            static_cast<uint16_t*>(dst)[i] = static_cast<uint16_t>(o[e >> 1] >> ((e & 1) * 16));
        }
    }
}

// ---- hadamard_grouped: out = the forward or inverse rotation of in, same type; out may be in (a wave loads its whole chunk before it stores, and
// chunks are disjoint).  bfloat16: transformed in float32, rounded to bfloat16 on store; a group that is not rotated keeps its bits.
template <int DT, int G, bool INVERSE>
__global__ void __launch_bounds__(kGroupedBlock)
hadamard_grouped_kernel(const void* in, void* out, int64_t numel, int64_t ngroups, uint32_t seed_lo, uint32_t seed_hi) {
    using T = GroupedQuantTile<DT_F32, 8, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    const int64_t v0 = g0 * T::V;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform

    u32x4 raw[NV];
    u32x2 t[NV];
    grouped_rot_load<DT, NV>(in, numel, v0, lane, full, raw, t);
    grouped_rotate_chunk<8, G, INVERSE>(raw, numel, g0, full, lane, seed_lo, seed_hi);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        if constexpr (DT == DT_F32) {
            grouped_store_vector<DT_F32>(out, numel, v0 + r * 64 + lane, full, raw[r]);
        } else {
            u32x2 o {f32x2_to_bf16x2_bits(__uint_as_float(raw[r][0]), __uint_as_float(raw[r][1])),
                     f32x2_to_bf16x2_bits(__uint_as_float(raw[r][2]), __uint_as_float(raw[r][3]))};
            if (!grouped_rot_whole<T, G>(r / T::RPG, numel, g0, full, lane)) o = t[r];
            grouped_rot_store_bf16x4(out, numel, v0 + r * 64 + lane, full, o);
        }
    }
}

// ---- quantize_grouped_rotated: the bytes, scales and zero points of quantize_grouped(y) with computed parameters, y the float32 forward rotation of
// the widened tensor -- the float32 pipeline whatever the tensor's type; y never reaches memory.
// One wave's chunk (NG groups of the float32 tile from group g0 on) of one tensor: the body of the single-tensor kernel and of the batch kernel.
template <int DT_IN, int BITS, int MODE, int G>
__device__ __forceinline__ void grouped_rot_quantize_chunk(const void* __restrict__ in, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                                           uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi,
                                                           const QuantParams& p0, int64_t g0, int lane, uint8_t* stage, float* s_a, float* s_b) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform

    u32x4 raw[NV];
    u32x2 t[NV];
    grouped_rot_load<DT_IN, NV>(in, numel, g0 * T::V, lane, full, raw, t);
    grouped_rotate_chunk<BITS, G, false>(raw, numel, g0, full, lane, rot_lo, rot_hi);
    grouped_quantize_chunk<DT_F32, BITS, MODE, G, false>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a, s_b);
}

template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_rotated_kernel(const void* __restrict__ in, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi, QuantParams p0) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];   // {min, max} of the chunk's groups, then {1/scale, zero point}

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    grouped_rot_quantize_chunk<DT_IN, BITS, MODE, G>(in, out, numel, scales, zero_points, ngroups, rot_lo, rot_hi, p0, g0, lane, s_out[wave], s_a[wave],
                                                     s_b[wave]);
}

// Batch: up to kGroupedBatchMax independent tensors in ONE launch, found through the prefix table of quantize_grouped_batch_kernel.  The table's
// unit is the chunk of the FLOAT32 tile, G * NG elements, whatever the tensors' type; numel, ngroups and the ragged last group are each member's own.
template <int DT_IN, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_grouped_rotated_batch_kernel(GroupedQuantBatchArgs a, uint32_t rot_lo, uint32_t rot_hi, QuantParams p0) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    grouped_rot_quantize_chunk<DT_IN, BITS, MODE, G>(a.in[t], a.out[t], numel, a.scales[t], a.zero_points[t], (numel + G - 1) / G, rot_lo, rot_hi, p0,
                                                     (c - a.chunk_begin[t]) * NG, lane, s_out[wave], s_a[wave], s_b[wave]);
}

// ---- dequantize_grouped_rotated: z = the float32 inverse rotation of dequantize_grouped(in -> float32, SET); out = convert(z) (SET) or
// convert(widen(out) + z) (ADD: one float32 add, one rounding).  The packed chunk arrives as the one term of a dequantize-sum on the float32 tile.
struct GroupedRotTerm {   // what grouped_park_term_partial reads of a term list
    const uint8_t* in[1];
    const float* scales[1];
    const uint8_t* zero_points[1];
};

// One wave's chunk (NG groups of the float32 tile from group g0 on) of one tensor: the body of the single-tensor kernel and of the batch kernel.
template <int DT_OUT, int BITS, int OP, int G>
__device__ __forceinline__ void grouped_rot_dequantize_chunk(const uint8_t* __restrict__ in, void* __restrict__ out, int64_t numel,
                                                             const float* __restrict__ scales, const uint8_t* __restrict__ zero_points, int64_t ngroups,
                                                             uint32_t rot_lo, uint32_t rot_hi, int64_t g0, int lane, uint8_t* stage, float* s_a, float* s_b,
                                                             int32_t* s_z) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    using L = GroupedTermLoad<DT_F32, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, PACK = 8 / BITS;
    const int64_t v0 = g0 * T::V;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform
    const int64_t gj = g0 + lane;
    const bool has_group = lane < NG && gj < ngroups;

    if (full) {
        L term;
        term.load(in, scales, zero_points, v0, gj, has_group, lane);
        grouped_park_term(term, stage, s_a, s_b, s_z, has_group, lane);
    } else {
        const GroupedRotTerm one {{in}, {scales}, {zero_points}};
        grouped_park_term_partial<T>(one, 0, v0, (numel + PACK - 1) / PACK - v0 * T::OB, gj, stage, s_a, s_b, s_z, has_group, lane);
    }
    [[maybe_unused]] u32x4 old[NV];
    [[maybe_unused]] u32x2 told[NV];
    if constexpr (OP == OP_ADD) grouped_rot_load<DT_OUT, NV>(out, numel, v0, lane, full, old, told);
    wave_lds_sync();

    u32x4 raw[NV];
    grouped_set_term<DT_F32, BITS, G>(raw, stage, s_a, s_b, s_z, lane);
    grouped_rotate_chunk<BITS, G, true>(raw, numel, g0, full, lane, rot_lo, rot_hi);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        if constexpr (OP == OP_ADD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) raw[r][e] = __float_as_uint(__fadd_rn(__uint_as_float(raw[r][e]), __uint_as_float(old[r][e])));
        }
        if constexpr (DT_OUT == DT_F32) {
            grouped_store_vector<DT_F32>(out, numel, v0 + r * 64 + lane, full, raw[r]);
        } else {
            const u32x2 o {f32x2_to_bf16x2_bits(__uint_as_float(raw[r][0]), __uint_as_float(raw[r][1])),
                           f32x2_to_bf16x2_bits(__uint_as_float(raw[r][2]), __uint_as_float(raw[r][3]))};
            grouped_rot_store_bf16x4(out, numel, v0 + r * 64 + lane, full, o);
        }
    }
}

template <int DT_OUT, int BITS, int OP, int G>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_grouped_rotated_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, int64_t numel, const float* __restrict__ scales,
                                  const uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_in[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];   // the groups' {scale, bias}
    __shared__ int32_t s_z[WAVES][NG];                 // their zero points

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    grouped_rot_dequantize_chunk<DT_OUT, BITS, OP, G>(in, out, numel, scales, zero_points, ngroups, rot_lo, rot_hi, g0, lane, s_in[wave], s_a[wave],
                                                      s_b[wave], s_z[wave]);
}

// Batch: up to kGroupedBatchMax independent packed tensors in ONE launch, found through the prefix table of quantize_grouped_batch_kernel.  The
// table's unit is again the chunk of the FLOAT32 quantize tile, G * NG elements -- NOT GroupedDequantTile's CHUNK_ELEMS, the unit of
// dequantize_grouped_batch_kernel: this kernel sits on the quantize tile, as the single-tensor one does.
template <int DT_OUT, int BITS, int OP, int G>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_grouped_rotated_batch_kernel(GroupedDequantBatchArgs a, uint32_t rot_lo, uint32_t rot_hi) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_in[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];
    __shared__ int32_t s_z[WAVES][NG];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    grouped_rot_dequantize_chunk<DT_OUT, BITS, OP, G>(a.in[t], a.out[t], numel, a.scales[t], a.zero_points[t], (numel + G - 1) / G, rot_lo, rot_hi,
                                                      (c - a.chunk_begin[t]) * NG, lane, s_in[wave], s_a[wave], s_b[wave], s_z[wave]);
}

// ---- reduce_quantize_grouped_rotated: the bytes, scales and zero points of quantize_grouped(y) with computed parameters, y = the float32 forward
// rotation of the widened accumulator + dequantize_grouped(term_0 -> float32) + ... in order, each term one separately rounded float32 add.  The
// terms are records of rotated values already, so ONE rotation serves the sum: the accumulator's, in front of the adds (it fixes the roundings).
// The term loop is reduce_quantize_grouped_kernel's on the float32 tile: term i + 1 in flight while term i is added, and the first term's loads
// issued in front of the accumulator's, so that the butterflies run under them.  acc is only read; y never reaches memory.
template <int DT_ACC, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
reduce_quantize_grouped_rotated_kernel(const void* __restrict__ acc, uint8_t* __restrict__ out, int64_t numel, float* __restrict__ scales,
                                       uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi, QuantParams p0,
                                       GroupedTerms terms) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    using L = GroupedTermLoad<DT_F32, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG, WAVES = kGroupedBlock / 64, PACK = 8 / BITS;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG];   // a term's {scale, bias}; then {min, max} of the chunk's groups, then {1/scale, zero point}
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
    uint8_t* stage = s_out[wave];
    const int count = terms.count;

    u32x4 raw[NV];
    u32x2 t[NV];
    L next;
    if (full && count > 0) next.load(terms.in[0], terms.scales[0], terms.zero_points[0], v0, gj, has_group, lane);
    grouped_rot_load<DT_ACC, NV>(acc, numel, v0, lane, full, raw, t);
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
    grouped_quantize_chunk<DT_F32, BITS, MODE, G, false>(raw, out, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a[wave], s_b[wave]);
}

// ---- dequantize_sum_grouped_rotated: s = dequantize_grouped(term_0 -> float32, SET) + dequantize_grouped(term_i -> float32) for i >= 1 in order,
// z = the float32 inverse rotation of s; out = convert(z) (SET) or convert(widen(out) + z) (ADD: one float32 add, one rounding).  It is
// dequantize_grouped_rotated_kernel with a term list: the first term is stored, the others are added (term i + 1 in flight meanwhile), and ONE
// rotation serves the sum.  terms.count >= 1; with one term the bytes are dequantize_grouped_rotated_kernel's.
template <int DT_OUT, int BITS, int OP, int G>
__global__ void __launch_bounds__(kGroupedBlock)
dequantize_sum_grouped_rotated_kernel(void* __restrict__ out, int64_t numel, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi, GroupedTerms terms) {
    using T = GroupedQuantTile<DT_F32, BITS, G>;
    using L = GroupedTermLoad<DT_F32, BITS, G>;
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

    L next;
    if (full) next.load(terms.in[0], terms.scales[0], terms.zero_points[0], v0, gj, has_group, lane);
    [[maybe_unused]] u32x4 old[NV];
    [[maybe_unused]] u32x2 told[NV];
    if constexpr (OP == OP_ADD) grouped_rot_load<DT_OUT, NV>(out, numel, v0, lane, full, old, told);
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

    u32x4 raw[NV];
    stage_term(0);
    grouped_set_term<DT_F32, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
    for (int i = 1; i < count; ++i) {
        wave_lds_sync();   // every lane has read term i - 1
        stage_term(i);
        grouped_add_term<DT_F32, DT_F32, BITS, G>(raw, stage, s_a[wave], s_b[wave], s_z[wave], lane);
    }
    grouped_rotate_chunk<BITS, G, true>(raw, numel, g0, full, lane, rot_lo, rot_hi);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        if constexpr (OP == OP_ADD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) raw[r][e] = __float_as_uint(__fadd_rn(__uint_as_float(raw[r][e]), __uint_as_float(old[r][e])));
        }
        if constexpr (DT_OUT == DT_F32) {
            grouped_store_vector<DT_F32>(out, numel, v0 + r * 64 + lane, full, raw[r]);
        } else {
            const u32x2 o {f32x2_to_bf16x2_bits(__uint_as_float(raw[r][0]), __uint_as_float(raw[r][1])),
                           f32x2_to_bf16x2_bits(__uint_as_float(raw[r][2]), __uint_as_float(raw[r][3]))};
            grouped_rot_store_bf16x4(out, numel, v0 + r * 64 + lane, full, o);
        }
    }
}

// ---- The guarded kernels, for buffers that are not 16-byte aligned: one wave per group, the group's float32 values in the block's LDS, element by
// element, the same bytes.  Correct, not fast.

// buf[0 .. G): rotated in place by the wave, the stages in the contract's order; G a power of two in [32, 4096]
template <bool INVERSE>
__device__ __forceinline__ void grouped_rot_guarded(float* buf, int G, int lane, uint32_t seed_lo, uint32_t seed_hi) {
    const int k = __builtin_ctz(G);
    const float c = __fmul_rn((k & 1) ? 0x1.6a09e6p+0f : 1.0f, __uint_as_float(static_cast<uint32_t>(127 - ((k + 1) >> 1)) << 23));
    auto sign_of = [&](int j) { return ((grouped_rot_sign_word(seed_lo, seed_hi, static_cast<uint32_t>(j) >> 4) >> (j & 15)) & 1u) << 31; };
    if constexpr (!INVERSE) {
        for (int j = lane; j < G; j += 64) buf[j] = __uint_as_float(__float_as_uint(buf[j]) ^ sign_of(j));
    }
    wave_lds_sync();
    for (int h = 1; h < G; h <<= 1) {
        for (int p = lane; p < G / 2; p += 64) {
            const int i = ((p & ~(h - 1)) << 1) | (p & (h - 1));
            const float a = buf[i], b = buf[i + h];
            buf[i] = __fadd_rn(a, b);
            buf[i + h] = __fsub_rn(a, b);
        }
        wave_lds_sync();
    }
    for (int j = lane; j < G; j += 64) {
        const float v = __fmul_rn(buf[j], c);
        buf[j] = INVERSE ? __uint_as_float(__float_as_uint(v) ^ sign_of(j)) : v;
    }
    wave_lds_sync();
}

template <int DT, bool INVERSE>
__global__ void __launch_bounds__(kGroupedRotGuardedBlock)
hadamard_grouped_scalar_kernel(const void* in, void* out, int64_t numel, int64_t group_size, int64_t ngroups, uint32_t seed_lo, uint32_t seed_hi) {
    __shared__ float buf[kGroupedMaxG];
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t b = g * group_size;
        const int len = static_cast<int>(b + group_size < numel ? group_size : numel - b);
        if (len < group_size) {   // the ragged group: its bits, unchanged
            if (in != out) {
                for (int o = lane; o < len; o += 64) {
                    if constexpr (DT == DT_F32) static_cast<uint32_t*>(out)[b + o] = static_cast<const uint32_t*>(in)[b + o];
                    else static_cast<uint16_t*>(out)[b + o] = static_cast<const uint16_t*>(in)[b + o];
                }
            }
            continue;
        }
        for (int o = lane; o < len; o += 64) buf[o] = InVec<DT>::load_scalar(in, b + o);
        grouped_rot_guarded<INVERSE>(buf, len, lane, seed_lo, seed_hi);
        for (int o = lane; o < len; o += 64) {
            if constexpr (DT == DT_F32) static_cast<float*>(out)[b + o] = buf[o];
            else static_cast<uint16_t*>(out)[b + o] = static_cast<uint16_t>(f32_to_bf16_bits(buf[o]));
        }
        wave_lds_sync();
    }
}

template <int DT_IN, int BITS, int MODE>
__global__ void __launch_bounds__(kGroupedRotGuardedBlock)
quantize_grouped_rotated_scalar_kernel(const void* __restrict__ in, uint8_t* __restrict__ out, int64_t numel, int64_t group_size, float* __restrict__ scales,
                                       uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi, float threshold, uint32_t seed_lo,
                                       uint32_t seed_hi, uint64_t index_base) {
    constexpr int PACK = 8 / BITS, QMAX = (1 << BITS) - 1;
    __shared__ float buf[kGroupedMaxG];
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t b = g * group_size;
        const int len = static_cast<int>(b + group_size < numel ? group_size : numel - b);
        for (int o = lane; o < len; o += 64) buf[o] = InVec<DT_IN>::load_scalar(in, b + o);
        if (len == group_size) grouped_rot_guarded<false>(buf, len, lane, rot_lo, rot_hi);
        else wave_lds_sync();
        QuantParams p;
        DequantParams d;   // not used: nothing is read back here
        grouped_guarded_params<BITS>([&](int o) { return buf[o]; }, len, lane, false, scales, zero_points, g, threshold, seed_lo, seed_hi, index_base, p, d);
        uint8_t* og = out + b / PACK;   // a group starts on a whole packed byte
        for (int by = lane; by * PACK < len; by += 64) {
            uint32_t acc = 0;
            for (int k = 0; k < PACK; ++k) {
                const int o = by * PACK + k;
                if (o >= len) break;
                acc |= quant_one<MODE, QMAX>(buf[o], p, static_cast<uint64_t>(b + o)) << (k * BITS);
            }
            og[by] = static_cast<uint8_t>(acc);
        }
        wave_lds_sync();
    }
}

template <int DT_OUT, int BITS, int OP>
__global__ void __launch_bounds__(kGroupedRotGuardedBlock)
dequantize_grouped_rotated_scalar_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, int64_t numel, int64_t group_size,
                                         const float* __restrict__ scales, const uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo,
                                         uint32_t rot_hi) {
    constexpr int FORM = DequantForm<BITS, DT_F32>::value;
    __shared__ float buf[kGroupedMaxG];
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t b = g * group_size;
        const int len = static_cast<int>(b + group_size < numel ? group_size : numel - b);
        DequantParams p {};
        p.scale = scales[g];
        p.zp32 = zero_points[g];
        p.zp64 = p.zp32;
        p.bias = __fmul_rn(-static_cast<float>(p.zp32), p.scale);
        for (int o = lane; o < len; o += 64) {
            const int64_t bit = (b + o) * BITS;
            buf[o] = dequant_one<FORM>((in[bit >> 3] >> (bit & 7)) & ((1u << BITS) - 1u), p);
        }
        if (len == group_size) grouped_rot_guarded<true>(buf, len, lane, rot_lo, rot_hi);
        else wave_lds_sync();
        for (int o = lane; o < len; o += 64) {
            const float z = buf[o];
            if constexpr (DT_OUT == DT_F32) {
                float* dst = static_cast<float*>(out);
                dst[b + o] = OP == OP_ADD ? __fadd_rn(z, dst[b + o]) : z;
            } else {
                uint16_t* dst = static_cast<uint16_t*>(out);
                dst[b + o] = static_cast<uint16_t>(f32_to_bf16_bits(OP == OP_ADD ? __fadd_rn(z, bf16_bits_to_f32(dst[b + o])) : z));
            }
        }
        wave_lds_sync();
    }
}

// element o of group g of term i of a term list, dequantized to float32 with the group's parameters (what dequantize_grouped -> float32 stores)
template <int BITS>
struct GroupedRotGuardedTerm {
    static constexpr int FORM = DequantForm<BITS, DT_F32>::value;
    DequantParams p {};
    const uint8_t* in;

    __device__ __forceinline__ GroupedRotGuardedTerm(const GroupedTerms& terms, int i, int64_t g) : in(terms.in[i]) {
        p.scale = terms.scales[i][g];
        p.zp32 = terms.zero_points[i][g];
        p.zp64 = p.zp32;
        p.bias = __fmul_rn(-static_cast<float>(p.zp32), p.scale);
    }

    __device__ __forceinline__ float operator()(int64_t element) const {
        const int64_t bit = element * BITS;
        return dequant_one<FORM>((in[bit >> 3] >> (bit & 7)) & ((1u << BITS) - 1u), p);
    }
};

// reduce_quantize_grouped_rotated, guarded: the accumulator's group widened into LDS and rotated (a whole group only), the terms added in order
// element by element -- a lane adds into the elements it holds --, then the tail of quantize_grouped_rotated_scalar_kernel.
template <int DT_ACC, int BITS, int MODE>
__global__ void __launch_bounds__(kGroupedRotGuardedBlock)
reduce_quantize_grouped_rotated_scalar_kernel(const void* __restrict__ acc, uint8_t* __restrict__ out, int64_t numel, int64_t group_size,
                                              float* __restrict__ scales, uint8_t* __restrict__ zero_points, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi,
                                              float threshold, uint32_t seed_lo, uint32_t seed_hi, uint64_t index_base, GroupedTerms terms) {
    constexpr int PACK = 8 / BITS, QMAX = (1 << BITS) - 1;
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
        wave_lds_sync();
        QuantParams p;
        DequantParams d;   // not used: nothing is read back here
        grouped_guarded_params<BITS>([&](int o) { return buf[o]; }, len, lane, false, scales, zero_points, g, threshold, seed_lo, seed_hi, index_base, p, d);
        uint8_t* og = out + b / PACK;   // a group starts on a whole packed byte
        for (int by = lane; by * PACK < len; by += 64) {
            uint32_t q = 0;
            for (int k = 0; k < PACK; ++k) {
                const int o = by * PACK + k;
                if (o >= len) break;
                q |= quant_one<MODE, QMAX>(buf[o], p, static_cast<uint64_t>(b + o)) << (k * BITS);
            }
            og[by] = static_cast<uint8_t>(q);
        }
        wave_lds_sync();
    }
}

// dequantize_sum_grouped_rotated, guarded: the first term stored into LDS, the others added in order, the sum rotated back (a whole group only),
// then the stores of dequantize_grouped_rotated_scalar_kernel.  terms.count >= 1.
template <int DT_OUT, int BITS, int OP>
__global__ void __launch_bounds__(kGroupedRotGuardedBlock)
dequantize_sum_grouped_rotated_scalar_kernel(void* __restrict__ out, int64_t numel, int64_t group_size, int64_t ngroups, uint32_t rot_lo, uint32_t rot_hi,
                                             GroupedTerms terms) {
    __shared__ float buf[kGroupedMaxG];
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t b = g * group_size;
        const int len = static_cast<int>(b + group_size < numel ? group_size : numel - b);
        for (int i = 0; i < terms.count; ++i) {
            const GroupedRotGuardedTerm<BITS> term(terms, i, g);
            for (int o = lane; o < len; o += 64) buf[o] = i == 0 ? term(b + o) : __fadd_rn(term(b + o), buf[o]);
        }
        if (len == group_size) grouped_rot_guarded<true>(buf, len, lane, rot_lo, rot_hi);
        else wave_lds_sync();
        for (int o = lane; o < len; o += 64) {
            const float z = buf[o];
            if constexpr (DT_OUT == DT_F32) {
                float* dst = static_cast<float*>(out);
                dst[b + o] = OP == OP_ADD ? __fadd_rn(z, dst[b + o]) : z;
            } else {
                uint16_t* dst = static_cast<uint16_t*>(out);
                dst[b + o] = static_cast<uint16_t>(f32_to_bf16_bits(OP == OP_ADD ? __fadd_rn(z, bf16_bits_to_f32(dst[b + o])) : z));
            }
        }
        wave_lds_sync();
    }
}

}  // namespace pq
