// Group-wise quantize-dequantize ("fake quantization", piquant_hip_quantize_dequantize_grouped): out (op)= dequantize_grouped(quantize_grouped(x))
// in ONE launch that reads x once and never writes the packed tensor -- the kernels and their launch bodies, one template per float type.
// kernels_grouped_requant.hip instantiates the float32 half (and holds the launchers of launch.hpp), kernels_grouped_requant_bf16.hip the bfloat16
// half: two translation units, so that `make -j` compiles them side by side.
//
// Streaming kernel: the quantize tile of grouped_kernels.hpp (a wave owns NG whole groups as NV rows of 16-byte vectors).  The wave loads its rows,
// runs the quantize chunk body with KEEP and REQUANT (segmented min / max and one epilogue per group unless the parameters are given, the
// quantization under the bounded-chunk rule; the packed words stay in the wave's LDS slice and nothing of them goes to memory), then reads its own
// packed words back, dequantizes them with the chunk's parked parameters in the pair's own form and stores 16 bytes per lane and row with
// write-through stores.  The input rows are dead behind the quantize step: for ADD the accumulator rows are loaded into those registers there, not
// beside the input (float32 -> uint2 already holds 16 rows per lane).  out == in works for SET and ADD: a wave reads and writes its own chunk only,
// and every read of the chunk's input comes before the chunk's first store.  No scan, no atomics, no grid barrier; waves never wait for one another.
//
// Templates: the float type, the quantized width, the rounding mode and the group size -- they shape the tile and the instruction stream of the hot
// loop.  Wave-uniform runtime branches: given or computed parameters (a branch around the min / max pass and the epilogue), the store op (one load
// and one add per vector) and whether computed parameters are written (scales != NULL).
#pragma once

#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

// out rows <- dequantize(the chunk's packed bytes in `stage`), for `add` added to the accumulator rows in acc (the fp32 sum rounded separately, a
// bfloat16 result rounded once: the grouped dequantize ADD); elements at or past numel are not written.  The read-back is grouped_residual_store's.
template <int DT, int BITS, int G, int NV_ = GroupedQuantTile<DT, BITS, G>::NV>
__device__ __forceinline__ void grouped_requant_store(const u32x4 (&acc)[NV_], void* out, bool add, int64_t numel, int64_t v0, bool full, int lane,
                                                      const uint8_t* stage, const float* s_scale, const float* s_zp) {
    using T = GroupedQuantTile<DT, BITS, G>;
    constexpr int EPV = T::EPV, NV = T::NV, RPG = T::RPG, SETS = T::SETS;
    DequantParams p[SETS];
    grouped_parked_dequant_params<DT, BITS, G>(p, s_scale, s_zp, lane);
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        float f[EPV];
        grouped_dequantize_row<DT, BITS, G>(stage, r, lane, p[r / RPG], f);
        if (add) {   // wave-uniform
            float old[EPV];
            InVec<DT>::unpack(acc[r], old);
#pragma unroll
            for (int e = 0; e < EPV; ++e) f[e] = __fadd_rn(f[e], old[e]);
        }
        u32x4 o;
        if constexpr (DT == DT_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = __float_as_uint(f[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f32x2_to_bf16x2_bits(f[2 * e], f[2 * e + 1]);
        }
        grouped_store_vector<DT>(out, numel, v0 + r * 64 + lane, full, o);
    }
}

// one wave's chunk (NG groups from group g0 on) of one tensor; the wave's LDS slices as in grouped_ef_chunk.  `in` and `out` may be the same buffer.
template <int DT, int BITS, int MODE, int G>
__device__ __forceinline__ void grouped_requant_chunk(const void* in, void* out, int64_t numel, float* scales, uint8_t* zero_points, int64_t ngroups,
                                                      const QuantParams& p0, int64_t g0, bool given, bool add, int lane, uint8_t* stage, float* s_a,
                                                      float* s_b, float* s_c) {
    using T = GroupedQuantTile<DT, BITS, G>;
    constexpr int NV = T::NV, NG = T::NG;
    const int64_t v0 = g0 * T::V;
    const bool full = (g0 + NG) * G <= numel;                       // wave-uniform

    u32x4 raw[NV];
    grouped_load<DT, NV>(in, numel, v0, lane, full, raw);
    grouped_quantize_chunk<DT, BITS, MODE, G, false, NV, true, true>(raw, nullptr, numel, scales, zero_points, ngroups, p0, g0, full, lane, stage, s_a, s_b, s_c,
                                                                     given);
    if (add) grouped_load<DT, NV>(out, numel, v0, lane, full, raw);   // the input rows are dead: the accumulator's take their registers
    grouped_requant_store<DT, BITS, G>(raw, out, add, numel, v0, full, lane, stage, s_c, s_b);
}

template <int DT, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_dequantize_grouped_kernel(const void* in, void* out, int64_t numel, float* scales, uint8_t* zero_points, int64_t ngroups, int given, int add,
                                   QuantParams p0) {
    using T = GroupedQuantTile<DT, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];   // {min, max}, then {1/scale, zero point, scale} of the chunk's groups

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t g0 = chunk * NG;
    if (g0 >= ngroups) return;
    grouped_requant_chunk<DT, BITS, MODE, G>(in, out, numel, scales, zero_points, ngroups, p0, g0, given != 0, add != 0, lane, s_out[wave], s_a[wave],
                                             s_b[wave], s_c[wave]);
}

// Up to kGroupedBatchMax independent tensors in ONE launch, found through the prefix table of quantize_grouped_batch_kernel.
struct GroupedRequantBatchArgs {
    const void* in[kGroupedBatchMax];
    void* out[kGroupedBatchMax];
    float* scales[kGroupedBatchMax];
    uint8_t* zero_points[kGroupedBatchMax];
    int64_t numel[kGroupedBatchMax];
    int64_t chunk_begin[kGroupedBatchMax + 1];
    int count;
};

template <int DT, int BITS, int MODE, int G>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_dequantize_grouped_batch_kernel(GroupedRequantBatchArgs a, int given, int add, QuantParams p0) {
    using T = GroupedQuantTile<DT, BITS, G>;
    constexpr int NG = T::NG, WAVES = kGroupedBlock / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[WAVES][T::OUT_BYTES];
    __shared__ float s_a[WAVES][NG], s_b[WAVES][NG], s_c[WAVES][NG];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    int t;
    if (!grouped_batch_tensor(a, c, t)) return;
    const int64_t numel = a.numel[t];
    grouped_requant_chunk<DT, BITS, MODE, G>(a.in[t], a.out[t], numel, a.scales[t], a.zero_points[t], (numel + G - 1) / G, p0, (c - a.chunk_begin[t]) * NG,
                                             given != 0, add != 0, lane, s_out[wave], s_a[wave], s_b[wave], s_c[wave]);
}

// Guarded form (grouped_guarded_params) for buffers that are not 16-byte aligned.  Given parameters, the store op and whether computed parameters
// are written are runtime here.  The group's min / max pass ends in a wave reduction, so every load of it is complete before the group's first
// store: out == in stays correct.
template <int DT, int BITS, int MODE>
__global__ void __launch_bounds__(kGroupedBlock)
quantize_dequantize_grouped_scalar_kernel(const void* in, void* out, int64_t numel, int64_t group_size, float* scales, uint8_t* zero_points, int64_t ngroups,
                                          int given, int add, float threshold, uint32_t seed_lo, uint32_t seed_hi, uint64_t index_base) {
    constexpr int QMAX = (1 << BITS) - 1, FORM = DequantForm<BITS, DT>::value;
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kGroupedBlock / 64);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the group loop is wave-uniform
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * (kGroupedBlock / 64) + wave; g < ngroups; g += waves) {
        const int64_t b = g * group_size;
        const int len = static_cast<int>(b + group_size < numel ? group_size : numel - b);   // <= 4096: 32-bit offsets inside the group
        QuantParams p;
        DequantParams d;
        grouped_guarded_params<BITS>([&](int o) { return InVec<DT>::load_scalar(in, b + o); }, len, lane, given != 0, scales, zero_points, g, threshold, seed_lo,
                                     seed_hi, index_base, p, d);
        for (int o0 = 0; o0 < len; o0 += 64) {
            const int o = o0 + lane;
            if (o >= len) continue;
            const uint32_t q = quant_one<MODE, QMAX>(InVec<DT>::load_scalar(in, b + o), p, static_cast<uint64_t>(b + o));
            float f = dequant_one<FORM>(q, d);
            if (add) f = __fadd_rn(f, InVec<DT>::load_scalar(out, b + o));
            if constexpr (DT == DT_F32) static_cast<float*>(out)[b + o] = f;
            else static_cast<uint16_t*>(out)[b + o] = static_cast<uint16_t>(f32_to_bf16_bits(f));
        }
    }
}

template <int DT>
void requant_batch(const GroupedRequantBatchLaunch& b, hipStream_t stream) {
    static_assert(kGroupedBatchMaxTensors == kGroupedBatchMax, "host and device batch limits");
    const char* what = "quantize_dequantize_grouped";
    if (b.count <= 0) return;
    if (b.count > kGroupedBatchMax) panic("%s_batch: %d tensors, at most %d per launch", what, b.count, kGroupedBatchMax);
    const QuantParams p = grouped_call_params(b.rm);
    const int given = b.params_given ? 1 : 0, add = b.op == OP_ADD ? 1 : 0;
    with_quant_bits(b.dt_out, [&](auto bi) {
        constexpr int BITS = decltype(bi)::value;
        with_round_mode<DT, BITS>(b.rm.round_mode, [&](auto mi) {
            constexpr int MODE = decltype(mi)::value;
            with_group_size(b.group_size, what, [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int NG = GroupedQuantTile<DT, BITS, G>::NG;
                GroupedRequantBatchArgs a {};
                for (int t = 0; t < b.count; ++t) {
                    a.in[t] = b.t[t].in;
                    a.out[t] = b.t[t].out;
                    a.scales[t] = b.t[t].scales;
                    a.zero_points[t] = b.t[t].zero_points;
                    a.numel[t] = b.t[t].numel;
                }
                a.count = b.count;
                const int64_t chunks = fill_chunk_table(a, static_cast<int64_t>(G) * NG);
                if (chunks == 0) return;
                const dim3 grid(grouped_blocks(chunks, what)), block(kGroupedBlock);
                if (b.count == 1)   // the single call: its arguments arrive as leading scalars, no table
                    PQ_LAUNCH((quantize_dequantize_grouped_kernel<DT, BITS, MODE, G>), grid, block, 0, stream, a.in[0], a.out[0], a.numel[0], a.scales[0],
                              a.zero_points[0], (a.numel[0] + G - 1) / G, given, add, p);
                else PQ_LAUNCH((quantize_dequantize_grouped_batch_kernel<DT, BITS, MODE, G>), grid, block, 0, stream, a, given, add, p);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

template <int DT>
void requant_guarded(const GroupedRequantLaunch& q, hipStream_t stream, int num_cu) {
    if (q.numel <= 0) return;
    const QuantParams p = grouped_call_params(q.rm);
    const int64_t ngroups = (q.numel + q.group_size - 1) / q.group_size;
    const dim3 grid(grouped_guarded_blocks(ngroups, num_cu));
    with_quant_bits(q.dt_out, [&](auto bi) {
        constexpr int BITS = decltype(bi)::value;
        with_round_mode<DT, BITS>(q.rm.round_mode, [&](auto mi) {
            constexpr int MODE = decltype(mi)::value;
            PQ_LAUNCH((quantize_dequantize_grouped_scalar_kernel<DT, BITS, MODE>), grid, dim3(kGroupedBlock), 0, stream, q.in, q.out, q.numel, q.group_size,
                      q.scales, q.zero_points, ngroups, q.params_given ? 1 : 0, q.op == OP_ADD ? 1 : 0, p.threshold, p.seed_lo, p.seed_hi, p.index_base);
        });
    });
    PQ_HIP(hipGetLastError());
}

// the launchers of the two halves
void launch_quantize_dequantize_grouped_batch_f32(const GroupedRequantBatchLaunch& b, hipStream_t stream);
void launch_quantize_dequantize_grouped_guarded_f32(const GroupedRequantLaunch& q, hipStream_t stream, int num_cu);
void launch_quantize_dequantize_grouped_batch_bf16(const GroupedRequantBatchLaunch& b, hipStream_t stream);
void launch_quantize_dequantize_grouped_guarded_bf16(const GroupedRequantLaunch& q, hipStream_t stream, int num_cu);

}  // namespace pq
