// Histogram clip search for per-tensor quantization parameters on gfx950 (include/piquant_hip.h, "HISTOGRAM CLIP SEARCH", has the definition).
//
// Three steps behind the min/max scan, all of them integer or binary64 arithmetic whose result does not depend on the grid:
//   1. clip_histogram_kernel   one more read stream over x: every block counts its share into a uint32[kClipBins] LDS histogram (32 KiB) with
//                              ds_add_u32 (no return value) and stores it, plain stores, as ITS row of the partials
//      clip_fold_kernel        sums the rows into uint64[kClipBins] (set or accumulated): integer sums, exact in any order
//   2. clip_search_kernel      one block per candidate: 8 contiguous bins per thread folded in registers, the wave's xor butterfly, the 16 wave
//                              sums in adjacent pairs -- together the adjacent-pair tree over the 8192 terms
//   3. clip_choose_kernel      one wave: the smallest error under strict <, the record, the choice, the errors
// No float atomics, no grid barrier, no spin-wait: the launches are ordered by the stream.
#pragma once

#include "minmax_kernels.hpp"

namespace pq {

constexpr int kClipBins = 8192;              // PIQUANT_HIP_CLIP_BINS
constexpr int kClipMaxSteps = 63;            // PIQUANT_HIP_CLIP_MAX_STEPS: r_k = 1 - k / 64 >= 1 / 32
constexpr int kClipHistBlock = 1024;         // one block per CU: 16 waves, four 16-byte loads in flight per lane (the scan's U)
constexpr int kClipHistU = 4;
constexpr int kClipHistBlocksPerCU = 1;
constexpr bool kClipHistGlobalAdds = false;  // how a block gives its counts out: its own row + a fold launch (false) or 64-bit global adds (true)
constexpr int kClipSearchBlock = 1024;       // x 8 bins per thread = kClipBins
constexpr int kClipFoldBlock = 1024;         // 16 waves x 64 bins: wave w sums rows w, w + 16, ...
constexpr int kClipFoldBins = 64;
static_assert(kClipSearchBlock * 8 == kClipBins, "eight contiguous bins per thread");
static_assert(kClipBins % kClipFoldBins == 0 && kClipBins % (4 * kClipHistBlock) == 0, "whole vectors and whole fold blocks");

// The range the histogram and the search share: the scan's pair behind the keys.
__device__ __forceinline__ void clip_range(const int32_t* keys, float& lo, float& hi) {
    lo = key_to_float(keys[0]);
    hi = -key_to_float(keys[1]);
}

// `vectors` == 0: the input is not even element-aligned, every element goes through the guarded loop behind the vector loop.
// `head`: elements in FRONT of `in`, fewer than a vector (the launcher moved `in` up to a 16-byte boundary, as the scan's does).
// Nothing outside [in - head, in + numel) is read: the vector loop ends with the last WHOLE vector and never clamps (a vector counted twice would
// be counted twice).
// GLOBAL_ADDS: the other way of giving the counts out -- no row, no fold launch: every block adds its non-zero counts to the caller's zeroed or running
// uint64[kClipBins] with 64-bit integer global adds whose result is not used (`partials` is then that array).  The library launches the form that
// measured faster (kClipHistGlobalAdds; tools/clip_hist_ab.hip times both in one run, profiles/EXPERIMENTS.md has the numbers).
template <int DT_IN, int U, bool NT, int BLOCK, bool GLOBAL_ADDS = false>
__global__ void __launch_bounds__(BLOCK) clip_histogram_kernel(const void* __restrict__ in, int64_t numel, const int32_t* __restrict__ keys,
                                                                uint32_t* __restrict__ partials, int head, uint32_t grid, int vectors) {
    constexpr int EPV = InVec<DT_IN>::EPV;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[kClipBins];
    for (int i = threadIdx.x; i < kClipBins; i += BLOCK) s_hist[i] = 0u;
    float lo, hi;
    clip_range(keys, lo, hi);
    __syncthreads();
    if (hi > lo) {   // grid-uniform; otherwise (nothing scanned, a constant tensor) the counts stay zero
        const float inv = __fdiv_rn(static_cast<float>(kClipBins), __fsub_rn(hi, lo));   // wf may be +inf (inv = 0), inv may be +inf
        auto count = [&](float x) {
            if (x == x) {   // NaNs are not counted
                float t = __fmul_rn(__fsub_rn(x, lo), inv);
                t = __builtin_fminf(__builtin_fmaxf(t, 0.0f), static_cast<float>(kClipBins - 1));   // fmaxf(NaN, 0) = 0: inf - inf, inf * 0
                (void)__hip_atomic_fetch_add(&s_hist[static_cast<int>(t)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        };
        auto count_vec = [&](const u32x4& raw) {
            float f[EPV];
            InVec<DT_IN>::unpack(raw, f);
#pragma unroll
            for (int e = 0; e < EPV; ++e) count(f[e]);
        };
        const u32x4* __restrict__ in16 = static_cast<const u32x4*>(in);
        const int64_t n_vec = vectors ? numel / EPV : 0;
        const int64_t tid = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
        const int64_t nthreads = static_cast<int64_t>(grid) * BLOCK;
        // rolling window of U loads per lane over the whole rounds (v = tid + k * nthreads, k < U, all inside the tensor), as the scan's
        u32x4 raw[U];
        int64_t base = tid;
        bool whole = base + (U - 1) * nthreads < n_vec;
        if (whole) {
#pragma unroll
            for (int k = 0; k < U; ++k) raw[k] = ld<NT>(in16 + base + k * nthreads);
        }
        while (whole) {
            const int64_t next = base + U * nthreads;
            const bool more = next + (U - 1) * nthreads < n_vec;
#pragma unroll
            for (int k = 0; k < U; ++k) {
                count_vec(raw[k]);
                if (more) raw[k] = ld<NT>(in16 + next + k * nthreads);
            }
            base = next;
            whole = more;
        }
        for (int64_t v = base; v < n_vec; v += nthreads) count_vec(ld<NT>(in16 + v));   // fewer than U vectors of this lane are left
        for (int64_t i = n_vec * EPV + tid; i < numel; i += nthreads) count(InVec<DT_IN>::load_scalar(in, i));
        if (blockIdx.x == 0 && static_cast<int>(threadIdx.x) < head) count(InVec<DT_IN>::load_scalar(in, static_cast<int64_t>(threadIdx.x) - head));
    }
    __syncthreads();
    if constexpr (GLOBAL_ADDS) {
        unsigned long long* hist = reinterpret_cast<unsigned long long*>(partials);
        for (int i = threadIdx.x; i < kClipBins; i += BLOCK) {
            const uint32_t c = s_hist[i];
            if (c != 0u) (void)__hip_atomic_fetch_add(hist + i, static_cast<unsigned long long>(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    u32x4* mine =reinterpret_cast<u32x4*>(partials + static_cast<size_t>(blockIdx.x) * kClipBins);
    const u32x4* s16 = reinterpret_cast<const u32x4*>(s_hist);
    for (int i = threadIdx.x; i < kClipBins / 4; i += BLOCK) mine[i] = s16[i];
}

// hist[j] (init ? = : +=) the sum of the rows' counts of bin j.  Block b owns bins [64 b, 64 b + 64): one thread per (row slice, bin), the
// slices meet in LDS.  rows == 0 with init != 0 zeroes the counts.
__global__ void __launch_bounds__(kClipFoldBlock) clip_fold_kernel(const uint32_t* __restrict__ partials, uint32_t rows, unsigned long long* __restrict__ hist, int init) {
    constexpr int WAVES = kClipFoldBlock / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = blockIdx.x * kClipFoldBins + lane;
    unsigned long long sum = 0;
#pragma unroll 8
    for (uint32_t r = wave; r < rows; r += WAVES) sum += partials[static_cast<size_t>(r) * kClipBins + bin];
    __shared__ unsigned long long s_sum[WAVES][kClipFoldBins];
    s_sum[wave][lane] = sum;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) sum += s_sum[w][lane];
        hist[bin] = init ? sum : hist[bin] + sum;
    }
}

// Candidate k of the search: the shrunk range and its ordinary epilogue.  false: not evaluated (k > 0 and not hi_k > lo_k).
__device__ __forceinline__ bool clip_candidate(float lo, float hi, int k, int bits, float& scale, int64_t& zp) {
    const float r = __fsub_rn(1.0f, __fmul_rn(static_cast<float>(k), 0.015625f));   // 1 - k / 64, exact
    const float lo_k = __fmul_rn(lo, r), hi_k = __fmul_rn(hi, r);
    quant_params_epilogue(float_to_key(lo_k), float_to_key(-hi_k), bits, scale, zp);
    return k == 0 || hi_k > lo_k;
}

// Block k: E_k from the folded counts, binary64, every operation rounded once (the unit is compiled without contraction; the intrinsics say so again).
__global__ void __launch_bounds__(kClipSearchBlock) clip_search_kernel(const int32_t* __restrict__ keys, const unsigned long long* __restrict__ hist, int bits,
                                                                        double* __restrict__ errors) {
    constexpr int WAVES = kClipSearchBlock / 64;
    const int k = blockIdx.x;
    const double nan = __builtin_nan("");
    float lo, hi;
    clip_range(keys, lo, hi);
    float scale;
    int64_t zp;
    const bool evaluated = hi > lo && clip_candidate(lo, hi, k, bits, scale, zp);   // block-uniform
    if (!evaluated) {
        if (threadIdx.x == 0) errors[k] = nan;
        return;
    }
    const double dlo = static_cast<double>(lo), s = static_cast<double>(scale), z = static_cast<double>(zp);
    const double qmax = static_cast<double>((uint64_t {1} << bits) - 1);
    const double W = __ddiv_rn(__dsub_rn(static_cast<double>(hi), dlo), static_cast<double>(kClipBins));
    double term[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int j = static_cast<int>(threadIdx.x) * 8 + i;
        const unsigned long long c = hist[j];
        const double m = __dadd_rn(dlo, __dmul_rn(static_cast<double>(j) + 0.5, W));
        double u = __dadd_rn(floor(__dadd_rn(__ddiv_rn(m, s), 0.5)), z);
        u = fmin(fmax(u, 0.0), qmax);   // fmax(NaN, 0) = 0
        const double d = __dmul_rn(__dsub_rn(u, z), s);
        const double e = __dsub_rn(m, d);
        term[i] = c == 0 ? 0.0 : __dmul_rn(static_cast<double>(c), __dmul_rn(e, e));
    }
    double sum = __dadd_rn(__dadd_rn(__dadd_rn(term[0], term[1]), __dadd_rn(term[2], term[3])), __dadd_rn(__dadd_rn(term[4], term[5]), __dadd_rn(term[6], term[7])));
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) sum = __dadd_rn(sum, __shfl_xor(sum, mask, 64));   // both partners form the same sum: the next level of the tree
    __shared__ double s_wave[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double w[WAVES];
#pragma unroll
        for (int i = 0; i < WAVES; ++i) w[i] = s_wave[i];
#pragma unroll
        for (int n = WAVES; n > 1; n >>= 1) {
#pragma unroll
            for (int i = 0; i < n / 2; ++i) w[i] = __dadd_rn(w[2 * i], w[2 * i + 1]);
        }
        errors[k] = w[0] != w[0] ? nan : w[0];   // one NaN pattern, whatever produced it
    }
}

// One wave: the choice, the record of the chosen candidate, and the caller's copies.  steps == 1 searches nothing: the record of the keys, choice 0,
// no error evaluated.  `errors` holds what clip_search_kernel's blocks 0 .. steps - 1 wrote.
__global__ void __launch_bounds__(64) clip_choose_kernel(const int32_t* __restrict__ keys, const double* __restrict__ errors, int bits, int steps, ParamRecord* __restrict__ out,
                                                          int32_t* __restrict__ out_choice, double* __restrict__ out_errors) {
    const int lane = threadIdx.x;
    const double nan = __builtin_nan("");
    const double mine = steps > 1 && lane < steps ? errors[lane] : nan;
    if (out_errors != nullptr && lane < kClipMaxSteps) out_errors[lane] = mine;
    __shared__ double s_e[64];
    s_e[lane] = mine;
    __syncthreads();
    if (lane != 0) return;
    float lo, hi;
    clip_range(keys, lo, hi);
    int best = 0;
    if (steps > 1 && hi > lo) {
        double e_best = s_e[0];
        for (int k = 1; k < steps; ++k) {
            if (s_e[k] < e_best) {   // strict: a tie or a NaN keeps the smaller k
                e_best = s_e[k];
                best = k;
            }
        }
    }
    float scale;
    int64_t zp;
    if (best == 0) quant_params_epilogue(keys[0], keys[1], bits, scale, zp);   // exactly compute_quant_params_device's record
    else (void)clip_candidate(lo, hi, best, bits, scale, zp);
    out->scale = scale;
    out->inv_scale = __fdiv_rn(1.0f, scale);
    out->zero_point = zp;
    if (out_choice != nullptr) *out_choice = best;
}

// choice 0 and no error evaluated: what the one-call form adds to compute_quant_params_device's record when steps == 1
__global__ void __launch_bounds__(64) clip_unsearched_kernel(int32_t* __restrict__ out_choice, double* __restrict__ out_errors) {
    if (out_errors != nullptr && static_cast<int>(threadIdx.x) < kClipMaxSteps) out_errors[threadIdx.x] = __builtin_nan("");
    if (out_choice != nullptr && threadIdx.x == 0) *out_choice = 0;
}

}  // namespace pq
