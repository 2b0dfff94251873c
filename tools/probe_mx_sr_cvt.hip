// Probe: what the gfx950 stochastic-rounding scaled conversions (v_cvt_scalef32_sr_pk_fp4_f32, v_cvt_scalef32_sr_fp8_f32,
// v_cvt_scalef32_sr_pk32_{fp6,bf6}_f32) do with their random operand, measured against the stochastic definition of include/piquant_hip.h
// (piquant_hip_quantize_mx_sr).  Not a test.
//   hipcc --offload-arch=gfx950 -O2 tools/probe_mx_sr_cvt.hip -o tools/probe_mx_sr_cvt && ./tools/probe_mx_sr_cvt
// Two questions per instruction.
//   bits     which bits of the operand are consumed: an input just below a code (every discarded mantissa bit set) is converted under the 32
//            one-bit operands 1 << b; the b that carry it up are printed as a mask, for an input in the format's normal range and one in its
//            denormal range.  For the packed forms the mask is taken per element (both of a pair; elements 0, 1 and 31 of 32): equal masks with
//            ONE operand mean the elements share the word.
//   follows  whether the instruction fed t << A reproduces the definition (magnitude hi iff floor(f * 2^24) + t >= 2^24) for the alignment A:
//            for A = 0 .. 8, mismatches are counted per class of input -- normal range, denormal range, exactly representable, at the top,
//            above the top (clipped by the nearest scale rule, absent under the headroom rule), infinity, NaN -- over every code interval of
//            the format, 33 fractions per interval chosen around the thresholds t drawn, both signs, scale bytes 127, 1 and 254.
// The tables this prints are recorded in DESIGN.md (section 4e, "Stochastic rounding").
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));

enum { FP4 = 0, FP8 = 1, E2M3 = 2, E3M2 = 3 };
static const char* kName[4] = {"FP4 E2M1 (sr_pk_fp4_f32)", "FP8 E4M3 (sr_fp8_f32)", "FP6 E2M3 (sr_pk32_fp6_f32)", "FP6 E3M2 (sr_pk32_bf6_f32)"};

// out[i] = code of x[i] under rand[i] and the scale operand, placed in element `slot` of the packed forms (the other elements +0)
template <int FMT>
__global__ void k_convert(const float* x, const uint32_t* rnd, const uint32_t* scale_bits, const int* slot, uint32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float sc = __uint_as_float(scale_bits[i]);
    if constexpr (FMT == FP4) {
        const f32x2 p {slot[i] == 0 ? x[i] : 0.f, slot[i] == 1 ? x[i] : 0.f};
        out[i] = (__builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, p, rnd[i], sc, 0) >> (4 * slot[i])) & 0xfu;
    } else if constexpr (FMT == FP8) {
        out[i] = static_cast<uint32_t>(__builtin_amdgcn_cvt_scalef32_sr_fp8_f32(0, x[i], rnd[i], sc, 0)) & 0xffu;
    } else {
        f32x32 v;
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] = j == slot[i] ? x[i] : 0.f;
        u32x6 c;
        if constexpr (FMT == E2M3) c = __builtin_amdgcn_cvt_scalef32_sr_pk32_fp6_f32(v, rnd[i], sc);
        else c = __builtin_amdgcn_cvt_scalef32_sr_pk32_bf6_f32(v, rnd[i], sc);
        const int bit = 6 * slot[i];
        const uint64_t two = static_cast<uint64_t>(c[bit / 32]) | (static_cast<uint64_t>(bit / 32 + 1 < 6 ? c[bit / 32 + 1] : 0u) << 32);
        out[i] = static_cast<uint32_t>(two >> (bit % 32)) & 0x3fu;
    }
}

struct Format {
    int mbits, emin, ncodes;   // mantissa bits, exponent of the smallest normal, number of non-negative finite codes
    uint32_t sign, nan;
};
static const Format kFmt[4] = {{1, 0, 8, 0x8, 0x0}, {3, -6, 127, 0x80, 0x7f}, {3, 0, 32, 0x20, 0x0}, {2, -2, 32, 0x20, 0x0}};

static double magnitude(int fmt, int c) {
    const Format& f = kFmt[fmt];
    const int e = c >> f.mbits, m = c & ((1 << f.mbits) - 1);
    return e == 0 ? std::ldexp(m, f.emin - f.mbits) : std::ldexp((1 << f.mbits) + m, e - 1 + f.emin - f.mbits);
}

static uint32_t mix32(uint32_t h) {
    h ^= h >> 16; h *= 0x21f0aaadu; h ^= h >> 15; h *= 0x735a2d97u; h ^= h >> 15;
    return h;
}

// the definition on a scaled value v >= 0 (sign apart): the code, or -1 when v is above the top (the headroom rule never produces that)
static int define(int fmt, double v, uint32_t t) {
    const Format& f = kFmt[fmt];
    if (v > magnitude(fmt, f.ncodes - 1)) return -1;
    int k = 0;
    while (k + 1 < f.ncodes && magnitude(fmt, k + 1) <= v) ++k;
    if (k + 1 == f.ncodes) return k;
    const double fr = (v - magnitude(fmt, k)) / (magnitude(fmt, k + 1) - magnitude(fmt, k));
    return k + (std::floor(fr * 16777216.0) + t >= 16777216.0 ? 1 : 0);
}

struct Case {
    float x;
    uint32_t rnd, scale_bits;
    int slot;
};

static std::vector<uint32_t> run(int fmt, const std::vector<Case>& cases) {
    const int n = static_cast<int>(cases.size());
    std::vector<float> x(n);
    std::vector<uint32_t> r(n), s(n), out(n);
    std::vector<int> slot(n);
    for (int i = 0; i < n; ++i) { x[i] = cases[i].x; r[i] = cases[i].rnd; s[i] = cases[i].scale_bits; slot[i] = cases[i].slot; }
    float* dx; uint32_t *dr, *ds, *dout; int* dslot;
    hipMalloc(&dx, n * 4); hipMalloc(&dr, n * 4); hipMalloc(&ds, n * 4); hipMalloc(&dslot, n * 4); hipMalloc(&dout, n * 4);
    hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice); hipMemcpy(dr, r.data(), n * 4, hipMemcpyHostToDevice);
    hipMemcpy(ds, s.data(), n * 4, hipMemcpyHostToDevice); hipMemcpy(dslot, slot.data(), n * 4, hipMemcpyHostToDevice);
    const dim3 grid((n + 255) / 256), block(256);
    if (fmt == FP4) hipLaunchKernelGGL(k_convert<FP4>, grid, block, 0, 0, dx, dr, ds, dslot, dout, n);
    if (fmt == FP8) hipLaunchKernelGGL(k_convert<FP8>, grid, block, 0, 0, dx, dr, ds, dslot, dout, n);
    if (fmt == E2M3) hipLaunchKernelGGL(k_convert<E2M3>, grid, block, 0, 0, dx, dr, ds, dslot, dout, n);
    if (fmt == E3M2) hipLaunchKernelGGL(k_convert<E3M2>, grid, block, 0, 0, dx, dr, ds, dslot, dout, n);
    hipMemcpy(out.data(), dout, n * 4, hipMemcpyDeviceToHost);
    hipFree(dx); hipFree(dr); hipFree(ds); hipFree(dslot); hipFree(dout);
    return out;
}

static void probe_bits(int fmt) {
    const Format& f = kFmt[fmt];
    const int slots[3] = {0, 1, fmt >= E2M3 ? 31 : 1}, nslots = fmt == FP8 ? 1 : fmt == FP4 ? 2 : 3;
    // just below code 2^mbits + 1 (normal range: every discarded bit set) and just below code 1 (denormal range)
    const float below[2] = {std::nextafterf(static_cast<float>(magnitude(fmt, (1 << f.mbits) + 1)), 0.f), std::nextafterf(static_cast<float>(magnitude(fmt, 1)), 0.f)};
    const int lower[2] = {1 << f.mbits, 0};
    std::vector<Case> cases;
    for (int which = 0; which < 2; ++which)
        for (int sl = 0; sl < nslots; ++sl)
            for (int b = 0; b < 32; ++b) cases.push_back({below[which], 1u << b, 127u << 23, slots[sl]});
    const std::vector<uint32_t> got = run(fmt, cases);
    size_t i = 0;
    for (int which = 0; which < 2; ++which)
        for (int sl = 0; sl < nslots; ++sl) {
            uint32_t up = 0, other = 0;
            for (int b = 0; b < 32; ++b, ++i) {
                if (static_cast<int>(got[i]) == lower[which] + 1) up |= 1u << b;
                else if (static_cast<int>(got[i]) != lower[which]) other |= 1u << b;
            }
            std::printf("  bits    %-8s element %2d: operand bits that carry 1 - ulp up: %08x   (neither lo nor hi under: %08x)\n", which ? "denormal" : "normal",
                        slots[sl], up, other);
        }
}

static void probe_follows(int fmt) {
    const Format& f = kFmt[fmt];
    const int top = f.ncodes - 1;
    std::vector<Case> cases;
    std::vector<uint32_t> ts;
    std::vector<std::string> cls;
    uint32_t counter = 0;
    auto add = [&](double v, int s, const char* c) {   // v of the scaled domain under scale byte s, both signs, every alignment
        const double d = std::ldexp(v, s - 127);
        const float x = static_cast<float>(d);
        if (std::isfinite(v) && (static_cast<double>(x) != d || !std::isfinite(x))) return;   // only points the scaling represents exactly
        const uint32_t t = mix32(counter++) >> 8;
        for (float g : {x, -x})
            for (uint32_t a = 0; a <= 8; ++a) { cases.push_back({g, t << a, static_cast<uint32_t>(s) << 23, 0}); ts.push_back(t); cls.push_back(c); }
    };
    for (int s : {127, 1, 254}) {
        for (int c = 0; c < top; ++c) {
            const double lo = magnitude(fmt, c), hi = magnitude(fmt, c + 1);
            const char* name = c < (1 << f.mbits) ? "denormal range" : "normal range";
            add(lo, s, "representable");
            for (int j = 0; j < 33; ++j) {   // fractions with floor(f * 2^24) at, just below and around 2^24 - t for the t this case draws
                const uint32_t t = mix32(counter) >> 8;
                const double need = 16777216.0 - t + (j % 3 - 1) * std::ldexp(1.0, (j / 3) * 2);
                if (need <= 0 || need >= 16777216.0) continue;
                add(lo + (hi - lo) * need / 16777216.0, s, name);
            }
        }
        add(magnitude(fmt, top), s, "at the top");
        add(magnitude(fmt, top) * 1.03, s, "above the top");
        add(magnitude(fmt, top) * 1.3, s, "above the top");
        add(INFINITY, s, "infinity");
        add(NAN, s, "NaN");
    }
    const std::vector<uint32_t> got = run(fmt, cases);
    std::map<std::string, std::vector<long>> tally;   // class -> cases, mismatches at A = 0 .. 8
    for (size_t i = 0; i < cases.size(); ++i) {
        const int a = static_cast<int>(i % 9), s = static_cast<int>(cases[i].scale_bits >> 23);
        const float x = cases[i].x;
        uint32_t want;
        if (std::isnan(x)) want = f.nan;
        else if (std::isinf(x)) want = top;
        else {
            const int c = define(fmt, std::fabs(std::ldexp(static_cast<double>(x), 127 - s)), ts[i]);
            want = c < 0 ? top : c;   // above the top: the nearest call's saturation, for the record
        }
        if (!std::isnan(x) && std::signbit(x)) want |= f.sign;
        const bool nan_ok = std::isnan(x) && fmt == FP8 && (got[i] & 0x7f) == 0x7f;
        auto& row = tally[cls[i]];
        row.resize(10);
        if (a == 0) ++row[0];
        if (!nan_ok && got[i] != want) ++row[1 + a];
    }
    for (const auto& kv : tally) {
        std::printf("  follows %-16s %6ld cases; mismatches with t << A, A = 0 .. 8:", kv.first.c_str(), kv.second[0]);
        for (int a = 0; a <= 8; ++a) std::printf(" %5ld", kv.second[1 + a]);
        std::printf("\n");
    }
}

int main() {
    for (int fmt = 0; fmt < 4; ++fmt) {
        std::printf("%s\n", kName[fmt]);
        probe_bits(fmt);
        probe_follows(fmt);
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
