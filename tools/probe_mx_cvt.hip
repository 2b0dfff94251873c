// Probe: what the gfx950 scaled conversions (v_cvt_scalef32_pk_{fp4,fp8}_f32, ..._pk_f32_{fp4,fp8}, ..._pk_bf16_{fp4,fp8}) do at the edges of the MX
// definition of include/piquant_hip.h: saturation, NaN, infinities, denormal inputs, a zero / denormal / all-ones scale exponent.  Not a test.
//   hipcc --offload-arch=gfx950 -O2 tools/probe_mx_cvt.hip -o tools/probe_mx_cvt && ./tools/probe_mx_cvt
// Encode: the scale operand is the float with bits s << 23 (2^(s - 127); +0.0 at s = 0), the input x = t * 2^(s - 127) for every interesting point t
// of the scaled domain (all midpoints between adjacent codes and their float32 neighbours, the saturation line, far above it) plus NaN, infinities,
// zeros and denormals; the model is the definition in double.  Decode: every code under every scale byte.  Mismatches are counted per class and the
// first few of each class printed.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

template <int FMT>   // 0: FP4 E2M1, 1: FP8 E4M3; out = code of x in the low field, code of the same x in the next field << 8
__global__ void k_encode(const float* x, const uint32_t* scale_bits, uint32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float sc = __uint_as_float(scale_bits[i]);
    if constexpr (FMT == 0) {
        const uint32_t r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, x[i], x[i], sc, 0);
        out[i] = (r & 0xfu) | (((r >> 4) & 0xfu) << 8);
    } else {
        const s16x2 r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(s16x2 {0, 0}, x[i], x[i], sc, false);
        out[i] = static_cast<uint16_t>(r[0]);
    }
}

template <int FMT, bool BF16>   // out[c * 256 + s] = float32 bits (or bfloat16 bits) of code c under scale byte s
__global__ void k_decode(uint32_t* out, int ncodes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncodes * 256) return;
    const uint32_t c = i >> 8;
    const float sc = __uint_as_float(static_cast<uint32_t>(i & 255) << 23);
    if constexpr (BF16) {
        bf16x2 r;
        if constexpr (FMT == 0) r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0);
        else r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, sc, false);
        out[i] = __builtin_bit_cast(uint16_t, r[0]);
    } else {
        f32x2 r;
        if constexpr (FMT == 0) r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, sc, 0);
        else r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c, sc, false);
        out[i] = __float_as_uint(r[0]);
    }
}

static double code_value(int fmt, uint32_t c) {   // NaN codes of E4M3: NAN
    if (fmt == 0) {
        static const double t[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
        return (c & 8 ? -1.0 : 1.0) * t[c & 7];
    }
    const int e = (c >> 3) & 15, m = c & 7;
    if (e == 15 && m == 7) return NAN;
    const double v = e == 0 ? std::ldexp(m, -9) : std::ldexp(8 + m, e - 10);
    return c & 0x80 ? -v : v;
}

static uint32_t model_encode(int fmt, float x, int s) {   // steps 4-7 of the definition
    const uint32_t sign = std::signbit(x) ? (fmt == 0 ? 8u : 0x80u) : 0u;
    if (std::isnan(x)) return fmt == 0 ? 0u : 0x7fu;
    const int top = fmt == 0 ? 7 : 0x7e;
    if (std::isinf(x)) return sign | top;
    const double v = std::fabs(std::ldexp(static_cast<double>(x), 127 - s));
    int best = 0;
    for (int c = 1; c <= top; ++c) {
        const double lo = code_value(fmt, best), hi = code_value(fmt, c), mid = 0.5 * (lo + hi);
        if (v > mid || (v == mid && (c & 1) == 0)) best = c;
    }
    return sign | best;
}

static float model_decode(int fmt, uint32_t c, int s) {
    const double v = code_value(fmt, c);
    if (s == 255 || std::isnan(v)) return NAN;
    const double d = std::ldexp(v, s - 127);
    if (std::fabs(d) > 3.4028235677973366e38) return std::signbit(d) ? -INFINITY : INFINITY;   // past the largest float32 + half an ulp
    return static_cast<float>(d);
}

static uint16_t bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if (std::isnan(f)) return 0x7fc0;
    return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

struct Tally {
    std::map<std::string, std::pair<long, long>> n;   // class -> {cases, mismatches}
    void add(const std::string& cls, bool bad, const char* fmt, ...) __attribute__((format(printf, 4, 5))) {
        auto& e = n[cls];
        ++e.first;
        if (!bad) return;
        if (++e.second <= 6) {
            va_list ap;
            va_start(ap, fmt);
            std::printf("    [%s] ", cls.c_str());
            std::vprintf(fmt, ap);
            std::printf("\n");
            va_end(ap);
        }
    }
    void print() const {
        for (const auto& kv : n) std::printf("  %-22s %8ld cases, %8ld mismatches\n", kv.first.c_str(), kv.second.first, kv.second.second);
    }
};

static void probe_encode(int fmt) {
    const int top = fmt == 0 ? 7 : 0x7e;
    const double vmax = code_value(fmt, top);
    std::vector<float> t;   // points of the scaled domain, positive
    for (int c = 0; c < top; ++c) {
        const float mid = static_cast<float>(0.5 * (code_value(fmt, c) + code_value(fmt, c + 1)));
        for (float f : {std::nextafterf(mid, 0.f), mid, std::nextafterf(mid, 1e9f), static_cast<float>(code_value(fmt, c + 1))}) t.push_back(f);
    }
    for (double k : {1.0, 1.0625, 1.14, 1.2, 1.3333, 1.9999, 2.0, 4.0, 1e3, 1e6, 1e12})
        t.push_back(static_cast<float>(vmax * k));
    t.push_back(std::nextafterf(static_cast<float>(vmax), 1e9f));
    for (double k : {1e-3, 1e-6, 1e-12, 1e-30}) t.push_back(static_cast<float>(code_value(fmt, 1) * k));
    std::vector<float> x;
    std::vector<uint32_t> sb;
    std::vector<int> ss;
    for (int s = 0; s < 256; ++s) {
        if (!(s < 4 || s > 250 || s % 16 == 7 || (s >= 118 && s <= 136))) continue;
        auto push = [&](float f) { for (float g : {f, -f}) { x.push_back(g); sb.push_back(static_cast<uint32_t>(s) << 23); ss.push_back(s); } };
        for (float tv : t) {
            const double d = std::ldexp(static_cast<double>(tv), s - 127);
            const float f = static_cast<float>(d);
            if (std::fabs(d) < 3.4e38 && static_cast<double>(f) == d) push(f);   // only points the scaling represents exactly
        }
        push(NAN); push(INFINITY); push(0.f); push(3.4028234663852886e38f);
        for (uint32_t bits : {1u, 2u, 3u, 0x400000u, 0x7fffffu, 0x800000u}) push(__builtin_bit_cast(float, bits));
    }
    const int n = static_cast<int>(x.size());
    float* dx; uint32_t *ds, *dout;
    hipMalloc(&dx, n * 4); hipMalloc(&ds, n * 4); hipMalloc(&dout, n * 4);
    hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice);
    hipMemcpy(ds, sb.data(), n * 4, hipMemcpyHostToDevice);
    if (fmt == 0) hipLaunchKernelGGL(k_encode<0>, dim3((n + 255) / 256), dim3(256), 0, 0, dx, ds, dout, n);
    else hipLaunchKernelGGL(k_encode<1>, dim3((n + 255) / 256), dim3(256), 0, 0, dx, ds, dout, n);
    std::vector<uint32_t> got(n);
    hipMemcpy(got.data(), dout, n * 4, hipMemcpyDeviceToHost);
    Tally tally;
    for (int i = 0; i < n; ++i) {
        const int s = ss[i];
        const uint32_t want = model_encode(fmt, x[i], s);
        uint32_t g0 = got[i] & 0xffu, g1 = fmt == 0 ? (got[i] >> 8) & 0xffu : (got[i] >> 8) & 0xffu;
        const bool nan_ok = fmt == 1 && std::isnan(x[i]) && (g0 & 0x7f) == 0x7f && (g1 & 0x7f) == 0x7f;
        const bool bad = !nan_ok && (g0 != want || g1 != want);
        const double v = std::fabs(std::ldexp(static_cast<double>(x[i]), 127 - s));
        std::string cls = std::isnan(x[i]) ? "nan" : std::isinf(x[i]) ? "inf" : (x[i] != 0.f && std::fabs(x[i]) < 1.17549435e-38f) ? "denormal input" : v > vmax ? "above max" : "in range";
        if (s == 0) cls += ", s=0";
        else if (s == 255) cls += ", s=255";
        tally.add(cls, bad, "x=%a (bits %08x) s=%d scaled=%g: got %02x / %02x, definition %02x", x[i], __builtin_bit_cast(uint32_t, x[i]), s,
                  std::ldexp(static_cast<double>(x[i]), 127 - s), g0, g1, want);
    }
    std::printf("encode %s: %d cases\n", fmt == 0 ? "FP4 E2M1" : "FP8 E4M3", n);
    tally.print();
    hipFree(dx); hipFree(ds); hipFree(dout);
}

static void probe_decode(int fmt, bool bf16) {
    const int ncodes = fmt == 0 ? 16 : 256, n = ncodes * 256;
    uint32_t* dout;
    hipMalloc(&dout, n * 4);
    const dim3 grid((n + 255) / 256), block(256);
    if (fmt == 0 && !bf16) hipLaunchKernelGGL((k_decode<0, false>), grid, block, 0, 0, dout, ncodes);
    if (fmt == 0 && bf16) hipLaunchKernelGGL((k_decode<0, true>), grid, block, 0, 0, dout, ncodes);
    if (fmt == 1 && !bf16) hipLaunchKernelGGL((k_decode<1, false>), grid, block, 0, 0, dout, ncodes);
    if (fmt == 1 && bf16) hipLaunchKernelGGL((k_decode<1, true>), grid, block, 0, 0, dout, ncodes);
    std::vector<uint32_t> got(n);
    hipMemcpy(got.data(), dout, n * 4, hipMemcpyDeviceToHost);
    Tally tally;
    for (int i = 0; i < n; ++i) {
        const uint32_t c = i >> 8;
        const int s = i & 255;
        const float want = model_decode(fmt, c, s);
        uint32_t wb = __builtin_bit_cast(uint32_t, want);
        if (bf16) wb = bf16_rne(want);
        const bool want_nan = std::isnan(want);
        const bool got_nan = bf16 ? ((got[i] & 0x7fffu) > 0x7f80u) : ((got[i] & 0x7fffffffu) > 0x7f800000u);
        const bool bad = want_nan ? !got_nan : got[i] != wb;
        const float fw = std::fabs(want);
        std::string cls = s == 255 ? "s=255" : std::isnan(code_value(fmt, c)) ? "nan code" : s == 0 ? "s=0" : std::isinf(want) ? "overflow" :
                          (want != 0.f && fw < (bf16 ? 1.17549435e-38f : 1.17549435e-38f)) ? "denormal result" : want == 0.f ? "zero" : "normal result";
        tally.add(cls, bad, "code %02x s=%d: got %08x, definition %08x (%a)", c, s, got[i], wb, want);
    }
    std::printf("decode %s -> %s: %d cases\n", fmt == 0 ? "FP4 E2M1" : "FP8 E4M3", bf16 ? "bfloat16" : "float32", n);
    tally.print();
    hipFree(dout);
}

int main() {
    for (int fmt : {0, 1}) probe_encode(fmt);
    for (int fmt : {0, 1})
        for (bool bf16 : {false, true}) probe_decode(fmt, bf16);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
