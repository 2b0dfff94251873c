// Probe: what the gfx950 FP6 scaled conversions (v_cvt_scalef32_2xpk16_{fp6,bf6}_f32, ..._pk32_{fp6,bf6}_bf16, ..._pk32_{f32,bf16}_{fp6,bf6}) do at
// the edges of the MXFP6 definition of include/piquant_hip.h, and how their 6 dwords are laid out.  The sibling of probe_mx_cvt.hip.  Not a test.
//   hipcc --offload-arch=gfx950 -O2 tools/probe_mx_fp6_cvt.hip -o tools/probe_mx_fp6_cvt && ./tools/probe_mx_fp6_cvt
// Layout: a block whose 32 slots hold 32 different code values (encode) or codes (decode); the 6 dwords are read as the dense little-endian string of
// 6-bit fields of the definition and the slot each field came from is printed ("identity" when field j is slot j; for 2xpk16 slot j < 16 is element j
// of the first operand, slot 16 + j element j of the second).  Edges: one value in all 32 slots of a block, every interesting point of the scaled
// domain (all midpoints between adjacent codes, the codes, their neighbours in the input type, the saturation line and far above it) under a spread
// of scale bytes, plus NaN, infinities, zeros and denormals; the model is the definition in double.  Decode: every code under every scale byte.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef __bf16 bf16x32 __attribute__((ext_vector_type(32)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

template <int FMT, bool BF16>   // FMT 2: E2M3 (fp6), 3: E3M2 (bf6); x: 32 values a case (float32 bits, or bfloat16 bits in the low half)
__global__ void k_encode(const uint32_t* x, const uint32_t* scale_bits, uint32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float sc = __uint_as_float(scale_bits[i]);
    u32x6 r;
    if constexpr (BF16) {
        bf16x32 v;
        for (int j = 0; j < 32; ++j) v[j] = __builtin_bit_cast(__bf16, static_cast<uint16_t>(x[i * 32 + j]));
        if constexpr (FMT == 2) r = __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(v, sc);
        else r = __builtin_amdgcn_cvt_scalef32_pk32_bf6_bf16(v, sc);
    } else {
        f32x16 a, b;
        for (int j = 0; j < 16; ++j) {
            a[j] = __uint_as_float(x[i * 32 + j]);
            b[j] = __uint_as_float(x[i * 32 + 16 + j]);
        }
        if constexpr (FMT == 2) r = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, sc);
        else r = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, sc);
    }
    for (int j = 0; j < 6; ++j) out[i * 6 + j] = r[j];
}

template <int FMT, bool BF16>   // codes: 6 dwords a case; out: 32 float32 bits (or bfloat16 bits) a case
__global__ void k_decode(const uint32_t* codes, const uint32_t* scale_bits, uint32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float sc = __uint_as_float(scale_bits[i]);
    u32x6 c;
    for (int j = 0; j < 6; ++j) c[j] = codes[i * 6 + j];
    if constexpr (BF16) {
        bf16x32 r;
        if constexpr (FMT == 2) r = __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, sc);
        else r = __builtin_amdgcn_cvt_scalef32_pk32_bf16_bf6(c, sc);
        const u32x16 w = __builtin_bit_cast(u32x16, r);   // as the kernels take it: 16 dwords, element 2 j in the low half of dword j
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            out[i * 32 + 2 * j] = w[j] & 0xffffu;
            out[i * 32 + 2 * j + 1] = w[j] >> 16;
        }
    } else {
        f32x32 r;
        if constexpr (FMT == 2) r = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(c, sc);
        else r = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(c, sc);
        for (int j = 0; j < 32; ++j) out[i * 32 + j] = __float_as_uint(r[j]);
    }
}

static double code_value(int fmt, uint32_t c) {
    double v;
    if (fmt == 2) {
        const int e = (c >> 3) & 3, m = c & 7;
        v = e == 0 ? m / 8.0 : std::ldexp(8 + m, e - 4);
    } else {
        const int e = (c >> 2) & 7, m = c & 3;
        v = e == 0 ? m / 16.0 : std::ldexp(4 + m, e - 5);
    }
    return c & 0x20 ? -v : v;
}

static uint32_t model_encode(int fmt, float x, int s) {   // steps 4-7 of the definition
    if (std::isnan(x)) return 0u;
    const uint32_t sign = std::signbit(x) ? 0x20u : 0u;
    if (std::isinf(x)) return sign | 0x1fu;
    const double v = std::fabs(std::ldexp(static_cast<double>(x), 127 - s));
    int best = 0;
    for (int c = 1; c <= 0x1f; ++c) {
        const double lo = code_value(fmt, best), hi = code_value(fmt, c), mid = 0.5 * (lo + hi);
        if (v > mid || (v == mid && (c & 1) == 0)) best = c;
    }
    return sign | best;
}

static float model_decode(int fmt, uint32_t c, int s) {
    if (s == 255) return NAN;
    const double d = std::ldexp(code_value(fmt, c), s - 127);
    if (std::fabs(d) > 3.4028235677973366e38) return std::signbit(d) ? -INFINITY : INFINITY;   // past the largest float32 + half an ulp
    return static_cast<float>(d);
}

static uint32_t f32_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float bits_f32(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static uint16_t bf16_rne(float f) {
    const uint32_t u = f32_bits(f);
    if (std::isnan(f)) return 0x7fc0;
    return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static uint32_t field(const uint32_t* w, int j) {   // bits [6 j, 6 j + 6) of the little-endian string of the 6 dwords
    const int bit = 6 * j;
    const uint64_t two = w[bit >> 5] | (static_cast<uint64_t>((bit >> 5) + 1 < 6 ? w[(bit >> 5) + 1] : 0u) << 32);
    return static_cast<uint32_t>(two >> (bit & 31)) & 0x3fu;
}

static void set_field(uint32_t* w, int j, uint32_t c) {
    for (int k = 0; k < 6; ++k)
        if ((c >> k) & 1u) w[(6 * j + k) >> 5] |= 1u << ((6 * j + k) & 31);
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

static const char* fmt_name(int fmt) { return fmt == 2 ? "FP6 E2M3" : "FP6 E3M2"; }

template <class T>
static T* to_device(const std::vector<T>& v) {
    T* d;
    hipMalloc(&d, v.size() * sizeof(T));
    hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}

static std::vector<uint32_t> run_encode(int fmt, bool bf16, const std::vector<uint32_t>& x, const std::vector<uint32_t>& sb) {
    const int n = static_cast<int>(sb.size());
    uint32_t *dx = to_device(x), *ds = to_device(sb), *dout;
    hipMalloc(&dout, n * 24);
    const dim3 grid((n + 63) / 64), block(64);
    if (fmt == 2 && !bf16) hipLaunchKernelGGL((k_encode<2, false>), grid, block, 0, 0, dx, ds, dout, n);
    if (fmt == 2 && bf16) hipLaunchKernelGGL((k_encode<2, true>), grid, block, 0, 0, dx, ds, dout, n);
    if (fmt == 3 && !bf16) hipLaunchKernelGGL((k_encode<3, false>), grid, block, 0, 0, dx, ds, dout, n);
    if (fmt == 3 && bf16) hipLaunchKernelGGL((k_encode<3, true>), grid, block, 0, 0, dx, ds, dout, n);
    std::vector<uint32_t> got(static_cast<size_t>(n) * 6);
    hipMemcpy(got.data(), dout, got.size() * 4, hipMemcpyDeviceToHost);
    hipFree(dx); hipFree(ds); hipFree(dout);
    return got;
}

static std::vector<uint32_t> run_decode(int fmt, bool bf16, const std::vector<uint32_t>& codes, const std::vector<uint32_t>& sb) {
    const int n = static_cast<int>(sb.size());
    uint32_t *dc = to_device(codes), *ds = to_device(sb), *dout;
    hipMalloc(&dout, static_cast<size_t>(n) * 128);
    const dim3 grid((n + 63) / 64), block(64);
    if (fmt == 2 && !bf16) hipLaunchKernelGGL((k_decode<2, false>), grid, block, 0, 0, dc, ds, dout, n);
    if (fmt == 2 && bf16) hipLaunchKernelGGL((k_decode<2, true>), grid, block, 0, 0, dc, ds, dout, n);
    if (fmt == 3 && !bf16) hipLaunchKernelGGL((k_decode<3, false>), grid, block, 0, 0, dc, ds, dout, n);
    if (fmt == 3 && bf16) hipLaunchKernelGGL((k_decode<3, true>), grid, block, 0, 0, dc, ds, dout, n);
    std::vector<uint32_t> got(static_cast<size_t>(n) * 32);
    hipMemcpy(got.data(), dout, got.size() * 4, hipMemcpyDeviceToHost);
    hipFree(dc); hipFree(ds); hipFree(dout);
    return got;
}

static void print_perm(const char* what, const int (&perm)[32]) {
    bool identity = true;
    for (int j = 0; j < 32; ++j) identity = identity && perm[j] == j;
    std::printf("layout %s: %s", what, identity ? "identity" : "NOT the definition's string; field j <- slot");
    if (!identity)
        for (int j = 0; j < 32; ++j) std::printf(" %d", perm[j]);
    std::printf("\n");
}

static void probe_layout(int fmt, bool bf16) {
    // encode: slot i holds the value of code (2 i + 1) % 64 -- 32 different codes of both signs -- under s = 127
    std::vector<uint32_t> x(32), sb {127u << 23};
    for (int i = 0; i < 32; ++i) {
        const float f = static_cast<float>(code_value(fmt, (2 * i + 1) % 64));
        x[i] = bf16 ? f32_bits(f) >> 16 : f32_bits(f);
    }
    const std::vector<uint32_t> enc = run_encode(fmt, bf16, x, sb);
    int perm[32];
    for (int j = 0; j < 32; ++j) {
        const uint32_t c = field(enc.data(), j);
        perm[j] = (c & 1u) ? static_cast<int>(c - 1) / 2 : -1;
    }
    std::printf("%s %s raw dwords: %08x %08x %08x %08x %08x %08x\n", fmt_name(fmt), bf16 ? "bfloat16" : "float32", enc[0], enc[1], enc[2], enc[3], enc[4], enc[5]);
    print_perm(bf16 ? "encode pk32 from bfloat16" : "encode 2xpk16 from float32", perm);
    // decode: field j holds code (2 j + 1) % 64
    std::vector<uint32_t> codes(6, 0u);
    for (int j = 0; j < 32; ++j) set_field(codes.data(), j, (2 * j + 1) % 64);
    const std::vector<uint32_t> dec = run_decode(fmt, bf16, codes, sb);
    for (int i = 0; i < 32; ++i) {
        perm[i] = -1;
        for (int j = 0; j < 32; ++j) {
            const float want = static_cast<float>(code_value(fmt, (2 * j + 1) % 64));
            if (dec[i] == (bf16 ? f32_bits(want) >> 16 : f32_bits(want))) perm[i] = j;
        }
    }
    print_perm(bf16 ? "decode pk32 to bfloat16 (slot i <- field)" : "decode pk32 to float32 (slot i <- field)", perm);
}

static void probe_encode(int fmt, bool bf16) {
    const double vmax = code_value(fmt, 0x1f);
    std::vector<double> t;   // points of the scaled domain, positive
    for (int c = 0; c < 0x1f; ++c) {
        t.push_back(0.5 * (code_value(fmt, c) + code_value(fmt, c + 1)));
        t.push_back(code_value(fmt, c + 1));
    }
    for (double k : {1.03, 1.0625, 1.14, 1.2, 1.3333, 1.9999, 2.0, 4.0, 1e3, 1e6, 1e12}) t.push_back(vmax * k);
    for (double k : {1e-3, 1e-6, 1e-12, 1e-30}) t.push_back(code_value(fmt, 1) * k);
    auto in_type = [&](float f) { return bf16 ? bits_f32(static_cast<uint32_t>(bf16_rne(f)) << 16) : f; };
    auto step = [&](float f, int dir) {   // the neighbour of a positive finite f in the input type
        const uint32_t u = f32_bits(f), ulp = bf16 ? 0x10000u : 1u;
        return bits_f32(dir > 0 ? u + ulp : u - ulp);
    };
    std::vector<float> xs;
    std::vector<int> ss;
    for (int s = 0; s < 255; ++s) {
        if (!(s < 4 || s > 248 || s % 16 == 7 || (s >= 118 && s <= 136))) continue;
        auto push = [&](float f) { for (float g : {f, -f}) { xs.push_back(g); ss.push_back(s); } };
        for (double tv : t) {
            const double d = std::ldexp(tv, s - 127);
            if (!(d < 3.3e38)) continue;
            const float f = in_type(static_cast<float>(d));
            if (f == 0.f || !std::isfinite(f)) continue;
            push(f);
            if (f32_bits(f) > (bf16 ? 0x10000u : 1u)) push(step(f, -1));
            if (std::isfinite(step(f, +1))) push(step(f, +1));
        }
        push(NAN); push(INFINITY); push(0.f); push(in_type(3.3e38f));
        for (uint32_t bits : {0x10000u, 0x20000u, 0x30000u, 0x400000u, 0x7f0000u, 0x800000u}) push(bits_f32(bits));
        if (!bf16)
            for (uint32_t bits : {1u, 2u, 3u, 0x7fffffu}) push(bits_f32(bits));
    }
    const int n = static_cast<int>(xs.size());
    std::vector<uint32_t> x(static_cast<size_t>(n) * 32), sb(n);
    for (int i = 0; i < n; ++i) {
        sb[i] = static_cast<uint32_t>(ss[i]) << 23;
        for (int j = 0; j < 32; ++j) x[static_cast<size_t>(i) * 32 + j] = bf16 ? f32_bits(xs[i]) >> 16 : f32_bits(xs[i]);
    }
    const std::vector<uint32_t> got = run_encode(fmt, bf16, x, sb);
    Tally tally;
    for (int i = 0; i < n; ++i) {
        const int s = ss[i];
        const uint32_t want = model_encode(fmt, xs[i], s);
        bool bad = false;
        uint32_t g0 = field(&got[static_cast<size_t>(i) * 6], 0), gbad = g0;
        for (int j = 0; j < 32; ++j) {
            const uint32_t g = field(&got[static_cast<size_t>(i) * 6], j);
            if (g != want) { bad = true; gbad = g; }
        }
        const double v = std::fabs(std::ldexp(static_cast<double>(xs[i]), 127 - s));
        std::string cls = std::isnan(xs[i]) ? "nan" : std::isinf(xs[i]) ? "inf" : (xs[i] != 0.f && std::fabs(xs[i]) < 1.17549435e-38f) ? "denormal input" :
                          v > vmax ? "above max" : "in range";
        if (s == 0) cls += ", s=0";
        tally.add(cls, bad, "x=%a (bits %08x) s=%d scaled=%g: got %02x (slot 0: %02x), definition %02x", xs[i], f32_bits(xs[i]), s,
                  std::ldexp(static_cast<double>(xs[i]), 127 - s), gbad, g0, want);
    }
    std::printf("encode %s from %s: %d cases\n", fmt_name(fmt), bf16 ? "bfloat16" : "float32", n);
    tally.print();
}

static void probe_decode(int fmt, bool bf16) {
    const int n = 64 * 256;
    std::vector<uint32_t> codes(static_cast<size_t>(n) * 6, 0u), sb(n);
    for (int i = 0; i < n; ++i) {
        sb[i] = static_cast<uint32_t>(i & 255) << 23;
        for (int j = 0; j < 32; ++j) set_field(&codes[static_cast<size_t>(i) * 6], j, i >> 8);
    }
    const std::vector<uint32_t> got = run_decode(fmt, bf16, codes, sb);
    Tally tally;
    for (int i = 0; i < n; ++i) {
        const uint32_t c = i >> 8;
        const int s = i & 255;
        const float want = model_decode(fmt, c, s);
        const uint32_t wb = bf16 ? bf16_rne(want) : f32_bits(want);
        bool bad = false;
        uint32_t g = got[static_cast<size_t>(i) * 32];
        for (int j = 0; j < 32; ++j) {
            const uint32_t gj = got[static_cast<size_t>(i) * 32 + j];
            const bool got_nan = bf16 ? ((gj & 0x7fffu) > 0x7f80u) : ((gj & 0x7fffffffu) > 0x7f800000u);
            if (std::isnan(want) ? !got_nan : gj != wb) { bad = true; g = gj; }
        }
        std::string cls = s == 255 ? "s=255" : s == 0 ? "s=0" : std::isinf(want) ? "overflow" : (want != 0.f && std::fabs(want) < 1.17549435e-38f) ? "denormal result" : want == 0.f ? "zero" :
                          "normal result";
        tally.add(cls, bad, "code %02x s=%d: got %08x, definition %08x (%a)", c, s, g, wb, want);
    }
    std::printf("decode %s -> %s: %d cases\n", fmt_name(fmt), bf16 ? "bfloat16" : "float32", n);
    tally.print();
}

int main() {
    for (int fmt : {2, 3})
        for (bool bf16 : {false, true}) probe_layout(fmt, bf16);
    for (int fmt : {2, 3})
        for (bool bf16 : {false, true}) probe_encode(fmt, bf16);
    for (int fmt : {2, 3})
        for (bool bf16 : {false, true}) probe_decode(fmt, bf16);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
