// Stand-alone stress program for the worker pool of libpiquant_cpu.so (csrc/cpu/piquant_cpu.cpp), built by tests/test_cpu_pool_stress.py together
// with the library's two sources under -fsanitize=thread and under -fsanitize=address,undefined.  Nothing here is loaded into Python.
//
// Contexts of 1, 2, 5 and 16 workers; interleaved quantize, dequantize and min/max calls at 0, 1, T - 1, 65536 T +- 1 and 2^20 elements; pauses
// longer than the workers' spin phase, so that they sleep on the condition variable and are woken; set_active_threads and set_affinity between
// calls; two caller threads on one context and on a context each; contexts destroyed while their workers spin and while they sleep.  Every
// result is compared with a one-worker scalar run made at the start of the same program.  Every buffer is exactly as long as the call needs
// (the address sanitizer sees the first byte outside it) and element aligned.  Exit status 0 and "ok" on stdout: nothing differed.
#include "piquant_cpu.h"

#include <sched.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <vector>

namespace {

enum { F32 = 0, BF16 = 1, UINT2 = 2, UINT4 = 3, UINT8 = 4 };
constexpr size_t kChunk = 65536;
constexpr float kTau = 0.37f;

struct Case {
    size_t n = 0;
    std::vector<float> x, acc;
    std::vector<uint16_t> xb;
    std::vector<uint8_t> codes8, codes4;
    // the one-worker scalar answers
    std::vector<uint8_t> q8, q4, q2;
    std::vector<float> d32;
    std::vector<uint16_t> d16;
    float lo = 0, hi = 0;
};

uint32_t next(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return s;
}

uint16_t to_bf16(float f) {   // round to nearest even; the data below has no NaN
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

[[noreturn]] void fail(const char* what, size_t n, size_t threads) {
    std::fprintf(stderr, "MISMATCH %s at %zu elements, %zu workers\n", what, n, threads);
    std::exit(1);
}

void quantize_all(piquant_cpu_context_t* ctx, const Case& c, std::vector<uint8_t>& q8, std::vector<uint8_t>& q4, std::vector<uint8_t>& q2) {
    q8.assign(c.n, 0xAA);
    q4.assign((c.n + 1) / 2, 0xAA);
    q2.assign((c.n + 3) / 4, 0xAA);
    piquant_cpu_quantize(ctx, c.x.data(), F32, q8.data(), UINT8, c.n, 2.0f / 255.0f, 127, 0, 0.0f);
    piquant_cpu_quantize(ctx, c.xb.data(), BF16, q4.data(), UINT4, c.n, 2.0f / 15.0f, 7, 1, kTau);
    piquant_cpu_quantize(ctx, c.x.data(), F32, q2.data(), UINT2, c.n, 2.0f / 3.0f, 1, 0, 0.0f);
}

void dequantize_all(piquant_cpu_context_t* ctx, const Case& c, std::vector<float>& d32, std::vector<uint16_t>& d16) {
    d32 = c.acc;
    d16.assign(c.n, 0xAAAA);
    piquant_cpu_dequantize(ctx, c.codes8.data(), UINT8, d32.data(), F32, c.n, 0.02f, 9, 1);      // ADD: reads what it writes
    piquant_cpu_dequantize(ctx, c.codes4.data(), UINT4, d16.data(), BF16, c.n, 0.3f, 2, 0);      // SET: the streaming form past 4 MiB
}

Case make_case(piquant_cpu_context_t* one, size_t n) {
    Case c;
    c.n = n;
    uint32_t s = static_cast<uint32_t>(n) * 2654435761u + 12345u;
    c.x.resize(n);
    c.acc.resize(n);
    c.xb.resize(n);
    c.codes8.resize(n);
    c.codes4.resize((n + 1) / 2);
    for (size_t i = 0; i < n; ++i) {
        c.x[i] = static_cast<float>(next(s) >> 8) * (2.0f / 16777216.0f) - 1.0f;
        c.acc[i] = static_cast<float>(next(s) >> 8) * (6.0f / 16777216.0f) - 3.0f;
        c.xb[i] = to_bf16(c.x[i]);
        c.codes8[i] = static_cast<uint8_t>(next(s) >> 24);
    }
    for (auto& b : c.codes4) b = static_cast<uint8_t>(next(s) >> 24);
    quantize_all(one, c, c.q8, c.q4, c.q2);
    dequantize_all(one, c, c.d32, c.d16);
    piquant_cpu_minmax(one, c.x.data(), F32, n, &c.lo, &c.hi);
    return c;
}

template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// the interleaved calls of one caller on one case
void check(piquant_cpu_context_t* ctx, const Case& c, size_t threads) {
    std::vector<uint8_t> q8, q4, q2;
    std::vector<float> d32;
    std::vector<uint16_t> d16;
    quantize_all(ctx, c, q8, q4, q2);
    float lo, hi;
    piquant_cpu_minmax(ctx, c.x.data(), F32, c.n, &lo, &hi);
    dequantize_all(ctx, c, d32, d16);
    if (!same(q8, c.q8)) fail("fp32 -> uint8", c.n, threads);
    if (!same(q4, c.q4)) fail("bf16 -> uint4 stochastic", c.n, threads);
    if (!same(q2, c.q2)) fail("fp32 -> uint2", c.n, threads);
    if (!same(d32, c.d32)) fail("uint8 -> fp32 ADD", c.n, threads);
    if (!same(d16, c.d16)) fail("uint4 -> bf16 SET", c.n, threads);
    if (lo != c.lo || hi != c.hi) fail("min/max", c.n, threads);
}

void nap() { std::this_thread::sleep_for(std::chrono::milliseconds(60)); }   // the workers spin for well under a millisecond, then sleep

std::vector<size_t> sizes_of(size_t T) { return {0, 1, T - 1, kChunk * T - 1, kChunk * T + 1, size_t {1} << 20}; }

std::vector<int> usable_cpus(size_t at_most) {
    std::vector<int> cpus;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) != 0) return cpus;
    for (int c = 0; c < CPU_SETSIZE && cpus.size() < at_most; ++c)
        if (CPU_ISSET(c, &set)) cpus.push_back(c);
    return cpus;
}

void two_callers(piquant_cpu_context_t* a, piquant_cpu_context_t* b, size_t threads_a, size_t threads_b, const std::map<size_t, Case>& cases) {
    const Case& small = cases.at(1);
    const Case& ragged = cases.at(kChunk * 2 + 1);
    const Case& large = cases.at(size_t {1} << 20);
    std::thread first([&] {
        for (int round = 0; round < 3; ++round) {
            check(a, large, threads_a);
            check(a, small, threads_a);
            if (round == 1) nap();
            check(a, ragged, threads_a);
        }
    });
    std::thread second([&] {
        for (int round = 0; round < 3; ++round) {
            check(b, ragged, threads_b);
            if (round == 0) nap();
            check(b, large, threads_b);
            check(b, small, threads_b);
        }
    });
    first.join();
    second.join();
}

}  // namespace

int main() {
    // the answers: one worker, scalar forms
    piquant_cpu_use_avx512(0);
    piquant_cpu_context_t* one = piquant_cpu_context_create(1);
    const size_t pools[] = {1, 2, 5, 16};
    std::map<size_t, Case> cases;
    for (size_t T : pools)
        for (size_t n : sizes_of(T))
            if (!cases.count(n)) cases.emplace(n, make_case(one, n));
    piquant_cpu_context_destroy(one);
    const int vector = piquant_cpu_use_avx512(1);   // stays 0 on a host without AVX-512: the scalar forms then run under the pool

    for (size_t T : pools) {
        piquant_cpu_context_t* ctx = piquant_cpu_context_create(T);
        if (piquant_cpu_num_threads(ctx) != T) fail("num_threads", 0, T);
        for (size_t n : sizes_of(T)) check(ctx, cases.at(n), T);                 // back to back: the workers spin between the calls
        nap();
        for (size_t n : sizes_of(T)) {                                           // every call wakes sleeping workers
            check(ctx, cases.at(n), T);
            if (n == 1 || n == kChunk * T + 1) nap();
        }
        for (size_t active : {T / 2 + 1, size_t {1}, T, size_t {3}, T}) {        // clamped to 1 .. T by the library
            piquant_cpu_set_active_threads(ctx, active);
            check(ctx, cases.at(kChunk * T + 1), T);
            check(ctx, cases.at(T - 1), T);
        }
        cpu_set_t before, after;
        CPU_ZERO(&before);
        CPU_ZERO(&after);
        sched_getaffinity(0, sizeof before, &before);
        const std::vector<int> cpus = usable_cpus(T);
        piquant_cpu_set_affinity(ctx, cpus.data(), cpus.size());
        check(ctx, cases.at(kChunk * T - 1), T);
        nap();
        check(ctx, cases.at(1), T);
        sched_getaffinity(0, sizeof after, &after);
        if (!CPU_EQUAL(&before, &after)) fail("the caller's affinity mask after a pinned call", 0, T);
        piquant_cpu_set_affinity(ctx, nullptr, 0);
        check(ctx, cases.at(kChunk * T + 1), T);
        two_callers(ctx, ctx, T, T, cases);                                      // two callers, one context
        check(ctx, cases.at(size_t {1} << 20), T);
        piquant_cpu_context_destroy(ctx);                                        // its workers still spin

        ctx = piquant_cpu_context_create(T);
        check(ctx, cases.at(kChunk * T + 1), T);
        nap();
        piquant_cpu_context_destroy(ctx);                                        // its workers sleep
        piquant_cpu_context_destroy(piquant_cpu_context_create(T));              // never called
    }

    piquant_cpu_context_t* a = piquant_cpu_context_create(2);
    piquant_cpu_context_t* b = piquant_cpu_context_create(5);
    two_callers(a, b, 2, 5, cases);                                              // two callers, a context each
    piquant_cpu_context_destroy(a);
    piquant_cpu_context_destroy(b);
    std::printf("ok (%s forms under the pool)\n", vector ? "AVX-512" : "scalar");
    return 0;
}
