// What the host units behind the group-wise and the MX calls of include/piquant_hip.h share (capi_grouped.cpp, capi_mx.cpp; host only, no kernel
// unit includes it): what a message names, the small rules of a buffer, the frame of a call and the loop of a batch.  Every entry reads the same
// way: validate, take the CallLock, resolve, draw the round mode ONCE, end in one run_call.
#pragma once

#include "context.hpp"

#include <type_traits>

namespace pq {

// An entry point and, for a list argument, the index in the list: what every message names.
struct Where {
    const char* entry;
    long index = -1;
};

[[noreturn]] __attribute__((format(printf, 2, 3))) inline void bad(const Where& w, const char* fmt, ...) {
    char what[192];
    std::va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(what, sizeof what, fmt, ap);
    va_end(ap);
    if (w.index < 0) panic("%s: %s", w.entry, what);
    panic("%s: %s (list index %ld)", w.entry, what, w.index);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// A buffer as the kernels take it: pageable host memory has no group-wise or MX path.
inline void* device_ptr(const Where& w, const Resolved& r) {
    if (r.pageable) bad(w, "device (or pinned) buffers are needed");
    return r.dev;
}

// Bytes of one element of a dequantized type (float32, bfloat16).
inline size_t element_size(piquant_dtype_t dtype) { return dtype == PIQUANT_DTYPE_F32 ? 4 : 2; }

// No kernel takes a tensor that is not even aligned to its element; `name` is what the message calls the buffer, or the pair of them.
inline void check_element_aligned(const Where& w, const char* name, const void* p, piquant_dtype_t dtype, const void* q = nullptr,
                                  piquant_dtype_t dtype_q = PIQUANT_DTYPE_F32) {
    if (reinterpret_cast<uintptr_t>(p) % element_size(dtype) != 0 || reinterpret_cast<uintptr_t>(q) % element_size(dtype_q) != 0)
        bad(w, "%s is not aligned to its element size", name);
}

inline int to_op(piquant_reduce_op_t op) { return op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET; }

// The context's lock and device, held from the first resolve to the return.
struct CallLock {
    std::lock_guard<std::mutex> lock;
    DeviceGuard guard;
    explicit CallLock(piquant_context_t* ctx) : lock(ctx->mu), guard(ctx->device) {}
};

// The frame every entry ends in (caller holds the CallLock): the scopes open around the launches only, then the wait of a blocking context, which
// reads what the launchers left (tl_stop_attached), not the scopes.  device_params: something the call reads is written by what was enqueued before
// it, so it is never launched out of order (IndependentCallScope); each call site says what.
template <class Launch>
void run_call(piquant_context_t* ctx, bool device_params, Launch launch) {
    {
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, device_params);
        launch();
    }
    if (ctx->blocking) wait_stream(ctx);
}

// The members of a batch, in order: an empty one is skipped, one that `streams` turns down runs `alone` in its place in the sequence (the guarded
// kernel, same bytes), the others collect in `b`, which is flushed whenever its t[] is full and at the end (the batch launchers return at
// count == 0).  member(i) checks and resolves member i.
template <class Batch, class Member, class Streams, class Alone, class Flush>
void run_batch(Batch& b, const size_t* numels, size_t count, Member member, Streams streams, Alone alone, Flush flush) {
    constexpr int capacity = static_cast<int>(std::extent_v<decltype(Batch::t)>);
    for (size_t i = 0; i < count; ++i) {
        if (numels[i] == 0) continue;
        const auto t = member(i);
        if (!streams(t)) {
            alone(t);
            continue;
        }
        b.t[b.count] = t;
        if (++b.count == capacity) {
            flush();
            b.count = 0;
        }
    }
    flush();
}

}  // namespace pq
