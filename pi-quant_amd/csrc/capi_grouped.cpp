// The group-wise entry points of include/piquant_hip.h: plain, batch, fused reduce, error feedback (EF), reduce + EF, EF with a float32 residual
// for a bfloat16 tensor, quantize-dequantize, the three calls of the randomized Hadamard rotation, the reduce and dequantize-sum in the rotated domain, the two error-feedback calls of the rotated domain, the batches of the rotated quantize, dequantize and error-feedback quantize, and the quantize with a per-group clip search and its batch.  All are stream-ordered, take device (or pinned) buffers only and read the same way: validate, lock and guard, resolve,
// draw the round mode ONCE, open the scopes, launch through the helpers below, wait.  The rules the entries share are stated on the helper that
// owns them.
#include "context.hpp"

using namespace pq;

namespace {

// An entry point and, for a list argument, the index in the list: what every message names.
struct Where {
    const char* entry;
    long index = -1;
};

[[noreturn]] void bad(const Where& w, const char* what) {
    if (w.index < 0) panic("%s: %s", w.entry, what);
    panic("%s: %s (list index %ld)", w.entry, what, w.index);
}

void check_group_size(size_t group_size, const char* entry = nullptr) {
    if (group_size < static_cast<size_t>(kGroupedMinG) || group_size > static_cast<size_t>(kGroupedMaxG) || (group_size & (group_size - 1)) != 0)
        panic("%s%sgroup size %zu is not a power of two in [%d, %d]", entry ? entry : "", entry ? ": " : "", group_size, kGroupedMinG, kGroupedMaxG);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// What needs neither the lock nor the device: no NULL among one tensor's buffers (the residual only where the call has one), scales 4-byte aligned.
void check_tensor(const Where& w, bool ef, const void* in, const void* residual, const void* out, const float* scales, const uint8_t* zero_points) {
    if (!in || !out || (ef && !residual) || !scales || !zero_points) bad(w, "NULL buffer");
    if (reinterpret_cast<uintptr_t>(scales) % 4 != 0) bad(w, "scales must be 4-byte aligned");
}

// The quantize-dequantize calls' form of it: with computed parameters scales and zero_points may BOTH be NULL (no parameters wanted).
void check_requant_tensor(const Where& w, bool params_given, const void* in, const void* out, const float* scales, const uint8_t* zero_points) {
    if (!in || !out) bad(w, "NULL buffer");
    if (!scales != !zero_points) bad(w, "one of scales / zero_points is NULL and the other is not");
    if (!scales && params_given) bad(w, "given parameters need scales and zero_points");
    if (reinterpret_cast<uintptr_t>(scales) % 4 != 0) bad(w, "scales must be 4-byte aligned");
}

// A buffer as the kernels take it: pageable host memory has no group-wise path.
void* device_ptr(const Where& w, const Resolved& r) {
    if (r.pageable) bad(w, "device (or pinned) buffers are needed");
    return r.dev;
}

// One tensor's buffers, resolved (caller holds ctx->mu); a NULL residual or out, or a NULL parameter pair (check_requant_tensor), is left out.  The parameter arrays are always classified: the
// context's assume-device mode speaks for the tensors the caller passes, not for them.
GroupedTensor resolve_tensor(const piquant_context_t* ctx, const Where& w, const void* in, const void* residual, const void* out, const float* scales,
                             const uint8_t* zero_points, size_t numel) {
    GroupedTensor t {};
    t.in = device_ptr(w, ctx->resolve_ptr(in));
    if (residual) t.residual = device_ptr(w, ctx->resolve_ptr(residual));
    if (out) t.out = device_ptr(w, ctx->resolve_ptr(out));
    if (scales) t.scales = static_cast<float*>(device_ptr(w, resolve(scales)));
    if (zero_points) t.zero_points = static_cast<uint8_t*>(device_ptr(w, resolve(zero_points)));
    t.numel = static_cast<int64_t>(numel);
    return t;
}

// The members of a batch, in order: an empty one is skipped, one that `streams` turns down runs `alone` in its place in the sequence (the guarded
// kernel, same bytes), the others collect in `b`, which is flushed every kGroupedBatchMaxTensors members and at the end (the batch launchers return
// at count == 0).  member(i) checks and resolves member i.
template <class Batch, class Member, class Streams, class Alone, class Flush>
void run_batch(Batch& b, const size_t* numels, size_t count, Member member, Streams streams, Alone alone, Flush flush) {
    for (size_t i = 0; i < count; ++i) {
        if (numels[i] == 0) continue;
        const GroupedTensor t = member(i);
        if (!streams(t)) {
            alone(t);
            continue;
        }
        b.t[b.count] = t;
        if (++b.count == kGroupedBatchMaxTensors) {
            flush();
            b.count = 0;
        }
    }
    flush();
}

// The terms of a reduce, each resolved as the grouped dequantize ADD that adds it into acc takes it, and whether all of them are 16-byte aligned.
// The call's one allocation.
struct Terms {
    std::vector<GroupedTensor> term;
    bool aligned = true;
};

Terms resolve_terms(const piquant_context_t* ctx, const char* entry, const void* const* inputs, const float* const* scales,
                    const uint8_t* const* zero_points, size_t count, void* acc_dev, size_t numel) {
    Terms ts;
    ts.term.resize(count);
    for (size_t i = 0; i < count; ++i) {
        const Where w {entry, static_cast<long>(i)};
        check_tensor(w, false, inputs[i], nullptr, acc_dev, scales[i], zero_points[i]);
        ts.term[i] = resolve_tensor(ctx, w, inputs[i], nullptr, nullptr, scales[i], zero_points[i], numel);
        ts.term[i].out = acc_dev;   // resolved by the caller
        ts.aligned = ts.aligned && aligned16(ts.term[i].in);
    }
    return ts;
}

// acc += dequantize_grouped(term i) for i in [from, to), in order: one grouped dequantize ADD launch each
void add_terms(piquant_context_t* ctx, const Terms& ts, size_t from, size_t to, const GroupedDequantCall& add) {
    for (size_t i = from; i < to; ++i) launch_dequantize_grouped(GroupedDequantLaunch {ts.term[i], add}, ctx->stream, ctx->num_cu);
}

// Index of the first term the fused reduce kernel takes; the terms in front of it go into acc by grouped dequantize ADD first.  Every buffer of
// the call aligned as its kernel loads it (16 bytes; 8 for a bfloat16 acc with a float32 residual): the surplus over kGroupedReduceMaxInputs goes
// first and the last terms are fused.  Anything misaligned: count, i.e. every term is added first and acc is quantized alone -- the two-step form,
// the same bytes.  (No terms: nothing to fuse either way.)
size_t fused_from(size_t count, bool all_aligned) {
    if (!all_aligned) return count;
    return count > static_cast<size_t>(kGroupedReduceMaxInputs) ? count - kGroupedReduceMaxInputs : 0;
}

// The residual of an error-feedback call: of the tensor's type, or float32 for a bfloat16 tensor (the kernels of kernels_grouped_ef_f32r.hip).
enum class Residual { Same, F32 };

Residual residual_kind(const char* entry, piquant_dtype_t dtype_in, piquant_dtype_t dtype_residual) {
    if (dtype_residual == dtype_in) return Residual::Same;
    if (dtype_in == PIQUANT_DTYPE_BF16 && dtype_residual == PIQUANT_DTYPE_F32) return Residual::F32;
    panic("%s: a %s residual for a %s tensor (the tensor's type, or float32 for a bfloat16 tensor, is needed)", entry, dtype_of(dtype_residual).name,
          dtype_of(dtype_in).name);
}

// The streaming EF kernels' rule: tensor, residual and output 16-byte aligned; with a float32 residual the bfloat16 tensor needs 8 bytes only
// (its lane-row is four elements).
bool ef_streams(Residual k, const GroupedTensor& t) {
    const bool in_ok = k == Residual::F32 ? (reinterpret_cast<uintptr_t>(t.in) & 7u) == 0 : aligned16(t.in);
    return in_ok && aligned16(t.residual) && aligned16(t.out);
}

// Types that differ leave room for a tensor or a residual that is not even aligned to its element: no kernel takes that.
void check_ef_elements(Residual k, const Where& w, const GroupedTensor& t) {
    if (k == Residual::F32 && (reinterpret_cast<uintptr_t>(t.in) % 2 != 0 || reinterpret_cast<uintptr_t>(t.residual) % 4 != 0))
        bad(w, "the tensor or its residual is not aligned to its element size");
}

void launch_ef_batch(Residual k, const GroupedEfBatchLaunch& b, hipStream_t stream) {
    if (k == Residual::F32) launch_quantize_grouped_ef_f32r_batch(b, stream);
    else launch_quantize_grouped_ef_batch(b, stream);
}

void launch_ef_guarded(Residual k, const GroupedEfLaunch& q, hipStream_t stream, int num_cu) {
    if (k == Residual::F32) launch_quantize_grouped_ef_f32r_guarded(q, stream, num_cu);
    else launch_quantize_grouped_ef_guarded(q, stream, num_cu);
}

// EF-quantize one (in, residual) pair: streaming (a batch of one, which launches the single-tensor kernel) if its alignment rule holds, else guarded
void ef_quantize_one(piquant_context_t* ctx, Residual k, const GroupedEfLaunch& q) {
    if (ef_streams(k, q)) launch_ef_batch(k, GroupedEfBatchLaunch {q, {q}, 1}, ctx->stream);
    else launch_ef_guarded(k, q, ctx->stream, ctx->num_cu);
}

// piquant_hip_quantize_grouped_ef_batch and the float32-residual path of piquant_hip_quantize_grouped_ef_mixed_batch, behind their type checks.
// ONE threshold (or per-element seed and base) for the whole batch, drawn whenever count > 0 -- also when every member is empty.
void quantize_grouped_ef_batch(piquant_context_t* ctx, const char* entry, Residual k, const void* const* inputs, piquant_dtype_t dtype_in,
                               void* const* residuals, void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels, size_t group_size,
                               float* const* scales, uint8_t* const* zero_points, size_t count, piquant_round_mode_t mode) {
    check_group_size(group_size);
    if (count == 0) return;   // before a stochastic threshold would be drawn
    if (!inputs || !residuals || !outputs || !numels || !scales || !zero_points) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    GroupedEfBatchLaunch b {{static_cast<int64_t>(group_size), dtype_in, dtype_out, false, round_mode_fields(ctx, mode)}, {}, 0};
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the residual is written by the previous step's call: always behind it
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, static_cast<long>(i)};
            check_tensor(w, true, inputs[i], residuals[i], outputs[i], scales[i], zero_points[i]);
            const GroupedTensor t = resolve_tensor(ctx, w, inputs[i], residuals[i], outputs[i], scales[i], zero_points[i], numels[i]);
            check_ef_elements(k, w, t);
            return t;
        },
        [&](const GroupedTensor& t) { return ef_streams(k, t); },
        [&](const GroupedTensor& t) { launch_ef_guarded(k, GroupedEfLaunch {t, b}, ctx->stream, ctx->num_cu); },
        [&] { launch_ef_batch(k, b, ctx->stream); });
    if (ctx->blocking) wait_stream(ctx);
}

// The three reduce entries behind their type checks: out = quantize_grouped(acc + terms [+ residual]), with error feedback when `ef`.
// The call's one threshold is drawn once, after every buffer is resolved, whichever form then runs; numel == 0 returns before it.  A float32
// residual for a bfloat16 accumulator fuses like the others (kernels_grouped_reduce_ef_f32r.hip), with ef_streams' rule for the accumulator:
// 8-byte aligned, the width of its loads.
void reduce_quantize_grouped(piquant_context_t* ctx, const char* entry, bool ef, Residual k, void* acc, piquant_dtype_t dtype_acc, void* residual,
                             const void* const* inputs, const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count,
                             void* out, piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                             piquant_round_mode_t mode) {
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    const Where w {entry};
    check_tensor(w, ef, acc, residual, out, scales, zero_points);
    if (count != 0 && (!inputs || !input_scales || !input_zero_points)) bad(w, "NULL term list");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, acc, ef ? residual : nullptr, out, scales, zero_points, numel);
    if (ef) check_ef_elements(k, w, t);
    const Terms terms = resolve_terms(ctx, entry, inputs, input_scales, input_zero_points, count, const_cast<void*>(t.in) /* acc */, numel);
    const bool aligned = terms.aligned && (ef ? ef_streams(k, t) : aligned16(t.in) && aligned16(t.out));
    const GroupedQuantCall call {static_cast<int64_t>(group_size), dtype_acc, dtype_out, false, round_mode_fields(ctx, mode)};
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // terms, parameters and residual are written by what was enqueued before: always behind it
    const size_t first = fused_from(count, aligned);
    add_terms(ctx, terms, 0, first, GroupedDequantCall {call.group_size, dtype_out, dtype_acc, OP_ADD});
    if (first < count) {
        GroupedReduceLaunch r {t, call, {}, static_cast<int>(count - first)};
        std::copy(terms.term.begin() + static_cast<std::ptrdiff_t>(first), terms.term.end(), r.term);
        if (!ef) launch_reduce_quantize_grouped(r, ctx->stream);
        else if (k == Residual::F32) launch_reduce_quantize_grouped_ef_f32r(r, ctx->stream);
        else launch_reduce_quantize_grouped_ef(r, ctx->stream);
    } else if (ef) {   // no terms, or the two-step form: quantize_grouped_ef(acc, residual)
        ef_quantize_one(ctx, k, GroupedEfLaunch {t, call});
    } else {           // quantize_grouped(acc)
        launch_quantize_grouped(GroupedQuantLaunch {t, call}, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

// Both quantize-dequantize entries behind their NULL-context check; `single`: the one tensor of piquant_hip_quantize_dequantize_grouped, whose messages
// carry no list index.  ONE threshold (or per-element seed and base) for the whole batch, drawn whenever count > 0 -- also when every member is empty.
void quantize_dequantize_grouped_batch(piquant_context_t* ctx, const char* entry, bool single, const void* const* inputs, piquant_dtype_t dtype_in_out,
                                       void* const* outputs, piquant_dtype_t quant_dtype, const size_t* numels, size_t group_size, float* const* scales,
                                       uint8_t* const* zero_points, size_t count, int params_given, piquant_round_mode_t mode, piquant_reduce_op_t op) {
    if (dtype_of(dtype_in_out).quant) panic("%s: dtype_in_out (%s) must be a dequantized type", entry, dtype_of(dtype_in_out).name);
    if (!dtype_of(quant_dtype).quant) panic("%s: quant_dtype (%s) must be a quantized type", entry, dtype_of(quant_dtype).name);
    if (mode != PIQUANT_NEAREST && mode != PIQUANT_STOCHASTIC) panic("%s: invalid round mode %d", entry, static_cast<int>(mode));
    if (op != PIQUANT_REDUCE_OP_SET && op != PIQUANT_REDUCE_OP_ADD) panic("%s: invalid reduce op %d", entry, static_cast<int>(op));
    check_group_size(group_size, entry);
    if (count == 0) return;   // before a stochastic threshold would be drawn
    const bool no_params = !scales && !zero_points;   // NULL lists: no parameters wanted
    if (!inputs || !outputs || !numels || (!scales != !zero_points) || (no_params && params_given != 0)) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const bool add = op == PIQUANT_REDUCE_OP_ADD;
    GroupedRequantBatchLaunch b {{{static_cast<int64_t>(group_size), dtype_in_out, quant_dtype, params_given != 0, round_mode_fields(ctx, mode)},
                                  add ? OP_ADD : OP_SET}, {}, 0};
    const size_t esize = dtype_in_out == PIQUANT_DTYPE_F32 ? 4 : 2;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, add || b.params_given);   // the accumulator and given parameters are written by what was enqueued before
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, single ? -1 : static_cast<long>(i)};
            float* sc = no_params ? nullptr : scales[i];
            uint8_t* zp = no_params ? nullptr : zero_points[i];
            check_requant_tensor(w, b.params_given, inputs[i], outputs[i], sc, zp);
            const GroupedTensor t = resolve_tensor(ctx, w, inputs[i], nullptr, outputs[i], sc, zp, numels[i]);
            if (reinterpret_cast<uintptr_t>(t.in) % esize != 0 || reinterpret_cast<uintptr_t>(t.out) % esize != 0)
                bad(w, "in or out is not aligned to its element size");
            return t;
        },
        [](const GroupedTensor& t) { return aligned16(t.in) && aligned16(t.out); },
        [&](const GroupedTensor& t) { launch_quantize_dequantize_grouped_guarded(GroupedRequantLaunch {t, b}, ctx->stream, ctx->num_cu); },
        [&] { launch_quantize_dequantize_grouped_batch(b, ctx->stream); });
    if (ctx->blocking) wait_stream(ctx);
}

}  // namespace

extern "C" {

void piquant_hip_quantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel,
                                  size_t group_size, float* scales, uint8_t* zero_points, int params_given, piquant_round_mode_t mode) {
    const Where w {"piquant_hip_quantize_grouped"};
    if (!ctx) bad(w, "context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    check_tensor(w, false, in, nullptr, out, scales, zero_points);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, in, nullptr, out, scales, zero_points, numel);
    // the call's one threshold (or the per-element seed and base), as quantize_uniform draws it
    const GroupedQuantLaunch q {t, {static_cast<int64_t>(group_size), dtype_in, dtype_out, params_given != 0, round_mode_fields(ctx, mode)}};
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, q.params_given);   // given parameters are written by whatever was enqueued just before
        launch_quantize_grouped(q, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_dequantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel,
                                    size_t group_size, const float* scales, const uint8_t* zero_points, piquant_reduce_op_t op) {
    const Where w {"piquant_hip_dequantize_grouped"};
    if (!ctx) bad(w, "context is NULL");
    check_dequant_types(dtype_in, dtype_out, op);
    check_group_size(group_size);
    if (numel == 0) return;
    check_tensor(w, false, in, nullptr, out, scales, zero_points);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, in, nullptr, out, scales, zero_points, numel);
    const GroupedDequantLaunch d {t, {static_cast<int64_t>(group_size), dtype_in, dtype_out, op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET}};
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, true);   // the parameters are written by whatever was enqueued just before
        launch_dequantize_grouped(d, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

// The three rotated calls (grouped_rot_kernels.hpp): the two entries above with the rotation's seed, and the stand-alone transform.  In and out
// 16-byte aligned: the streaming kernels; anything else element-aligned: the guarded ones, the same bytes.
void piquant_hip_hadamard_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype, void* out, size_t numel, size_t group_size,
                                  uint64_t seed, int inverse) {
    const Where w {"piquant_hip_hadamard_grouped"};
    if (!ctx) bad(w, "context is NULL");
    if (dtype_of(dtype).quant) panic("%s: dtype (%s) must be a dequantized type", w.entry, dtype_of(dtype).name);
    check_group_size(group_size, w.entry);
    if (numel == 0) return;
    if (!in || !out) bad(w, "NULL buffer");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, in, nullptr, out, nullptr, nullptr, numel);
    const size_t esize = dtype == PIQUANT_DTYPE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(t.in) % esize != 0 || reinterpret_cast<uintptr_t>(t.out) % esize != 0) bad(w, "in or out is not aligned to its element size");
    const GroupedHadamardLaunch h {t.in, t.out, t.numel, static_cast<int64_t>(group_size), dtype, seed, inverse != 0};
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, false);
        launch_hadamard_grouped(h, !(aligned16(t.in) && aligned16(t.out)), ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_grouped_rotated(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out,
                                          size_t numel, size_t group_size, float* scales, uint8_t* zero_points, uint64_t seed, piquant_round_mode_t mode) {
    const Where w {"piquant_hip_quantize_grouped_rotated"};
    if (!ctx) bad(w, "context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    check_tensor(w, false, in, nullptr, out, scales, zero_points);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, in, nullptr, out, scales, zero_points, numel);
    if (reinterpret_cast<uintptr_t>(t.in) % (dtype_in == PIQUANT_DTYPE_F32 ? 4 : 2) != 0) bad(w, "in is not aligned to its element size");
    // the call's one threshold (or the per-element seed and base), as piquant_hip_quantize_grouped draws it
    const GroupedQuantLaunch q {t, {static_cast<int64_t>(group_size), dtype_in, dtype_out, false, round_mode_fields(ctx, mode)}};
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, false);
        launch_quantize_grouped_rotated(q, seed, !(aligned16(t.in) && aligned16(t.out)), ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_dequantize_grouped_rotated(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out,
                                            size_t numel, size_t group_size, const float* scales, const uint8_t* zero_points, uint64_t seed,
                                            piquant_reduce_op_t op) {
    const Where w {"piquant_hip_dequantize_grouped_rotated"};
    if (!ctx) bad(w, "context is NULL");
    check_dequant_types(dtype_in, dtype_out, op);
    check_group_size(group_size);
    if (numel == 0) return;
    check_tensor(w, false, in, nullptr, out, scales, zero_points);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, in, nullptr, out, scales, zero_points, numel);
    if (reinterpret_cast<uintptr_t>(t.out) % (dtype_out == PIQUANT_DTYPE_F32 ? 4 : 2) != 0) bad(w, "out is not aligned to its element size");
    const GroupedDequantLaunch d {t, {static_cast<int64_t>(group_size), dtype_in, dtype_out, op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET}};
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, true);   // the parameters are written by whatever was enqueued just before
        launch_dequantize_grouped_rotated(d, seed, !(aligned16(t.in) && aligned16(t.out)), ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

// The two steps of a grouped collective in the rotated domain: ONE launch each, streaming when acc / out and every term's packed bytes are 16-byte
// aligned, guarded otherwise.  More than kGroupedReduceMaxInputs terms abort: the float32 running sum has nowhere to be spilled to.
void piquant_hip_reduce_quantize_grouped_rotated(piquant_context_t* ctx, const void* acc, piquant_dtype_t dtype_acc, const void* const* inputs,
                                                 const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count, void* out,
                                                 piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                                 uint64_t seed, piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_reduce_quantize_grouped_rotated";
    const Where w {entry};
    if (!ctx) bad(w, "context is NULL");
    check_dynamic_types(dtype_acc, dtype_out, mode);
    check_group_size(group_size, entry);
    if (count > static_cast<size_t>(kGroupedReduceMaxInputs)) panic("%s: %zu terms, at most %d", entry, count, kGroupedReduceMaxInputs);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    check_tensor(w, false, acc, nullptr, out, scales, zero_points);
    if (count != 0 && (!inputs || !input_scales || !input_zero_points)) bad(w, "NULL term list");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, acc, nullptr, out, scales, zero_points, numel);
    if (reinterpret_cast<uintptr_t>(t.in) % (dtype_acc == PIQUANT_DTYPE_F32 ? 4 : 2) != 0) bad(w, "acc is not aligned to its element size");
    const Terms terms = resolve_terms(ctx, entry, inputs, input_scales, input_zero_points, count, t.out, numel);
    // the call's one threshold (or the per-element seed and base), as piquant_hip_quantize_grouped draws it
    GroupedReduceLaunch r {t, {static_cast<int64_t>(group_size), dtype_acc, dtype_out, false, round_mode_fields(ctx, mode)}, {}, static_cast<int>(count)};
    std::copy(terms.term.begin(), terms.term.end(), r.term);
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, true);   // terms and parameters are written by what was enqueued before: always behind it
        launch_reduce_quantize_grouped_rotated(r, seed, !(terms.aligned && aligned16(t.in) && aligned16(t.out)), ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

// Error feedback in the rotated domain: the two quantizing calls above with a float32 residual of rotated values (grouped_rot_ef_kernels.hpp).
// ONE launch each: streaming when the tensor is aligned as its rows are loaded (16 bytes; 8 for bfloat16) and residual, out and every term's packed
// bytes are 16-byte aligned, guarded otherwise.  Without terms the reduce IS the quantize: one body serves both entries.
void piquant_hip_reduce_quantize_grouped_rotated_ef(piquant_context_t* ctx, const void* acc, piquant_dtype_t dtype_acc, float* residual,
                                                    const void* const* inputs, const float* const* input_scales,
                                                    const uint8_t* const* input_zero_points, size_t count, void* out, piquant_dtype_t dtype_out,
                                                    size_t numel, size_t group_size, float* scales, uint8_t* zero_points, uint64_t seed,
                                                    piquant_round_mode_t mode) {
    const char* entry = count == 0 ? "piquant_hip_quantize_grouped_rotated_ef" : "piquant_hip_reduce_quantize_grouped_rotated_ef";
    const Where w {entry};
    if (!ctx) bad(w, "context is NULL");
    check_dynamic_types(dtype_acc, dtype_out, mode);
    check_group_size(group_size, entry);
    if (count > static_cast<size_t>(kGroupedReduceMaxInputs)) panic("%s: %zu terms, at most %d", entry, count, kGroupedReduceMaxInputs);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    check_tensor(w, true, acc, residual, out, scales, zero_points);
    if (count != 0 && (!inputs || !input_scales || !input_zero_points)) bad(w, "NULL term list");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const GroupedTensor t = resolve_tensor(ctx, w, acc, residual, out, scales, zero_points, numel);
    const bool f32 = dtype_acc == PIQUANT_DTYPE_F32;
    if (reinterpret_cast<uintptr_t>(t.in) % (f32 ? 4 : 2) != 0 || reinterpret_cast<uintptr_t>(t.residual) % 4 != 0)
        bad(w, "the tensor or its residual is not aligned to its element size");
    const Terms terms = resolve_terms(ctx, entry, inputs, input_scales, input_zero_points, count, t.out, numel);
    const bool streams = terms.aligned && (reinterpret_cast<uintptr_t>(t.in) & (f32 ? 15u : 7u)) == 0 && aligned16(t.residual) && aligned16(t.out);
    // the call's one threshold (or the per-element seed and base), as piquant_hip_quantize_grouped draws it
    GroupedReduceLaunch r {t, {static_cast<int64_t>(group_size), dtype_acc, dtype_out, false, round_mode_fields(ctx, mode)}, {}, static_cast<int>(count)};
    std::copy(terms.term.begin(), terms.term.end(), r.term);
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, true);   // the residual is written by the previous step's call: always behind it
        if (count == 0) launch_quantize_grouped_rotated_ef(GroupedEfLaunch {t, r}, seed, !streams, ctx->stream, ctx->num_cu);
        else launch_reduce_quantize_grouped_rotated_ef(r, seed, !streams, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_grouped_rotated_ef(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, float* residual, void* out,
                                             piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                             uint64_t seed, piquant_round_mode_t mode) {
    piquant_hip_reduce_quantize_grouped_rotated_ef(ctx, in, dtype_in, residual, nullptr, nullptr, nullptr, 0, out, dtype_out, numel, group_size, scales,
                                                   zero_points, seed, mode);
}

void piquant_hip_dequantize_sum_grouped_rotated(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count, void* out,
                                                piquant_dtype_t dtype_out, size_t numel, size_t group_size, uint64_t seed, piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_dequantize_sum_grouped_rotated";
    const Where w {entry};
    if (!ctx) bad(w, "context is NULL");
    check_dequant_types(dtype_in, dtype_out, op);
    check_group_size(group_size, entry);
    if (count == 0) bad(w, "no terms (count must be at least 1)");
    if (count > static_cast<size_t>(kGroupedReduceMaxInputs)) panic("%s: %zu terms, at most %d", entry, count, kGroupedReduceMaxInputs);
    if (!inputs || !input_scales || !input_zero_points) bad(w, "NULL term list");
    if (numel == 0) return;   // a no-op whatever the buffers are: an empty tensor's address may be NULL
    if (!out) bad(w, "NULL buffer");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    void* out_dev = device_ptr(w, ctx->resolve_ptr(out));
    if (reinterpret_cast<uintptr_t>(out_dev) % (dtype_out == PIQUANT_DTYPE_F32 ? 4 : 2) != 0) bad(w, "out is not aligned to its element size");
    const Terms terms = resolve_terms(ctx, entry, inputs, input_scales, input_zero_points, count, out_dev, numel);
    GroupedDequantSumLaunch d {{static_cast<int64_t>(group_size), dtype_in, dtype_out, op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET}, out_dev,
                               static_cast<int64_t>(numel), {}, static_cast<int>(count)};
    std::copy(terms.term.begin(), terms.term.end(), d.term);
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, true);   // terms, parameters and an ADD's out are written by what was enqueued before: always behind it
        launch_dequantize_sum_grouped_rotated(d, seed, !(terms.aligned && aligned16(out_dev)), ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                        piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, float* const* scales,
                                        uint8_t* const* zero_points, size_t count, int params_given, piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_quantize_grouped_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (count == 0) return;   // before a stochastic threshold would be drawn
    if (!inputs || !outputs || !numels || !scales || !zero_points) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    // ONE threshold (or per-element seed and base) for the whole batch, also when every member is empty
    GroupedQuantBatchLaunch b {{static_cast<int64_t>(group_size), dtype_in, dtype_out, params_given != 0, round_mode_fields(ctx, mode)}, {}, 0};
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, b.params_given);
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, static_cast<long>(i)};
            check_tensor(w, false, inputs[i], nullptr, outputs[i], scales[i], zero_points[i]);
            return resolve_tensor(ctx, w, inputs[i], nullptr, outputs[i], scales[i], zero_points[i], numels[i]);
        },
        [](const GroupedTensor& t) { return aligned16(t.in) && aligned16(t.out); },
        [&](const GroupedTensor& t) { launch_quantize_grouped(GroupedQuantLaunch {t, b}, ctx->stream, ctx->num_cu); },
        [&] { launch_quantize_grouped_batch(b, ctx->stream); });
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_dequantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                          piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, const float* const* scales,
                                          const uint8_t* const* zero_points, size_t count, piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_dequantize_grouped_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dequant_types(dtype_in, dtype_out, op);
    check_group_size(group_size);
    if (count == 0) return;
    if (!inputs || !outputs || !numels || !scales || !zero_points) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    GroupedDequantBatchLaunch b {{static_cast<int64_t>(group_size), dtype_in, dtype_out, op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET}, {}, 0};
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the parameters are written by whatever was enqueued just before
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, static_cast<long>(i)};
            check_tensor(w, false, inputs[i], nullptr, outputs[i], scales[i], zero_points[i]);
            return resolve_tensor(ctx, w, inputs[i], nullptr, outputs[i], scales[i], zero_points[i], numels[i]);
        },
        [](const GroupedTensor& t) { return aligned16(t.in) && aligned16(t.out); },
        [&](const GroupedTensor& t) { launch_dequantize_grouped(GroupedDequantLaunch {t, b}, ctx->stream, ctx->num_cu); },
        [&] { launch_dequantize_grouped_batch(b, ctx->stream); });
    if (ctx->blocking) wait_stream(ctx);
}

// The batches of the three rotated calls: the rules of the two batches above and of quantize_grouped_ef_batch (ONE threshold, or per-element seed and
// base, per batch, drawn whenever count > 0; empty members skipped; one streaming launch per kGroupedBatchMaxTensors members), with the rotation's
// seed.  A member that fails its single call's alignment rule runs alone, in its place in the sequence, through that call's guarded launch.
void piquant_hip_quantize_grouped_rotated_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                                piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, float* const* scales,
                                                uint8_t* const* zero_points, size_t count, uint64_t seed, piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_quantize_grouped_rotated_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (count == 0) return;   // before a stochastic threshold would be drawn
    if (!inputs || !outputs || !numels || !scales || !zero_points) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    // ONE threshold (or per-element seed and base) for the whole batch, also when every member is empty
    GroupedQuantBatchLaunch b {{static_cast<int64_t>(group_size), dtype_in, dtype_out, false, round_mode_fields(ctx, mode)}, {}, 0};
    const size_t esize = dtype_in == PIQUANT_DTYPE_F32 ? 4 : 2;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, false);
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, static_cast<long>(i)};
            check_tensor(w, false, inputs[i], nullptr, outputs[i], scales[i], zero_points[i]);
            const GroupedTensor t = resolve_tensor(ctx, w, inputs[i], nullptr, outputs[i], scales[i], zero_points[i], numels[i]);
            if (reinterpret_cast<uintptr_t>(t.in) % esize != 0) bad(w, "in is not aligned to its element size");
            return t;
        },
        [](const GroupedTensor& t) { return aligned16(t.in) && aligned16(t.out); },
        [&](const GroupedTensor& t) { launch_quantize_grouped_rotated(GroupedQuantLaunch {t, b}, seed, true, ctx->stream, ctx->num_cu); },
        [&] { launch_quantize_grouped_rotated_batch(b, seed, ctx->stream); });
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_dequantize_grouped_rotated_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                                  piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, const float* const* scales,
                                                  const uint8_t* const* zero_points, size_t count, uint64_t seed, piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_dequantize_grouped_rotated_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dequant_types(dtype_in, dtype_out, op);
    check_group_size(group_size);
    if (count == 0) return;
    if (!inputs || !outputs || !numels || !scales || !zero_points) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    GroupedDequantBatchLaunch b {{static_cast<int64_t>(group_size), dtype_in, dtype_out, op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET}, {}, 0};
    const size_t esize = dtype_out == PIQUANT_DTYPE_F32 ? 4 : 2;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the parameters are written by whatever was enqueued just before
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, static_cast<long>(i)};
            check_tensor(w, false, inputs[i], nullptr, outputs[i], scales[i], zero_points[i]);
            const GroupedTensor t = resolve_tensor(ctx, w, inputs[i], nullptr, outputs[i], scales[i], zero_points[i], numels[i]);
            if (reinterpret_cast<uintptr_t>(t.out) % esize != 0) bad(w, "out is not aligned to its element size");
            return t;
        },
        [](const GroupedTensor& t) { return aligned16(t.in) && aligned16(t.out); },
        [&](const GroupedTensor& t) { launch_dequantize_grouped_rotated(GroupedDequantLaunch {t, b}, seed, true, ctx->stream, ctx->num_cu); },
        [&] { launch_dequantize_grouped_rotated_batch(b, seed, ctx->stream); });
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_grouped_rotated_ef_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, float* const* residuals,
                                                   void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels, size_t group_size,
                                                   float* const* scales, uint8_t* const* zero_points, size_t count, uint64_t seed,
                                                   piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_quantize_grouped_rotated_ef_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size, entry);
    if (count == 0) return;   // before a stochastic threshold would be drawn
    if (!inputs || !residuals || !outputs || !numels || !scales || !zero_points) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    // ONE threshold (or per-element seed and base) for the whole batch, also when every member is empty
    GroupedEfBatchLaunch b {{static_cast<int64_t>(group_size), dtype_in, dtype_out, false, round_mode_fields(ctx, mode)}, {}, 0};
    const bool f32 = dtype_in == PIQUANT_DTYPE_F32;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the residual is written by the previous step's call: always behind it
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, static_cast<long>(i)};
            check_tensor(w, true, inputs[i], residuals[i], outputs[i], scales[i], zero_points[i]);
            const GroupedTensor t = resolve_tensor(ctx, w, inputs[i], residuals[i], outputs[i], scales[i], zero_points[i], numels[i]);
            if (reinterpret_cast<uintptr_t>(t.in) % (f32 ? 4 : 2) != 0 || reinterpret_cast<uintptr_t>(t.residual) % 4 != 0)
                bad(w, "the tensor or its residual is not aligned to its element size");
            return t;
        },
        [&](const GroupedTensor& t) { return (reinterpret_cast<uintptr_t>(t.in) & (f32 ? 15u : 7u)) == 0 && aligned16(t.residual) && aligned16(t.out); },
        [&](const GroupedTensor& t) { launch_quantize_grouped_rotated_ef(GroupedEfLaunch {t, b}, seed, true, ctx->stream, ctx->num_cu); },
        [&] { launch_quantize_grouped_rotated_ef_batch(b, seed, ctx->stream); });
    if (ctx->blocking) wait_stream(ctx);
}

// The clip search (grouped_clip_kernels.hpp): piquant_hip_quantize_grouped_batch's rules with computed parameters, the candidates' count and the
// members' choices.  A member whose in or out is not 16-byte aligned runs alone through the guarded launch: the same bytes.  steps == 1 searches
// nothing: it IS quantize_grouped with computed parameters, so its launches are made and the members' choices are zeroed on the stream.
void piquant_hip_quantize_grouped_clipped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                                piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, float* const* scales,
                                                uint8_t* const* zero_points, uint8_t* const* choices, size_t count, int steps,
                                                piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_quantize_grouped_clipped_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size, entry);
    if (steps < 1 || steps > 12) panic("%s: steps %d is not in [1, 12]", entry, steps);
    if (count == 0) return;   // before a stochastic threshold would be drawn
    if (!inputs || !outputs || !numels || !scales || !zero_points) panic("%s: NULL argument", entry);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    // ONE threshold (or per-element seed and base) for the whole batch, also when every member is empty
    GroupedQuantBatchLaunch b {{static_cast<int64_t>(group_size), dtype_in, dtype_out, false, round_mode_fields(ctx, mode)}, {}, 0};
    const size_t esize = dtype_in == PIQUANT_DTYPE_F32 ? 4 : 2;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, false);
    run_batch(
        b, numels, count,
        [&](size_t i) {
            const Where w {entry, static_cast<long>(i)};
            check_tensor(w, false, inputs[i], nullptr, outputs[i], scales[i], zero_points[i]);
            GroupedTensor t = resolve_tensor(ctx, w, inputs[i], nullptr, outputs[i], scales[i], zero_points[i], numels[i]);
            if (reinterpret_cast<uintptr_t>(t.in) % esize != 0) bad(w, "in is not aligned to its element size");
            if (choices && choices[i]) t.choices = static_cast<uint8_t*>(device_ptr(w, resolve(choices[i])));
            if (steps == 1 && t.choices) PQ_HIP(hipMemsetAsync(t.choices, 0, (numels[i] + group_size - 1) / group_size, ctx->stream));
            return t;
        },
        [](const GroupedTensor& t) { return aligned16(t.in) && aligned16(t.out); },
        [&](const GroupedTensor& t) {
            if (steps == 1) launch_quantize_grouped(GroupedQuantLaunch {t, b}, ctx->stream, ctx->num_cu);
            else launch_quantize_grouped_clipped_guarded(GroupedQuantLaunch {t, b}, steps, ctx->stream, ctx->num_cu);
        },
        [&] {
            if (steps == 1 && b.count == 1) launch_quantize_grouped(GroupedQuantLaunch {b.t[0], b}, ctx->stream, ctx->num_cu);   // the single kernel
            else if (steps == 1) launch_quantize_grouped_batch(b, ctx->stream);
            else launch_quantize_grouped_clipped_batch(b, steps, ctx->stream);
        });
    if (ctx->blocking) wait_stream(ctx);
}

// The single call is a batch of one, which launches the single-tensor kernel; an empty tensor returns behind the argument checks and draws nothing.
void piquant_hip_quantize_grouped_clipped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out,
                                          size_t numel, size_t group_size, float* scales, uint8_t* zero_points, uint8_t* choices, int steps,
                                          piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped_clipped: context is NULL");
    piquant_hip_quantize_grouped_clipped_batch(ctx, &in, dtype_in, &out, dtype_out, &numel, group_size, &scales, &zero_points, &choices, numel == 0 ? 0 : 1,
                                               steps, mode);
}

void piquant_hip_reduce_quantize_grouped(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, const void* const* inputs,
                                         const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count, void* out,
                                         piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                         piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_reduce_quantize_grouped";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_acc, dtype_out, mode);
    reduce_quantize_grouped(ctx, entry, false, Residual::Same, acc, dtype_acc, nullptr, inputs, input_scales, input_zero_points, count, out, dtype_out, numel,
                            group_size, scales, zero_points, mode);
}

// out (op)= the terms, in order.  Everything 16-byte aligned: one launch per kGroupedReduceMaxInputs terms, the first with the call's op and the
// others ADD -- the composition rounds to dtype_out at every term, so where the launches are cut changes no byte.  Anything misaligned: the
// composition itself, one guarded grouped dequantize per term.
void piquant_hip_dequantize_sum_grouped(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, const float* const* input_scales,
                                        const uint8_t* const* input_zero_points, size_t count, void* out, piquant_dtype_t dtype_out, size_t numel,
                                        size_t group_size, piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_dequantize_sum_grouped";
    const Where w {entry};
    if (!ctx) bad(w, "context is NULL");
    check_dequant_types(dtype_in, dtype_out, op);
    check_group_size(group_size, entry);
    if (count == 0) bad(w, "no terms (count must be at least 1)");
    if (!inputs || !input_scales || !input_zero_points) bad(w, "NULL term list");
    if (!out) bad(w, "NULL buffer");
    if (numel == 0) return;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    void* out_dev = device_ptr(w, ctx->resolve_ptr(out));
    if (reinterpret_cast<uintptr_t>(out_dev) % (dtype_out == PIQUANT_DTYPE_F32 ? 4 : 2) != 0) bad(w, "out is not aligned to its element size");
    const Terms terms = resolve_terms(ctx, entry, inputs, input_scales, input_zero_points, count, out_dev, numel);
    const int first_op = op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET;
    const GroupedDequantCall call {static_cast<int64_t>(group_size), dtype_in, dtype_out, first_op};
    {   // both scopes end before the wait
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, true);   // terms, parameters and an ADD's out are written by what was enqueued before: always behind it
        if (terms.aligned && aligned16(out_dev)) {
            for (size_t from = 0; from < count; from += kGroupedReduceMaxInputs) {
                const size_t n = std::min(count - from, static_cast<size_t>(kGroupedReduceMaxInputs));
                GroupedDequantSumLaunch d {call, out_dev, static_cast<int64_t>(numel), {}, static_cast<int>(n)};
                if (from != 0) d.op = OP_ADD;
                std::copy_n(terms.term.begin() + static_cast<std::ptrdiff_t>(from), n, d.term);
                launch_dequantize_sum_grouped(d, ctx->stream);
            }
        } else {
            add_terms(ctx, terms, 0, 1, call);
            add_terms(ctx, terms, 1, count, GroupedDequantCall {call.group_size, dtype_in, dtype_out, OP_ADD});
        }
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_grouped_ef_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* residuals,
                                           void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, float* const* scales,
                                           uint8_t* const* zero_points, size_t count, piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_quantize_grouped_ef_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_in, dtype_out, mode);
    quantize_grouped_ef_batch(ctx, entry, Residual::Same, inputs, dtype_in, residuals, outputs, dtype_out, numels, group_size, scales, zero_points, count, mode);
}

// The single EF calls go through their batch entry with one tensor, which launches the single-tensor kernel.
void piquant_hip_quantize_grouped_ef(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* residual, void* out, piquant_dtype_t dtype_out,
                                     size_t numel, size_t group_size, float* scales, uint8_t* zero_points, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped_ef: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    piquant_hip_quantize_grouped_ef_batch(ctx, &in, dtype_in, &residual, &out, dtype_out, &numel, group_size, &scales, &zero_points, 1, mode);
}

void piquant_hip_reduce_quantize_grouped_ef(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, void* residual, const void* const* inputs,
                                            const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count, void* out,
                                            piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                            piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_reduce_quantize_grouped_ef";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_acc, dtype_out, mode);
    reduce_quantize_grouped(ctx, entry, true, Residual::Same, acc, dtype_acc, residual, inputs, input_scales, input_zero_points, count, out, dtype_out, numel,
                            group_size, scales, zero_points, mode);
}

// Error feedback with the residual's type named: the residual's type equal to the tensor's forwards to the entries above (which draw; the
// forwarding entry does not), a bfloat16 tensor with a float32 residual runs the same bodies with Residual::F32.
void piquant_hip_quantize_grouped_ef_mixed_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* residuals,
                                                 piquant_dtype_t dtype_residual, void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                 size_t group_size, float* const* scales, uint8_t* const* zero_points, size_t count,
                                                 piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_quantize_grouped_ef_mixed_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_in, dtype_out, mode);
    if (residual_kind(entry, dtype_in, dtype_residual) == Residual::Same) {
        piquant_hip_quantize_grouped_ef_batch(ctx, inputs, dtype_in, residuals, outputs, dtype_out, numels, group_size, scales, zero_points, count, mode);
        return;
    }
    quantize_grouped_ef_batch(ctx, entry, Residual::F32, inputs, dtype_in, residuals, outputs, dtype_out, numels, group_size, scales, zero_points, count, mode);
}

void piquant_hip_quantize_grouped_ef_mixed(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* residual, piquant_dtype_t dtype_residual,
                                           void* out, piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                           piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_quantize_grouped_ef_mixed";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_in, dtype_out, mode);
    if (residual_kind(entry, dtype_in, dtype_residual) == Residual::Same) {
        piquant_hip_quantize_grouped_ef(ctx, in, dtype_in, residual, out, dtype_out, numel, group_size, scales, zero_points, mode);
        return;
    }
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    piquant_hip_quantize_grouped_ef_mixed_batch(ctx, &in, dtype_in, &residual, dtype_residual, &out, dtype_out, &numel, group_size, &scales, &zero_points, 1,
                                                mode);
}

void piquant_hip_reduce_quantize_grouped_ef_mixed(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, void* residual,
                                                  piquant_dtype_t dtype_residual, const void* const* inputs, const float* const* input_scales,
                                                  const uint8_t* const* input_zero_points, size_t count, void* out, piquant_dtype_t dtype_out, size_t numel,
                                                  size_t group_size, float* scales, uint8_t* zero_points, piquant_round_mode_t mode) {
    const char* entry = "piquant_hip_reduce_quantize_grouped_ef_mixed";
    if (!ctx) panic("%s: context is NULL", entry);
    check_dynamic_types(dtype_acc, dtype_out, mode);
    if (residual_kind(entry, dtype_acc, dtype_residual) == Residual::Same) {
        piquant_hip_reduce_quantize_grouped_ef(ctx, acc, dtype_acc, residual, inputs, input_scales, input_zero_points, count, out, dtype_out, numel, group_size,
                                               scales, zero_points, mode);
        return;
    }
    reduce_quantize_grouped(ctx, entry, true, Residual::F32, acc, dtype_acc, residual, inputs, input_scales, input_zero_points, count, out, dtype_out, numel,
                            group_size, scales, zero_points, mode);
}

void piquant_hip_quantize_dequantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in_out, void* const* outputs,
                                                   piquant_dtype_t quant_dtype, const size_t* numels, size_t group_size, float* const* scales,
                                                   uint8_t* const* zero_points, size_t count, int params_given, piquant_round_mode_t mode,
                                                   piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_quantize_dequantize_grouped_batch";
    if (!ctx) panic("%s: context is NULL", entry);
    quantize_dequantize_grouped_batch(ctx, entry, false, inputs, dtype_in_out, outputs, quant_dtype, numels, group_size, scales, zero_points, count,
                                      params_given, mode, op);
}

// The single call is a batch of one, which launches the single-tensor kernel; an empty tensor returns behind the argument checks and draws nothing.
void piquant_hip_quantize_dequantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in_out, void* out, piquant_dtype_t quant_dtype,
                                             size_t numel, size_t group_size, float* scales, uint8_t* zero_points, int params_given,
                                             piquant_round_mode_t mode, piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_quantize_dequantize_grouped";
    if (!ctx) panic("%s: context is NULL", entry);
    const bool no_params = !scales && !zero_points;
    quantize_dequantize_grouped_batch(ctx, entry, true, &in, dtype_in_out, &out, quant_dtype, &numel, group_size, no_params ? nullptr : &scales,
                                      no_params ? nullptr : &zero_points, numel == 0 ? 0 : 1, params_given, mode, op);
}

}  // extern "C"
