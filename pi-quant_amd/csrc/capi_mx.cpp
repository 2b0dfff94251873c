// The MX entry points of include/piquant_hip.h (mx_kernels.hpp, mx_reduce_kernels.hpp, mx_ef_kernels.hpp): fixed blocks of 32 FP4 E2M1 / FP8 E4M3
// codes under one E8M0 scale byte -- no groups, no zero points, and the rounding of the stochastic calls is a function of (seed, index) the caller
// passes, so nothing is drawn.  The two single calls and the stochastic quantize (one body: quantize_mx_call, quantize_mx_batch_call), the wire (the fused reduce,
// the dequantize-sum and the two batches) and the three error-feedback calls on a float32 residual.  All are stream-ordered, take device (or pinned) buffers only and read as capi_frame.hpp says; the terms of the
// wire are resolved without allocating (at most kMxMaxInputs a launch, on the stack).
#include "capi_frame.hpp"

using namespace pq;

static_assert(PIQUANT_HIP_MX_FP4_E2M1 == MX_FP4_E2M1 && PIQUANT_HIP_MX_FP8_E4M3 == MX_FP8_E4M3 && PIQUANT_HIP_MX_FP6_E2M3 == MX_FP6_E2M3 &&
                  PIQUANT_HIP_MX_FP6_E3M2 == MX_FP6_E3M2,
              "piquant_hip_mx_format_t and the kernels' format codes");

namespace {

bool is_fp6(piquant_hip_mx_format_t fmt) { return fmt == PIQUANT_HIP_MX_FP6_E2M3 || fmt == PIQUANT_HIP_MX_FP6_E3M2; }

// What every MX call checks first; `float_name` is what the message calls the float side ("input", "output", "float type").  The FP6 formats are
// served by the two single calls only (`fp6`).
void check_mx_call(const Where& w, const piquant_context_t* ctx, const char* float_name, piquant_dtype_t dtype, piquant_hip_mx_format_t fmt,
                   bool fp6 = false) {
    if (!ctx) bad(w, "context is NULL");
    if (dtype != PIQUANT_DTYPE_F32 && dtype != PIQUANT_DTYPE_BF16) bad(w, "the %s must be float32 or bfloat16", float_name);
    if (is_fp6(fmt)) {
        if (!fp6) bad(w, "FP6 is not supported here: the format must be FP4 E2M1 or FP8 E4M3 (FP6 E2M3 / E3M2: quantize_mx and dequantize_mx only)");
    } else if (fmt != PIQUANT_HIP_MX_FP4_E2M1 && fmt != PIQUANT_HIP_MX_FP8_E4M3) {
        bad(w, "the format must be FP4 E2M1, FP8 E4M3, FP6 E2M3 or FP6 E3M2");
    }
}

void check_mx_op(const Where& w, piquant_reduce_op_t op) {
    if (op != PIQUANT_REDUCE_OP_SET && op != PIQUANT_REDUCE_OP_ADD) bad(w, "the reduce op must be SET or ADD");
}

void* mx_float_ptr(const piquant_context_t* ctx, const Where& w, const void* p, piquant_dtype_t dtype) {
    void* dev = device_ptr(w, ctx->resolve_ptr(p));
    check_element_aligned(w, "the float tensor", dev, dtype);
    return dev;
}

// the float32 residual of the error-feedback calls
float* mx_residual_ptr(const piquant_context_t* ctx, const Where& w, float* residual) {
    return static_cast<float*>(mx_float_ptr(ctx, w, residual, PIQUANT_DTYPE_F32));
}

// The scale bytes are classified whatever the context assumes of the tensors the caller passes.
template <class Scales>
Scales* mx_scales_ptr(const Where& w, Scales* scales) {
    return static_cast<Scales*>(device_ptr(w, resolve(scales)));
}

// terms [from, from + n) into `term`; false when one of their buffers is not 16-byte aligned
bool resolve_mx_terms(const piquant_context_t* ctx, const char* entry, const void* const* codes, const uint8_t* const* scales, size_t from, size_t n,
                      MxTerm* term) {
    bool aligned = true;
    for (size_t i = 0; i < n; ++i) {
        const Where w {entry, static_cast<long>(from + i)};
        if (!codes[from + i] || !scales[from + i]) bad(w, "NULL buffer");
        term[i] = MxTerm {device_ptr(w, ctx->resolve_ptr(codes[from + i])), mx_scales_ptr(w, scales[from + i])};
        aligned = aligned && aligned16(term[i].codes) && aligned16(term[i].scales);
    }
    return aligned;
}

// piquant_hip_quantize_mx and piquant_hip_quantize_mx_sr (stochastic: seed and index_base travel by value into the launch)
void quantize_mx_call(const Where& w, piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* codes, uint8_t* scales, size_t numel,
                      piquant_hip_mx_format_t fmt, bool stochastic, uint64_t seed, uint64_t index_base) {
    check_mx_call(w, ctx, "input", dtype_in, fmt, true);
    if (numel == 0) return;
    if (!in || !codes || !scales) bad(w, "NULL buffer");
    const CallLock lock(ctx);
    const MxQuantLaunch q {device_ptr(w, ctx->resolve_ptr(in)), device_ptr(w, ctx->resolve_ptr(codes)), mx_scales_ptr(w, scales), static_cast<int64_t>(numel),
                           dtype_in, fmt, stochastic, seed, index_base};
    check_element_aligned(w, "in", q.in, dtype_in);
    run_call(ctx, false, [&] {
        if (is_fp6(fmt)) launch_quantize_mx_fp6(q, ctx->stream, ctx->num_cu);
        else launch_quantize_mx(q, ctx->stream, ctx->num_cu);
    });
}

// The batches: run_batch's rule, with "streams" meaning every buffer of the member 16-byte aligned; a member that is not runs alone through the
// single launch (the guarded kernel, the same bytes).  index_bases: NULL for the nearest batch, else the stochastic one's (member i: index_bases[i]).
void quantize_mx_batch_call(const char* entry, piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* codes,
                            uint8_t* const* scales, const size_t* numels, size_t count, piquant_hip_mx_format_t fmt, uint64_t seed,
                            const uint64_t* index_bases) {
    check_mx_call(Where {entry}, ctx, "float type", dtype_in, fmt);
    if (count == 0) return;
    if (!inputs || !codes || !scales || !numels) panic("%s: NULL argument", entry);
    const CallLock lock(ctx);
    MxQuantBatchLaunch b {};
    run_call(ctx, false, [&] {
        run_batch(
            b, numels, count,
            [&](size_t i) {
                const Where w {entry, static_cast<long>(i)};
                if (!inputs[i] || !codes[i] || !scales[i]) bad(w, "NULL buffer");
                return MxQuantLaunch {mx_float_ptr(ctx, w, inputs[i], dtype_in), device_ptr(w, ctx->resolve_ptr(codes[i])), mx_scales_ptr(w, scales[i]),
                                      static_cast<int64_t>(numels[i]), dtype_in, fmt, index_bases != nullptr, seed, index_bases ? index_bases[i] : 0};
            },
            [](const MxQuantLaunch& q) { return aligned16(q.in) && aligned16(q.codes) && aligned16(q.scales); },
            [&](const MxQuantLaunch& q) { launch_quantize_mx(q, ctx->stream, ctx->num_cu); },
            [&] { launch_quantize_mx_batch(b, ctx->stream); });
    });
}

}  // namespace

extern "C" {

void piquant_hip_quantize_mx(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* codes, uint8_t* scales, size_t numel,
                             piquant_hip_mx_format_t fmt) {
    quantize_mx_call(Where {"piquant_hip_quantize_mx"}, ctx, in, dtype_in, codes, scales, numel, fmt, false, 0, 0);
}

void piquant_hip_quantize_mx_sr(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* codes, uint8_t* scales, size_t numel,
                                piquant_hip_mx_format_t fmt, uint64_t seed, uint64_t index_base) {
    quantize_mx_call(Where {"piquant_hip_quantize_mx_sr"}, ctx, in, dtype_in, codes, scales, numel, fmt, true, seed, index_base);
}

void piquant_hip_dequantize_mx(piquant_context_t* ctx, const void* codes, const uint8_t* scales, void* out, piquant_dtype_t dtype_out, size_t numel,
                               piquant_hip_mx_format_t fmt, piquant_reduce_op_t op) {
    const Where w {"piquant_hip_dequantize_mx"};
    check_mx_call(w, ctx, "output", dtype_out, fmt, true);
    check_mx_op(w, op);
    if (numel == 0) return;
    if (!codes || !scales || !out) bad(w, "NULL buffer");
    const CallLock lock(ctx);
    const MxDequantLaunch d {device_ptr(w, ctx->resolve_ptr(codes)), mx_scales_ptr(w, scales), device_ptr(w, ctx->resolve_ptr(out)),
                             static_cast<int64_t>(numel), dtype_out, fmt, to_op(op)};
    check_element_aligned(w, "out", d.out, dtype_out);
    // the scale bytes are written by whatever was enqueued just before
    run_call(ctx, true, [&] {
        if (is_fp6(fmt)) launch_dequantize_mx_fp6(d, ctx->stream, ctx->num_cu);
        else launch_dequantize_mx(d, ctx->stream, ctx->num_cu);
    });
}

void piquant_hip_reduce_quantize_mx(piquant_context_t* ctx, const void* acc, piquant_dtype_t dtype_acc, const void* const* codes, const uint8_t* const* scales,
                                    size_t count, void* out_codes, uint8_t* out_scales, size_t numel, piquant_hip_mx_format_t fmt) {
    const char* entry = "piquant_hip_reduce_quantize_mx";
    const Where w {entry};
    check_mx_call(w, ctx, "float type", dtype_acc, fmt);
    if (count > static_cast<size_t>(kMxMaxInputs)) panic("%s: %zu terms, at most %d", entry, count, kMxMaxInputs);
    if (numel == 0) return;
    if (!acc || !out_codes || !out_scales) bad(w, "NULL buffer");
    if (count != 0 && (!codes || !scales)) bad(w, "NULL term list");
    const CallLock lock(ctx);
    MxReduceLaunch r {mx_float_ptr(ctx, w, acc, dtype_acc), device_ptr(w, ctx->resolve_ptr(out_codes)), mx_scales_ptr(w, out_scales),
                      static_cast<int64_t>(numel), dtype_acc, fmt, {}, static_cast<int>(count)};
    const bool aligned = resolve_mx_terms(ctx, entry, codes, scales, 0, count, r.term) && aligned16(r.acc) && aligned16(r.codes) && aligned16(r.scales);
    // acc and the terms are written by what was enqueued before: always behind it
    run_call(ctx, true, [&] { launch_reduce_quantize_mx(r, !aligned, ctx->stream, ctx->num_cu); });
}

// Everything 16-byte aligned: one launch per kMxMaxInputs terms, the first with the call's op and the others ADD -- the composition rounds to
// dtype_out at every term, so where the launches are cut changes no byte.  Anything misaligned: the composition itself, one dequantize_mx per term.
void piquant_hip_dequantize_sum_mx(piquant_context_t* ctx, const void* const* codes, const uint8_t* const* scales, size_t count, void* out,
                                   piquant_dtype_t dtype_out, size_t numel, piquant_hip_mx_format_t fmt, piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_dequantize_sum_mx";
    const Where w {entry};
    check_mx_call(w, ctx, "float type", dtype_out, fmt);
    check_mx_op(w, op);
    if (count == 0) bad(w, "no terms (count must be at least 1)");
    if (!codes || !scales) bad(w, "NULL term list");
    if (numel == 0) return;
    if (!out) bad(w, "NULL buffer");
    const CallLock lock(ctx);
    void* out_dev = mx_float_ptr(ctx, w, out, dtype_out);
    bool aligned = aligned16(out_dev);
    for (size_t from = 0; from < count; from += kMxMaxInputs) {   // every term is checked before anything is launched
        MxTerm term[kMxMaxInputs];
        aligned = resolve_mx_terms(ctx, entry, codes, scales, from, std::min(count - from, static_cast<size_t>(kMxMaxInputs)), term) && aligned;
    }
    // the terms and an ADD's out are written by what was enqueued before: always behind it
    run_call(ctx, true, [&] {
        for (size_t from = 0; from < count; from += kMxMaxInputs) {
            const size_t n = std::min(count - from, static_cast<size_t>(kMxMaxInputs));
            MxDequantSumLaunch d {out_dev, static_cast<int64_t>(numel), dtype_out, fmt, from == 0 ? to_op(op) : OP_ADD, {}, static_cast<int>(n)};
            resolve_mx_terms(ctx, entry, codes, scales, from, n, d.term);
            if (aligned) {
                launch_dequantize_sum_mx(d, ctx->stream);
                continue;
            }
            for (size_t i = 0; i < n; ++i)
                launch_dequantize_mx(MxDequantLaunch {d.term[i].codes, d.term[i].scales, out_dev, d.numel, dtype_out, fmt, i == 0 ? d.op : OP_ADD}, ctx->stream,
                                     ctx->num_cu);
        }
    });
}

void piquant_hip_quantize_mx_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* codes, uint8_t* const* scales,
                                   const size_t* numels, size_t count, piquant_hip_mx_format_t fmt) {
    quantize_mx_batch_call("piquant_hip_quantize_mx_batch", ctx, inputs, dtype_in, codes, scales, numels, count, fmt, 0, nullptr);
}

void piquant_hip_quantize_mx_sr_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* codes,
                                      uint8_t* const* scales, const size_t* numels, size_t count, piquant_hip_mx_format_t fmt, uint64_t seed,
                                      const uint64_t* index_bases) {
    const char* entry = "piquant_hip_quantize_mx_sr_batch";
    if (count != 0 && !index_bases) panic("%s: NULL argument", entry);
    quantize_mx_batch_call(entry, ctx, inputs, dtype_in, codes, scales, numels, count, fmt, seed, index_bases);
}

// run_batch's rule again (quantize_mx_batch_call has it).
void piquant_hip_dequantize_mx_batch(piquant_context_t* ctx, const void* const* codes, const uint8_t* const* scales, void* const* outputs,
                                     piquant_dtype_t dtype_out, const size_t* numels, size_t count, piquant_hip_mx_format_t fmt, piquant_reduce_op_t op) {
    const char* entry = "piquant_hip_dequantize_mx_batch";
    check_mx_call(Where {entry}, ctx, "float type", dtype_out, fmt);
    check_mx_op(Where {entry}, op);
    if (count == 0) return;
    if (!codes || !scales || !outputs || !numels) panic("%s: NULL argument", entry);
    const CallLock lock(ctx);
    MxDequantBatchLaunch b {};
    // the scale bytes are written by whatever was enqueued just before
    run_call(ctx, true, [&] {
        run_batch(
            b, numels, count,
            [&](size_t i) {
                const Where w {entry, static_cast<long>(i)};
                if (!codes[i] || !scales[i] || !outputs[i]) bad(w, "NULL buffer");
                return MxDequantLaunch {device_ptr(w, ctx->resolve_ptr(codes[i])), mx_scales_ptr(w, scales[i]), mx_float_ptr(ctx, w, outputs[i], dtype_out),
                                        static_cast<int64_t>(numels[i]), dtype_out, fmt, to_op(op)};
            },
            [](const MxDequantLaunch& d) { return aligned16(d.codes) && aligned16(d.scales) && aligned16(d.out); },
            [&](const MxDequantLaunch& d) { launch_dequantize_mx(d, ctx->stream, ctx->num_cu); },
            [&] { launch_dequantize_mx_batch(b, ctx->stream); });
    });
}

// ---- error feedback (mx_ef_kernels.hpp): the residual is float32 and read: every call runs behind what was enqueued before it ----

void piquant_hip_quantize_mx_ef(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, float* residual, void* codes, uint8_t* scales, size_t numel,
                                piquant_hip_mx_format_t fmt) {
    const Where w {"piquant_hip_quantize_mx_ef"};
    check_mx_call(w, ctx, "input", dtype_in, fmt);
    if (numel == 0) return;
    if (!in || !residual || !codes || !scales) bad(w, "NULL buffer");
    const CallLock lock(ctx);
    const MxEfLaunch q {mx_float_ptr(ctx, w, in, dtype_in), mx_residual_ptr(ctx, w, residual), device_ptr(w, ctx->resolve_ptr(codes)), mx_scales_ptr(w, scales),
                        static_cast<int64_t>(numel), dtype_in, fmt};
    run_call(ctx, true, [&] { launch_quantize_mx_ef(q, ctx->stream, ctx->num_cu); });
}

void piquant_hip_quantize_mx_ef_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, float* const* residuals, void* const* codes,
                                      uint8_t* const* scales, const size_t* numels, size_t count, piquant_hip_mx_format_t fmt) {
    const char* entry = "piquant_hip_quantize_mx_ef_batch";
    check_mx_call(Where {entry}, ctx, "float type", dtype_in, fmt);
    if (count == 0) return;
    if (!inputs || !residuals || !codes || !scales || !numels) panic("%s: NULL argument", entry);
    const CallLock lock(ctx);
    MxEfBatchLaunch b {};
    run_call(ctx, true, [&] {
        run_batch(
            b, numels, count,
            [&](size_t i) {
                const Where w {entry, static_cast<long>(i)};
                if (!inputs[i] || !residuals[i] || !codes[i] || !scales[i]) bad(w, "NULL buffer");
                return MxEfLaunch {mx_float_ptr(ctx, w, inputs[i], dtype_in), mx_residual_ptr(ctx, w, residuals[i]), device_ptr(w, ctx->resolve_ptr(codes[i])),
                                   mx_scales_ptr(w, scales[i]), static_cast<int64_t>(numels[i]), dtype_in, fmt};
            },
            [](const MxEfLaunch& q) { return aligned16(q.in) && aligned16(q.residual) && aligned16(q.codes) && aligned16(q.scales); },
            [&](const MxEfLaunch& q) { launch_quantize_mx_ef(q, ctx->stream, ctx->num_cu); },
            [&] { launch_quantize_mx_ef_batch(b, ctx->stream); });
    });
}

void piquant_hip_reduce_quantize_mx_ef(piquant_context_t* ctx, const void* acc, piquant_dtype_t dtype_acc, float* residual, const void* const* codes,
                                       const uint8_t* const* scales, size_t count, void* out_codes, uint8_t* out_scales, size_t numel,
                                       piquant_hip_mx_format_t fmt) {
    const char* entry = "piquant_hip_reduce_quantize_mx_ef";
    const Where w {entry};
    check_mx_call(w, ctx, "float type", dtype_acc, fmt);
    if (count > static_cast<size_t>(kMxMaxInputs)) panic("%s: %zu terms, at most %d", entry, count, kMxMaxInputs);
    if (numel == 0) return;
    if (!acc || !residual || !out_codes || !out_scales) bad(w, "NULL buffer");
    if (count != 0 && (!codes || !scales)) bad(w, "NULL term list");
    const CallLock lock(ctx);
    MxReduceEfLaunch r {mx_float_ptr(ctx, w, acc, dtype_acc), mx_residual_ptr(ctx, w, residual), device_ptr(w, ctx->resolve_ptr(out_codes)),
                        mx_scales_ptr(w, out_scales), static_cast<int64_t>(numel), dtype_acc, fmt, {}, static_cast<int>(count)};
    const bool aligned = resolve_mx_terms(ctx, entry, codes, scales, 0, count, r.term) && aligned16(r.acc) && aligned16(r.residual) && aligned16(r.codes) &&
                         aligned16(r.scales);
    run_call(ctx, true, [&] { launch_reduce_quantize_mx_ef(r, !aligned, ctx->stream, ctx->num_cu); });
}

}  // extern "C"
