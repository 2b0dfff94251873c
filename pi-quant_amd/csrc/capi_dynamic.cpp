// The additive entry points of include/piquant_hip.h that have no twin in piquant.h: one-pass sums and batches of dequantize,
// the reference's C++-only quantize_dequantize_fused, and compute_quant_params + quantize as one call (one launch when the tensor
// fits on the chip), its batched form and the reduce variant.
#include "context.hpp"

#include <cstring>

using namespace pq;

// out (op)= sum of the dequantized inputs, stream-ordered; caller holds ctx->mu and the device guard, and waits if the context is blocking
static void dequantize_sum_locked(piquant_context_t* ctx, const void* const* inputs, const piquant_hip_params_t* const* device_params, size_t count,
                                  piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel, piquant_reduce_op_t op) {
    const Resolved rout = ctx->resolve_ptr(out);
    if (rout.pageable) panic("piquant_hip_dequantize_sum needs device (or pinned) buffers");
    // more inputs than one launch takes: the first launch carries the caller's op, the following ones accumulate
    for (size_t first = 0; first < count; first += kDequantSumMaxInputs) {
        DequantSumLaunch d {};
        d.count = static_cast<int>(std::min<size_t>(kDequantSumMaxInputs, count - first));
        for (int i = 0; i < d.count; ++i) {
            if (!inputs[first + i] || !device_params[first + i]) panic("dequantize_sum: NULL input %zu", first + i);
            const Resolved ri = ctx->resolve_ptr(inputs[first + i]), rp = resolve(device_params[first + i]);
            if (ri.pageable || rp.pageable) panic("piquant_hip_dequantize_sum needs device (or pinned) buffers");
            d.in[i] = ri.dev;
            d.params[i] = rp.dev;
        }
        d.out = rout.dev;
        d.numel = static_cast<int64_t>(numel);
        d.dt_in = dtype_in;
        d.dt_out = dtype_out;
        d.op = (first == 0 && op == PIQUANT_REDUCE_OP_SET) ? OP_SET : OP_ADD;
        launch_dequantize_sum(d, ctx->stream, ctx->num_cu);
    }
}

extern "C" {

void piquant_hip_dequantize_sum(piquant_context_t* ctx, const void* const* inputs, const piquant_hip_params_t* const* device_params, size_t count,
                                piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel, piquant_reduce_op_t op) {
    if (!ctx) panic("piquant_hip_dequantize_sum: context is NULL");
    const dtype_row& dti = dtype_of(dtype_in);
    const dtype_row& dto = dtype_of(dtype_out);
    if (!dti.quant) panic("dequantize: input dtype (%s) must be a quantized type", dti.name);
    if (dto.quant) panic("dequantize: output dtype (%s) must be a dequantized type", dto.name);
    if (op != PIQUANT_REDUCE_OP_SET && op != PIQUANT_REDUCE_OP_ADD) panic("dequantize: invalid reduce op %d", static_cast<int>(op));
    if (count == 0 || numel == 0) return;
    if (!inputs || !device_params || !out) panic("dequantize_sum: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    dequantize_sum_locked(ctx, inputs, device_params, count, dtype_in, out, dtype_out, numel, op);
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_dequantize_dp_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                     piquant_dtype_t dtype_out, const size_t* numels, const piquant_hip_params_t* const* device_params, size_t count,
                                     piquant_reduce_op_t op) {
    if (!ctx) panic("piquant_hip_dequantize_dp_batch: context is NULL");
    const dtype_row& dti = dtype_of(dtype_in);
    const dtype_row& dto = dtype_of(dtype_out);
    if (!dti.quant) panic("dequantize: input dtype (%s) must be a quantized type", dti.name);
    if (dto.quant) panic("dequantize: output dtype (%s) must be a dequantized type", dto.name);
    if (op != PIQUANT_REDUCE_OP_SET && op != PIQUANT_REDUCE_OP_ADD) panic("dequantize: invalid reduce op %d", static_cast<int>(op));
    if (count == 0) return;
    if (!inputs || !outputs || !numels || !device_params) panic("piquant_hip_dequantize_dp_batch: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    size_t i = 0;
    while (i < count) {
        DequantBatchLaunch d {};
        d.dt_in = dtype_in;
        d.dt_out = dtype_out;
        d.op = op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET;
        while (i < count && d.count < kDequantBatchMaxInputs) {
            if (numels[i] != 0) {
                if (!inputs[i] || !outputs[i] || !device_params[i]) panic("dequantize: NULL buffer %zu", i);
                const Resolved ri = ctx->resolve_ptr(inputs[i]), ro = ctx->resolve_ptr(outputs[i]), rp = resolve(device_params[i]);
                if (ri.pageable || ro.pageable || rp.pageable) panic("piquant_hip_dequantize_dp_batch needs device (or pinned) buffers");
                d.in[d.count] = ri.dev;
                d.out[d.count] = ro.dev;
                d.params[d.count] = rp.dev;
                d.numel[d.count] = static_cast<int64_t>(numels[i]);
                ++d.count;
            }
            ++i;
        }
        launch_dequantize_batch(d, ctx->stream);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_dequantize(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in_out, void* out, piquant_dtype_t quant_dtype,
                                     size_t numel, float scale, int64_t zero_point, piquant_round_mode_t mode, piquant_reduce_op_t op) {
    if (!ctx) panic("piquant_hip_quantize_dequantize: context is NULL");
    // reference src/piquant.cpp:353-355
    if (dtype_of(dtype_in_out).quant) panic("quantize_dequantize: input dtype must be a dequantized type");
    if (!dtype_of(quant_dtype).quant) panic("quantize_dequantize: quant dtype must be a quantized type");
    if (mode != PIQUANT_NEAREST && mode != PIQUANT_STOCHASTIC) panic("quantize_dequantize: invalid round mode %d", static_cast<int>(mode));
    if (op != PIQUANT_REDUCE_OP_SET && op != PIQUANT_REDUCE_OP_ADD) panic("quantize_dequantize: invalid reduce op %d", static_cast<int>(op));
    if (numel == 0) return;
    if (!in || !out) panic("quantize_dequantize: NULL buffer");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved rin = ctx->resolve_ptr(in), rout = ctx->resolve_ptr(out);
    if (rin.pageable || rout.pageable) panic("quantize_dequantize: device (or pinned) buffers required");
    RequantLaunch r {};
    r.in = rin.dev;
    r.out = rout.dev;
    r.numel = static_cast<int64_t>(numel);
    r.dt_inout = dtype_in_out;
    r.quant_dtype = quant_dtype;
    r.op = op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET;
    r.scale = scale;
    {   // bfp16_t(scale): round to nearest even, NaN quieted (reference include/piquant.hpp:86-90)
        uint32_t u;
        __builtin_memcpy(&u, &scale, 4);
        uint32_t b = (u & 0x7fffffffu) > 0x7f800000u ? ((u >> 16) | 64u) : ((u + (0x7fffu + ((u >> 16) & 1u))) >> 16);
        b <<= 16;
        __builtin_memcpy(&r.scale_bf16, &b, 4);
    }
    r.inv_scale = 1.0f / scale;
    r.zero_point = zero_point;
    if (mode == PIQUANT_NEAREST) r.round_mode = RM_NEAREST_I64;
    else if (ctx->per_element) {
        r.round_mode = RM_STOCH_ELEM;
        r.seed = ctx->elem_seed;
        r.index_base = ctx->elem_base;
    } else {
        r.round_mode = RM_STOCH_CALL;
        r.threshold = draw_threshold(ctx);
    }
    launch_requantize(r, ctx->stream, ctx->num_cu);
    if (ctx->blocking) wait_stream(ctx);
}

// compute_quant_params + quantize of ONE tensor on resolved device pointers; `q` carries dtypes and the round-mode fields.
// Caller holds ctx->mu and the device guard.
static void quantize_dynamic_one(piquant_context_t* ctx, QuantLaunch q, const void* in_dev, void* out_dev, size_t numel,
                                 void* params_dev) {
    MinmaxAction params_action;
    params_action.action = MM_PARAMS;
    params_action.bits = dtype_of(static_cast<piquant_dtype_t>(q.dt_out)).bits;
    params_action.dst = params_dev;
    if (numel == 0) {   // parameters of an empty tensor: the device epilogue writes the degenerate record (1.0, qmax >> 1) for the armed identities
        scan(ctx, nullptr, static_cast<piquant_dtype_t>(q.dt_in), 0, params_action);
        return;
    }
    q.in = in_dev;
    q.out = out_dev;
    q.numel = static_cast<int64_t>(numel);
    q.ref_out_align = -1;   // the one-launch call is position-independent whatever the context's layout mode says (include/piquant_hip.h)
    // One launch with the tensor held on chip between the scan and the quantization when it fits; otherwise (or with fusion
    // switched off) the same result from two launches: the scan, whose last block writes the record, and a quantize that reads it.
    bool fused = false;
    if (ctx->fusion && fused_launch_applies(q, ctx->num_cu)) {
        order_context_state(ctx);
                FusedLaunchOrder order(ctx->device, ctx->stream);
        q.barrier_timeout_us = ctx->barrier_timeout_us;
        fused = launch_fused_params_quantize(q, ctx->d_fused, params_dev, ctx->stream, ctx->num_cu);
    }
    if (!fused) {
        scan(ctx, in_dev, static_cast<piquant_dtype_t>(q.dt_in), numel, params_action);
        q.dyn_params = params_dev;
        launch_quantize(q, ctx->stream, ctx->num_cu);
    }
}

static void check_dynamic_types(piquant_dtype_t dtype_in, piquant_dtype_t dtype_out, piquant_round_mode_t mode) {
    const dtype_row& dti = dtype_of(dtype_in);
    const dtype_row& dto = dtype_of(dtype_out);
    if (dti.quant) panic("quantize: input dtype (%s) must be a dequantized type", dti.name);
    if (!dto.quant) panic("quantize: output dtype (%s) must be a quantized type", dto.name);
    if (mode != PIQUANT_NEAREST && mode != PIQUANT_STOCHASTIC) panic("quantize: invalid round mode %d", static_cast<int>(mode));
}

void piquant_hip_quantize_dynamic(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel,
                                  piquant_hip_params_t* device_params, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_dynamic: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    if (!device_params) panic("piquant_hip_quantize_dynamic: NULL parameter record");
    if (numel != 0 && (!in || !out)) panic("quantize: NULL buffer");

    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved rp = resolve(device_params);
    if (rp.pageable) panic("piquant_hip_quantize_dynamic: the parameter record must live in device (or pinned) memory");
    QuantLaunch q {};
    q.dt_in = dtype_in;
    q.dt_out = dtype_out;
    fill_round_mode(ctx, q, mode);
    if (numel == 0) {
        quantize_dynamic_one(ctx, q, nullptr, nullptr, 0, rp.dev);
    } else {
        const Resolved rin = ctx->resolve_ptr(in), rout = ctx->resolve_ptr(out);
        if (rin.pageable || rout.pageable) panic("piquant_hip_quantize_dynamic needs device (or pinned) buffers");
        quantize_dynamic_one(ctx, q, rin.dev, rout.dev, numel, rp.dev);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_dynamic_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                        piquant_dtype_t dtype_out, const size_t* numels, piquant_hip_params_t* const* device_params, size_t count,
                                        piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_dynamic_batch: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    if (count == 0) return;
    if (!inputs || !outputs || !numels || !device_params) panic("piquant_hip_quantize_dynamic_batch: NULL argument");

    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    QuantLaunch q {};
    q.dt_in = dtype_in;
    q.dt_out = dtype_out;
    fill_round_mode(ctx, q, mode);   // stochastic: ONE threshold for the whole batch, as one call of the reference has one
    struct Item {
        const void* in;
        void* out;
        size_t numel;
        void* params;
    };
    std::vector<Item> items(count);
    for (size_t i = 0; i < count; ++i) {
        if (!device_params[i]) panic("piquant_hip_quantize_dynamic_batch: NULL parameter record %zu", i);
        const Resolved rp = resolve(device_params[i]);
        if (rp.pageable) panic("piquant_hip_quantize_dynamic_batch: parameter records must live in device (or pinned) memory");
        items[i] = {nullptr, nullptr, numels[i], rp.dev};
        if (numels[i] == 0) continue;
        if (!inputs[i] || !outputs[i]) panic("quantize: NULL buffer %zu", i);
        const Resolved rin = ctx->resolve_ptr(inputs[i]), rout = ctx->resolve_ptr(outputs[i]);
        if (rin.pageable || rout.pageable) panic("piquant_hip_quantize_dynamic_batch needs device (or pinned) buffers");
        items[i].in = rin.dev;
        items[i].out = rout.dev;
    }
    // Up to kFusedBatchMax non-empty tensors per launch: one sub-grid, one barrier, one parameter record each.  Whatever does not
    // qualify (fusion off, reference-layout mode, a misaligned or oversized tensor in the group) goes one tensor at a time.
    size_t i = 0;
    while (i < count) {
        FusedBatch b {};
        size_t j = i;
        while (j < count && b.count < kFusedBatchMax) {
            if (items[j].numel != 0) {
                b.in[b.count] = items[j].in;
                b.out[b.count] = items[j].out;
                b.numel[b.count] = static_cast<int64_t>(items[j].numel);
                b.params[b.count] = items[j].params;
                ++b.count;
            }
            ++j;
        }
        bool fused = false;
        if (ctx->fusion && !ctx->reference_layout && b.count > 1) {
            order_context_state(ctx);
                FusedLaunchOrder order(ctx->device, ctx->stream);
            q.barrier_timeout_us = ctx->barrier_timeout_us;
            fused = launch_fused_params_quantize_batch(q, b, ctx->d_fused, ctx->stream, ctx->num_cu);
        }
        for (size_t k = i; k < j; ++k) {
            if (fused && items[k].numel != 0) continue;
            quantize_dynamic_one(ctx, q, items[k].in, items[k].out, items[k].numel, items[k].params);
        }
        i = j;
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_reduce_quantize_dynamic(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, const void* const* inputs,
                                         const piquant_hip_params_t* const* input_params, size_t count, void* out, piquant_dtype_t dtype_out, size_t numel,
                                         piquant_hip_params_t* device_params, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_reduce_quantize_dynamic: context is NULL");
    check_dynamic_types(dtype_acc, dtype_out, mode);
    if (!device_params) panic("piquant_hip_reduce_quantize_dynamic: NULL parameter record");
    if (numel == 0 || count == 0) {   // nothing to add (or nothing at all): the plain call
        piquant_hip_quantize_dynamic(ctx, acc, dtype_acc, out, dtype_out, numel, device_params, mode);
        return;
    }
    if (!acc || !out || !inputs || !input_params) panic("piquant_hip_reduce_quantize_dynamic: NULL argument");
    // ONE critical section for the whole call: the per-call stochastic threshold is drawn once and handed down in the launch descriptor to
    // whichever path runs (a fused attempt that does not qualify and the two-step path behind it must quantize with the SAME draw, or the bytes
    // -- and every later draw of a seeded context -- would depend on whether fusion was tried); no shared context state is touched for it.
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved rp = resolve(device_params), racc = ctx->resolve_ptr(acc), rout = ctx->resolve_ptr(out);
    if (rp.pageable || racc.pageable || rout.pageable) panic("piquant_hip_reduce_quantize_dynamic needs device (or pinned) buffers");
    QuantLaunch q {};
    q.dt_in = dtype_acc;
    q.dt_out = dtype_out;
    fill_round_mode(ctx, q, mode);
    bool fused = false;
    if (ctx->fusion && !ctx->reference_layout && count <= static_cast<size_t>(kDequantSumMaxInputs)) {
        QuantLaunch f = q;
        f.in = racc.dev;
        f.out = rout.dev;
        f.numel = static_cast<int64_t>(numel);
        DequantSumLaunch terms {};
        terms.count = static_cast<int>(count);
        terms.dt_in = dtype_out;
        for (size_t i = 0; i < count; ++i) {
            if (!inputs[i] || !input_params[i]) panic("piquant_hip_reduce_quantize_dynamic: NULL input %zu", i);
            const Resolved ri = ctx->resolve_ptr(inputs[i]), rq = resolve(input_params[i]);
            if (ri.pageable || rq.pageable) panic("piquant_hip_reduce_quantize_dynamic needs device (or pinned) buffers");
            terms.in[i] = ri.dev;
            terms.params[i] = rq.dev;
        }
        order_context_state(ctx);
        FusedLaunchOrder order(ctx->device, ctx->stream);
        f.barrier_timeout_us = ctx->barrier_timeout_us;
        fused = launch_fused_reduce_quantize(f, terms, ctx->d_fused, rp.dev, ctx->stream, ctx->num_cu);
    }
    if (!fused) {
        // the same result in two steps (and with `acc` updated on the way): one-pass sum into acc, then parameters + quantize with q's round mode
        dequantize_sum_locked(ctx, inputs, input_params, count, dtype_out, acc, dtype_acc, numel, PIQUANT_REDUCE_OP_ADD);
        quantize_dynamic_one(ctx, q, racc.dev, rout.dev, numel, rp.dev);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_signal_flags(piquant_context_t* ctx, uint32_t* const* flags, size_t count, uint32_t value) {
    if (!ctx) panic("piquant_hip_signal_flags: context is NULL");
    if (count == 0) return;
    if (!flags) panic("piquant_hip_signal_flags: NULL flag list");
    for (size_t i = 0; i < count; ++i)
        if (!flags[i]) panic("piquant_hip_signal_flags: NULL flag %zu", i);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    peer_timeout_pending(ctx, "piquant_hip_signal_flags");
    launch_signal_flags(flags, static_cast<int>(count), value, peer_timeout_record_dev(ctx), ctx->stream);
}

void piquant_hip_wait_flags(piquant_context_t* ctx, const uint32_t* flags, size_t count, uint32_t value, uint32_t timeout_us) {
    if (!ctx) panic("piquant_hip_wait_flags: context is NULL");
    if (count == 0) return;
    if (!flags) panic("piquant_hip_wait_flags: NULL flag array");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    if (stream_is_capturing(ctx->stream)) panic("piquant_hip_wait_flags cannot be captured into a hipGraph: the value waited for changes with every exchange");
    peer_timeout_pending(ctx, "piquant_hip_wait_flags");
    launch_wait_flags(flags, static_cast<int>(count), value, timeout_us, peer_timeout_record_dev(ctx), ctx->stream);
}

void* piquant_hip_peer_alloc(piquant_context_t* ctx, size_t bytes, int fine_grained, uint32_t fill_word, void* out_ipc_handle) {
    if (!ctx) panic("piquant_hip_peer_alloc: context is NULL");
    if (bytes == 0 || bytes % 4 != 0) panic("piquant_hip_peer_alloc: %zu bytes (a positive multiple of 4 is needed)", bytes);
    if (!out_ipc_handle) panic("piquant_hip_peer_alloc: NULL handle buffer");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    void* p = nullptr;
    // fine-grained: words ANOTHER device writes while a kernel of this one polls them (flags, mailboxes) -- coarse-grained device memory
    // is only coherent with other agents at kernel boundaries
    if (fine_grained) PQ_HIP(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained));
    else PQ_HIP(hipMalloc(&p, bytes));
    PQ_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), static_cast<int>(fill_word), bytes / 4));
    PQ_HIP(hipDeviceSynchronize());
    static_assert(sizeof(hipIpcMemHandle_t) == PIQUANT_HIP_IPC_HANDLE_BYTES, "IPC handle size");
    hipIpcMemHandle_t h;
    PQ_HIP(hipIpcGetMemHandle(&h, p));
    std::memcpy(out_ipc_handle, &h, sizeof h);
    return p;
}

void* piquant_hip_peer_open(piquant_context_t* ctx, const void* ipc_handle) {
    if (!ctx) panic("piquant_hip_peer_open: context is NULL");
    if (!ipc_handle) panic("piquant_hip_peer_open: NULL handle");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipIpcMemHandle_t h;
    std::memcpy(&h, ipc_handle, sizeof h);
    void* p = nullptr;
    PQ_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));   // maps the peer's allocation for THIS device (peer access enabled on the way)
    return p;
}

void piquant_hip_peer_close(piquant_context_t* ctx, void* mapped) {
    if (!ctx) panic("piquant_hip_peer_close: context is NULL");
    if (!mapped) return;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    PQ_HIP(hipIpcCloseMemHandle(mapped));
}

void piquant_hip_peer_free(piquant_context_t* ctx, void* allocated) {
    if (!ctx) panic("piquant_hip_peer_free: context is NULL");
    if (!allocated) return;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    PQ_HIP(hipFree(allocated));
}

void piquant_hip_exchange_minmax_keys(piquant_context_t* ctx, const int32_t* device_keys, uint64_t* const* peer_slots, uint64_t* my_slots, size_t count,
                                      int32_t* out_keys, uint32_t timeout_us) {
    if (!ctx) panic("piquant_hip_exchange_minmax_keys: context is NULL");
    if (!device_keys || !peer_slots || !my_slots || !out_keys) panic("piquant_hip_exchange_minmax_keys: NULL argument");
    if (count < 1 || count > static_cast<size_t>(kKeyExchangeMaxRanks)) panic("piquant_hip_exchange_minmax_keys: %zu ranks (1..%d supported)", count, kKeyExchangeMaxRanks);
    for (size_t i = 0; i < count; ++i)
        if (!peer_slots[i]) panic("piquant_hip_exchange_minmax_keys: NULL slot of rank %zu", i);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    if (stream_is_capturing(ctx->stream)) panic("piquant_hip_exchange_minmax_keys cannot be captured into a hipGraph: the mailbox parity changes with every exchange");
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "mailbox words");
    peer_timeout_pending(ctx, "piquant_hip_exchange_minmax_keys");
    launch_exchange_keys(device_keys, reinterpret_cast<unsigned long long* const*>(peer_slots), reinterpret_cast<unsigned long long*>(my_slots), static_cast<int>(count),
                         out_keys, timeout_us, peer_timeout_record_dev(ctx), ctx->stream);
}

int piquant_hip_peer_timeout(piquant_context_t* ctx, uint32_t* out_rank, uint32_t* out_expected, uint32_t* out_seen) {
    if (!ctx) panic("piquant_hip_peer_timeout: context is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->done_dev) return 0;
    volatile uint32_t* rec = ctx->done + kPeerTimeoutRecordWord;
    const uint32_t kind = __atomic_load_n(rec + 0, __ATOMIC_ACQUIRE);
    if (kind == kPeerTimeoutNone) return 0;
    if (out_rank) *out_rank = rec[1];
    if (out_expected) *out_expected = rec[2];
    if (out_seen) *out_seen = rec[3];
    __atomic_store_n(rec + 0, static_cast<uint32_t>(kPeerTimeoutNone), __ATOMIC_RELEASE);   // reported: cleared
    return static_cast<int>(kind);
}

}  // extern "C"

extern "C" {

// Group-wise quantization (include/piquant_hip.h): one launch each, stream-ordered, device (or pinned) buffers only.
static void check_group_size(size_t group_size) {
    if (group_size < static_cast<size_t>(kGroupedMinG) || group_size > static_cast<size_t>(kGroupedMaxG) || (group_size & (group_size - 1)) != 0)
        panic("group size %zu is not a power of two in [%d, %d]", group_size, kGroupedMinG, kGroupedMaxG);
}

void piquant_hip_quantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel,
                                  size_t group_size, float* scales, uint8_t* zero_points, int params_given, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (numel == 0) return;
    if (!in || !out || !scales || !zero_points) panic("quantize_grouped: NULL buffer");
    if (reinterpret_cast<uintptr_t>(scales) % 4 != 0) panic("quantize_grouped: scales must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved rin = ctx->resolve_ptr(in), rout = ctx->resolve_ptr(out), rs = resolve(scales), rz = resolve(zero_points);
    if (rin.pageable || rout.pageable || rs.pageable || rz.pageable) panic("piquant_hip_quantize_grouped needs device (or pinned) buffers");
    QuantLaunch rm {};
    fill_round_mode(ctx, rm, mode);   // the call's one threshold (or the per-element seed and base), as quantize_uniform draws it
    GroupedQuantLaunch q {};
    q.in = rin.dev;
    q.out = rout.dev;
    q.numel = static_cast<int64_t>(numel);
    q.group_size = static_cast<int64_t>(group_size);
    q.scales = static_cast<float*>(rs.dev);
    q.zero_points = static_cast<uint8_t*>(rz.dev);
    q.params_given = params_given != 0;
    q.dt_in = dtype_in;
    q.dt_out = dtype_out;
    q.round_mode = rm.round_mode;
    q.threshold = rm.threshold;
    q.seed = rm.seed;
    q.index_base = rm.index_base;
    {
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, q.params_given);
        launch_quantize_grouped(q, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_dequantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel,
                                    size_t group_size, const float* scales, const uint8_t* zero_points, piquant_reduce_op_t op) {
    if (!ctx) panic("piquant_hip_dequantize_grouped: context is NULL");
    const dtype_row& dti = dtype_of(dtype_in);
    const dtype_row& dto = dtype_of(dtype_out);
    if (!dti.quant) panic("dequantize: input dtype (%s) must be a quantized type", dti.name);
    if (dto.quant) panic("dequantize: output dtype (%s) must be a dequantized type", dto.name);
    if (op != PIQUANT_REDUCE_OP_SET && op != PIQUANT_REDUCE_OP_ADD) panic("dequantize: invalid reduce op %d", static_cast<int>(op));
    check_group_size(group_size);
    if (numel == 0) return;
    if (!in || !out || !scales || !zero_points) panic("dequantize_grouped: NULL buffer");
    if (reinterpret_cast<uintptr_t>(scales) % 4 != 0) panic("dequantize_grouped: scales must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved rin = ctx->resolve_ptr(in), rout = ctx->resolve_ptr(out), rs = resolve(scales), rz = resolve(zero_points);
    if (rin.pageable || rout.pageable || rs.pageable || rz.pageable) panic("piquant_hip_dequantize_grouped needs device (or pinned) buffers");
    GroupedDequantLaunch d {};
    d.in = rin.dev;
    d.out = rout.dev;
    d.numel = static_cast<int64_t>(numel);
    d.group_size = static_cast<int64_t>(group_size);
    d.scales = static_cast<const float*>(rs.dev);
    d.zero_points = static_cast<const uint8_t*>(rz.dev);
    d.dt_in = dtype_in;
    d.dt_out = dtype_out;
    d.op = op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET;
    {
        StopEventScope completion(ctx);
        IndependentCallScope independent(ctx, true);   // the parameters are written by whatever was enqueued just before
        launch_dequantize_grouped(d, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

}  // extern "C"

extern "C" {

// Batches and the fused reduce of the group-wise calls (include/piquant_hip.h): stream-ordered, device (or pinned) buffers only, no allocation.
static inline bool grouped_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

void piquant_hip_quantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                        piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, float* const* scales,
                                        uint8_t* const* zero_points, size_t count, int params_given, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped_batch: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (count == 0) return;
    if (!inputs || !outputs || !numels || !scales || !zero_points) panic("piquant_hip_quantize_grouped_batch: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    QuantLaunch rm {};
    fill_round_mode(ctx, rm, mode);   // ONE threshold (or per-element seed and base) for the whole batch
    GroupedQuantBatchLaunch b {};
    b.group_size = static_cast<int64_t>(group_size);
    b.params_given = params_given != 0;
    b.dt_in = dtype_in;
    b.dt_out = dtype_out;
    b.round_mode = rm.round_mode;
    b.threshold = rm.threshold;
    b.seed = rm.seed;
    b.index_base = rm.index_base;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, b.params_given);
    for (size_t i = 0; i < count; ++i) {
        if (numels[i] == 0) continue;
        if (!inputs[i] || !outputs[i] || !scales[i] || !zero_points[i]) panic("quantize_grouped_batch: NULL buffer %zu", i);
        if (reinterpret_cast<uintptr_t>(scales[i]) % 4 != 0) panic("quantize_grouped_batch: scales %zu must be 4-byte aligned", i);
        const Resolved rin = ctx->resolve_ptr(inputs[i]), rout = ctx->resolve_ptr(outputs[i]), rs = resolve(scales[i]), rz = resolve(zero_points[i]);
        if (rin.pageable || rout.pageable || rs.pageable || rz.pageable) panic("piquant_hip_quantize_grouped_batch needs device (or pinned) buffers");
        if (!grouped_aligned16(rin.dev) || !grouped_aligned16(rout.dev)) {   // the single call's guarded kernel, same bytes
            GroupedQuantLaunch q {};
            q.in = rin.dev;
            q.out = rout.dev;
            q.numel = static_cast<int64_t>(numels[i]);
            q.group_size = b.group_size;
            q.scales = static_cast<float*>(rs.dev);
            q.zero_points = static_cast<uint8_t*>(rz.dev);
            q.params_given = b.params_given;
            q.dt_in = dtype_in;
            q.dt_out = dtype_out;
            q.round_mode = b.round_mode;
            q.threshold = b.threshold;
            q.seed = b.seed;
            q.index_base = b.index_base;
            launch_quantize_grouped(q, ctx->stream, ctx->num_cu);
            continue;
        }
        b.in[b.count] = rin.dev;
        b.out[b.count] = rout.dev;
        b.scales[b.count] = static_cast<float*>(rs.dev);
        b.zero_points[b.count] = static_cast<uint8_t*>(rz.dev);
        b.numel[b.count] = static_cast<int64_t>(numels[i]);
        if (++b.count == kGroupedBatchMaxTensors) {
            launch_quantize_grouped_batch(b, ctx->stream);
            b.count = 0;
        }
    }
    launch_quantize_grouped_batch(b, ctx->stream);
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_dequantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                          piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, const float* const* scales,
                                          const uint8_t* const* zero_points, size_t count, piquant_reduce_op_t op) {
    if (!ctx) panic("piquant_hip_dequantize_grouped_batch: context is NULL");
    const dtype_row& dti = dtype_of(dtype_in);
    const dtype_row& dto = dtype_of(dtype_out);
    if (!dti.quant) panic("dequantize: input dtype (%s) must be a quantized type", dti.name);
    if (dto.quant) panic("dequantize: output dtype (%s) must be a dequantized type", dto.name);
    if (op != PIQUANT_REDUCE_OP_SET && op != PIQUANT_REDUCE_OP_ADD) panic("dequantize: invalid reduce op %d", static_cast<int>(op));
    check_group_size(group_size);
    if (count == 0) return;
    if (!inputs || !outputs || !numels || !scales || !zero_points) panic("piquant_hip_dequantize_grouped_batch: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    GroupedDequantBatchLaunch b {};
    b.group_size = static_cast<int64_t>(group_size);
    b.dt_in = dtype_in;
    b.dt_out = dtype_out;
    b.op = op == PIQUANT_REDUCE_OP_ADD ? OP_ADD : OP_SET;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the parameters are written by whatever was enqueued just before
    for (size_t i = 0; i < count; ++i) {
        if (numels[i] == 0) continue;
        if (!inputs[i] || !outputs[i] || !scales[i] || !zero_points[i]) panic("dequantize_grouped_batch: NULL buffer %zu", i);
        if (reinterpret_cast<uintptr_t>(scales[i]) % 4 != 0) panic("dequantize_grouped_batch: scales %zu must be 4-byte aligned", i);
        const Resolved rin = ctx->resolve_ptr(inputs[i]), rout = ctx->resolve_ptr(outputs[i]), rs = resolve(scales[i]), rz = resolve(zero_points[i]);
        if (rin.pageable || rout.pageable || rs.pageable || rz.pageable) panic("piquant_hip_dequantize_grouped_batch needs device (or pinned) buffers");
        if (!grouped_aligned16(rin.dev) || !grouped_aligned16(rout.dev)) {
            GroupedDequantLaunch d {};
            d.in = rin.dev;
            d.out = rout.dev;
            d.numel = static_cast<int64_t>(numels[i]);
            d.group_size = b.group_size;
            d.scales = static_cast<const float*>(rs.dev);
            d.zero_points = static_cast<const uint8_t*>(rz.dev);
            d.dt_in = dtype_in;
            d.dt_out = dtype_out;
            d.op = b.op;
            launch_dequantize_grouped(d, ctx->stream, ctx->num_cu);
            continue;
        }
        b.in[b.count] = rin.dev;
        b.out[b.count] = rout.dev;
        b.scales[b.count] = static_cast<const float*>(rs.dev);
        b.zero_points[b.count] = static_cast<const uint8_t*>(rz.dev);
        b.numel[b.count] = static_cast<int64_t>(numels[i]);
        if (++b.count == kGroupedBatchMaxTensors) {
            launch_dequantize_grouped_batch(b, ctx->stream);
            b.count = 0;
        }
    }
    launch_dequantize_grouped_batch(b, ctx->stream);
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_reduce_quantize_grouped(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, const void* const* inputs,
                                         const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count, void* out,
                                         piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                         piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_reduce_quantize_grouped: context is NULL");
    check_dynamic_types(dtype_acc, dtype_out, mode);
    check_group_size(group_size);
    if (numel == 0) return;
    if (!acc || !out || !scales || !zero_points) panic("reduce_quantize_grouped: NULL buffer");
    if (count != 0 && (!inputs || !input_scales || !input_zero_points)) panic("piquant_hip_reduce_quantize_grouped: NULL argument");
    if (reinterpret_cast<uintptr_t>(scales) % 4 != 0) panic("reduce_quantize_grouped: scales must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved racc = ctx->resolve_ptr(acc), rout = ctx->resolve_ptr(out), rs = resolve(scales), rz = resolve(zero_points);
    if (racc.pageable || rout.pageable || rs.pageable || rz.pageable) panic("piquant_hip_reduce_quantize_grouped needs device (or pinned) buffers");
    // the terms, resolved; every buffer 16-byte aligned takes the fused kernel, anything else the two-step form (same bytes)
    std::vector<const void*> tin(count);
    std::vector<const float*> tsc(count);
    std::vector<const uint8_t*> tzp(count);
    bool aligned = grouped_aligned16(racc.dev) && grouped_aligned16(rout.dev);
    for (size_t i = 0; i < count; ++i) {
        if (!inputs[i] || !input_scales[i] || !input_zero_points[i]) panic("reduce_quantize_grouped: NULL input %zu", i);
        if (reinterpret_cast<uintptr_t>(input_scales[i]) % 4 != 0) panic("reduce_quantize_grouped: input scales %zu must be 4-byte aligned", i);
        const Resolved ri = ctx->resolve_ptr(inputs[i]), rsi = resolve(input_scales[i]), rzi = resolve(input_zero_points[i]);
        if (ri.pageable || rsi.pageable || rzi.pageable) panic("piquant_hip_reduce_quantize_grouped needs device (or pinned) buffers");
        tin[i] = ri.dev;
        tsc[i] = static_cast<const float*>(rsi.dev);
        tzp[i] = static_cast<const uint8_t*>(rzi.dev);
        aligned = aligned && grouped_aligned16(ri.dev);
    }
    QuantLaunch rm {};
    fill_round_mode(ctx, rm, mode);   // the call's one threshold, whichever form runs
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the terms' parameters are written by whatever was enqueued just before
    // terms that are not fused: grouped dequantize ADD into acc, in order
    const size_t fused_from = aligned ? (count > static_cast<size_t>(kGroupedReduceMaxInputs) ? count - kGroupedReduceMaxInputs : 0) : count;
    for (size_t i = 0; i < fused_from; ++i) {
        GroupedDequantLaunch d {};
        d.in = tin[i];
        d.out = racc.dev;
        d.numel = static_cast<int64_t>(numel);
        d.group_size = static_cast<int64_t>(group_size);
        d.scales = tsc[i];
        d.zero_points = tzp[i];
        d.dt_in = dtype_out;
        d.dt_out = dtype_acc;
        d.op = OP_ADD;
        launch_dequantize_grouped(d, ctx->stream, ctx->num_cu);
    }
    if (aligned && count > 0) {
        GroupedReduceLaunch r {};
        r.acc = racc.dev;
        r.out = rout.dev;
        r.numel = static_cast<int64_t>(numel);
        r.group_size = static_cast<int64_t>(group_size);
        r.scales = static_cast<float*>(rs.dev);
        r.zero_points = static_cast<uint8_t*>(rz.dev);
        for (size_t i = fused_from; i < count; ++i) {
            r.in[r.count] = tin[i];
            r.in_scales[r.count] = tsc[i];
            r.in_zero_points[r.count] = tzp[i];
            ++r.count;
        }
        r.dt_acc = dtype_acc;
        r.dt_out = dtype_out;
        r.round_mode = rm.round_mode;
        r.threshold = rm.threshold;
        r.seed = rm.seed;
        r.index_base = rm.index_base;
        launch_reduce_quantize_grouped(r, ctx->stream);
    } else {   // k == 0, or the two-step form: quantize_grouped(acc)
        GroupedQuantLaunch q {};
        q.in = racc.dev;
        q.out = rout.dev;
        q.numel = static_cast<int64_t>(numel);
        q.group_size = static_cast<int64_t>(group_size);
        q.scales = static_cast<float*>(rs.dev);
        q.zero_points = static_cast<uint8_t*>(rz.dev);
        q.params_given = false;
        q.dt_in = dtype_acc;
        q.dt_out = dtype_out;
        q.round_mode = rm.round_mode;
        q.threshold = rm.threshold;
        q.seed = rm.seed;
        q.index_base = rm.index_base;
        launch_quantize_grouped(q, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

// Error feedback (include/piquant_hip.h, piquant_hip_quantize_grouped_ef).  The single call goes through the batch entry with one tensor, which
// launches the single-tensor kernel.
void piquant_hip_quantize_grouped_ef_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* residuals,
                                           void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, float* const* scales,
                                           uint8_t* const* zero_points, size_t count, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped_ef_batch: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (count == 0) return;
    if (!inputs || !residuals || !outputs || !numels || !scales || !zero_points) panic("piquant_hip_quantize_grouped_ef_batch: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    QuantLaunch rm {};
    fill_round_mode(ctx, rm, mode);   // ONE threshold (or per-element seed and base) for the whole batch
    GroupedEfBatchLaunch b {};
    b.group_size = static_cast<int64_t>(group_size);
    b.dt_in = dtype_in;
    b.dt_out = dtype_out;
    b.round_mode = rm.round_mode;
    b.threshold = rm.threshold;
    b.seed = rm.seed;
    b.index_base = rm.index_base;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the residual is written by the previous step's call: always behind it
    for (size_t i = 0; i < count; ++i) {
        if (numels[i] == 0) continue;
        if (!inputs[i] || !residuals[i] || !outputs[i] || !scales[i] || !zero_points[i]) panic("quantize_grouped_ef: NULL buffer %zu", i);
        if (reinterpret_cast<uintptr_t>(scales[i]) % 4 != 0) panic("quantize_grouped_ef: scales %zu must be 4-byte aligned", i);
        const Resolved rin = ctx->resolve_ptr(inputs[i]), rres = ctx->resolve_ptr(residuals[i]), rout = ctx->resolve_ptr(outputs[i]), rs = resolve(scales[i]),
                       rz = resolve(zero_points[i]);
        if (rin.pageable || rres.pageable || rout.pageable || rs.pageable || rz.pageable) panic("piquant_hip_quantize_grouped_ef needs device (or pinned) buffers");
        const int t = b.count;
        b.in[t] = rin.dev;
        b.residual[t] = rres.dev;
        b.out[t] = rout.dev;
        b.scales[t] = static_cast<float*>(rs.dev);
        b.zero_points[t] = static_cast<uint8_t*>(rz.dev);
        b.numel[t] = static_cast<int64_t>(numels[i]);
        if (!grouped_aligned16(rin.dev) || !grouped_aligned16(rres.dev) || !grouped_aligned16(rout.dev)) {   // the guarded kernel, same bytes
            launch_quantize_grouped_ef_guarded(b, t, ctx->stream, ctx->num_cu);
            continue;
        }
        if (++b.count == kGroupedBatchMaxTensors) {
            launch_quantize_grouped_ef_batch(b, ctx->stream);
            b.count = 0;
        }
    }
    launch_quantize_grouped_ef_batch(b, ctx->stream);
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_grouped_ef(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* residual, void* out, piquant_dtype_t dtype_out,
                                     size_t numel, size_t group_size, float* scales, uint8_t* zero_points, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped_ef: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    piquant_hip_quantize_grouped_ef_batch(ctx, &in, dtype_in, &residual, &out, dtype_out, &numel, group_size, &scales, &zero_points, 1, mode);
}

// Error feedback on a re-quantized partial sum (include/piquant_hip.h).  Every buffer 16-byte aligned: the surplus over kGroupedReduceMaxInputs terms
// goes into acc by grouped dequantize ADD launches and the last terms are fused with the residual in ONE launch.  Anything else: the two-step
// composition that defines the call -- every term by grouped dequantize ADD, then quantize_grouped_ef(acc, residual) -- with the call's one threshold.
void piquant_hip_reduce_quantize_grouped_ef(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, void* residual, const void* const* inputs,
                                            const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count, void* out,
                                            piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                            piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_reduce_quantize_grouped_ef: context is NULL");
    check_dynamic_types(dtype_acc, dtype_out, mode);
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    if (!acc || !residual || !out || !scales || !zero_points) panic("reduce_quantize_grouped_ef: NULL buffer");
    if (count != 0 && (!inputs || !input_scales || !input_zero_points)) panic("piquant_hip_reduce_quantize_grouped_ef: NULL argument");
    if (reinterpret_cast<uintptr_t>(scales) % 4 != 0) panic("reduce_quantize_grouped_ef: scales must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved racc = ctx->resolve_ptr(acc), rres = ctx->resolve_ptr(residual), rout = ctx->resolve_ptr(out), rs = resolve(scales), rz = resolve(zero_points);
    if (racc.pageable || rres.pageable || rout.pageable || rs.pageable || rz.pageable)
        panic("piquant_hip_reduce_quantize_grouped_ef needs device (or pinned) buffers");
    std::vector<const void*> tin(count);
    std::vector<const float*> tsc(count);
    std::vector<const uint8_t*> tzp(count);
    bool aligned = grouped_aligned16(racc.dev) && grouped_aligned16(rres.dev) && grouped_aligned16(rout.dev);
    for (size_t i = 0; i < count; ++i) {
        if (!inputs[i] || !input_scales[i] || !input_zero_points[i]) panic("reduce_quantize_grouped_ef: NULL input %zu", i);
        if (reinterpret_cast<uintptr_t>(input_scales[i]) % 4 != 0) panic("reduce_quantize_grouped_ef: input scales %zu must be 4-byte aligned", i);
        const Resolved ri = ctx->resolve_ptr(inputs[i]), rsi = resolve(input_scales[i]), rzi = resolve(input_zero_points[i]);
        if (ri.pageable || rsi.pageable || rzi.pageable) panic("piquant_hip_reduce_quantize_grouped_ef needs device (or pinned) buffers");
        tin[i] = ri.dev;
        tsc[i] = static_cast<const float*>(rsi.dev);
        tzp[i] = static_cast<const uint8_t*>(rzi.dev);
        aligned = aligned && grouped_aligned16(ri.dev);
    }
    QuantLaunch rm {};
    fill_round_mode(ctx, rm, mode);   // the call's one threshold, whichever form runs
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // terms, parameters and residual are written by what was enqueued before: always behind it
    const size_t fused_from = aligned ? (count > static_cast<size_t>(kGroupedReduceMaxInputs) ? count - kGroupedReduceMaxInputs : 0) : count;
    for (size_t i = 0; i < fused_from; ++i) {
        GroupedDequantLaunch d {};
        d.in = tin[i];
        d.out = racc.dev;
        d.numel = static_cast<int64_t>(numel);
        d.group_size = static_cast<int64_t>(group_size);
        d.scales = tsc[i];
        d.zero_points = tzp[i];
        d.dt_in = dtype_out;
        d.dt_out = dtype_acc;
        d.op = OP_ADD;
        launch_dequantize_grouped(d, ctx->stream, ctx->num_cu);
    }
    if (aligned && count > 0) {
        GroupedReduceEfLaunch e {};
        GroupedReduceLaunch& r = e.r;
        e.residual = rres.dev;
        r.acc = racc.dev;
        r.out = rout.dev;
        r.numel = static_cast<int64_t>(numel);
        r.group_size = static_cast<int64_t>(group_size);
        r.scales = static_cast<float*>(rs.dev);
        r.zero_points = static_cast<uint8_t*>(rz.dev);
        for (size_t i = fused_from; i < count; ++i) {
            r.in[r.count] = tin[i];
            r.in_scales[r.count] = tsc[i];
            r.in_zero_points[r.count] = tzp[i];
            ++r.count;
        }
        r.dt_acc = dtype_acc;
        r.dt_out = dtype_out;
        r.round_mode = rm.round_mode;
        r.threshold = rm.threshold;
        r.seed = rm.seed;
        r.index_base = rm.index_base;
        launch_reduce_quantize_grouped_ef(e, ctx->stream);
    } else {   // k == 0, or the two-step form: quantize_grouped_ef(acc, residual), streaming or guarded by its own alignment rule
        GroupedEfBatchLaunch b {};
        b.in[0] = racc.dev;
        b.residual[0] = rres.dev;
        b.out[0] = rout.dev;
        b.scales[0] = static_cast<float*>(rs.dev);
        b.zero_points[0] = static_cast<uint8_t*>(rz.dev);
        b.numel[0] = static_cast<int64_t>(numel);
        b.group_size = static_cast<int64_t>(group_size);
        b.dt_in = dtype_acc;
        b.dt_out = dtype_out;
        b.round_mode = rm.round_mode;
        b.threshold = rm.threshold;
        b.seed = rm.seed;
        b.index_base = rm.index_base;
        if (grouped_aligned16(racc.dev) && grouped_aligned16(rres.dev) && grouped_aligned16(rout.dev)) {
            b.count = 1;
            launch_quantize_grouped_ef_batch(b, ctx->stream);
        } else {
            launch_quantize_grouped_ef_guarded(b, 0, ctx->stream, ctx->num_cu);
        }
    }
    if (ctx->blocking) wait_stream(ctx);
}

// Error feedback with the residual's type named (include/piquant_hip.h, piquant_hip_quantize_grouped_ef_mixed): the residual's type equal to the
// tensor's forwards to the calls above; a bfloat16 tensor with a float32 residual runs the kernels of kernels_grouped_ef_f32r.hip.
static bool grouped_ef_f32_residual(const char* what, piquant_dtype_t dtype_in, piquant_dtype_t dtype_residual) {
    if (dtype_residual == dtype_in) return false;
    if (dtype_in == PIQUANT_DTYPE_BF16 && dtype_residual == PIQUANT_DTYPE_F32) return true;
    panic("%s: a %s residual for a %s tensor (the tensor's type, or float32 for a bfloat16 tensor, is needed)", what, dtype_of(dtype_residual).name,
          dtype_of(dtype_in).name);
}

// the streaming kernels' rule: 16-byte residual and output, 8-byte tensor (its lane-row is four bfloat16 elements)
static inline bool grouped_f32r_aligned(const void* in, const void* residual, const void* out) {
    return (reinterpret_cast<uintptr_t>(in) & 7u) == 0 && grouped_aligned16(residual) && grouped_aligned16(out);
}

void piquant_hip_quantize_grouped_ef_mixed_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* residuals,
                                                 piquant_dtype_t dtype_residual, void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                 size_t group_size, float* const* scales, uint8_t* const* zero_points, size_t count,
                                                 piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped_ef_mixed_batch: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    if (!grouped_ef_f32_residual("piquant_hip_quantize_grouped_ef_mixed_batch", dtype_in, dtype_residual)) {
        piquant_hip_quantize_grouped_ef_batch(ctx, inputs, dtype_in, residuals, outputs, dtype_out, numels, group_size, scales, zero_points, count, mode);
        return;
    }
    check_group_size(group_size);
    if (count == 0) return;
    if (!inputs || !residuals || !outputs || !numels || !scales || !zero_points) panic("piquant_hip_quantize_grouped_ef_mixed_batch: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    QuantLaunch rm {};
    fill_round_mode(ctx, rm, mode);   // ONE threshold (or per-element seed and base) for the whole batch
    GroupedEfBatchLaunch b {};
    b.group_size = static_cast<int64_t>(group_size);
    b.dt_in = dtype_in;
    b.dt_out = dtype_out;
    b.round_mode = rm.round_mode;
    b.threshold = rm.threshold;
    b.seed = rm.seed;
    b.index_base = rm.index_base;
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // the residual is written by the previous step's call: always behind it
    for (size_t i = 0; i < count; ++i) {
        if (numels[i] == 0) continue;
        if (!inputs[i] || !residuals[i] || !outputs[i] || !scales[i] || !zero_points[i]) panic("quantize_grouped_ef_mixed: NULL buffer %zu", i);
        if (reinterpret_cast<uintptr_t>(scales[i]) % 4 != 0) panic("quantize_grouped_ef_mixed: scales %zu must be 4-byte aligned", i);
        const Resolved rin = ctx->resolve_ptr(inputs[i]), rres = ctx->resolve_ptr(residuals[i]), rout = ctx->resolve_ptr(outputs[i]), rs = resolve(scales[i]),
                       rz = resolve(zero_points[i]);
        if (rin.pageable || rres.pageable || rout.pageable || rs.pageable || rz.pageable)
            panic("piquant_hip_quantize_grouped_ef_mixed needs device (or pinned) buffers");
        if (reinterpret_cast<uintptr_t>(rin.dev) % 2 != 0 || reinterpret_cast<uintptr_t>(rres.dev) % 4 != 0)
            panic("quantize_grouped_ef_mixed: tensor %zu or its residual is not aligned to its element size", i);
        const int t = b.count;
        b.in[t] = rin.dev;
        b.residual[t] = rres.dev;
        b.out[t] = rout.dev;
        b.scales[t] = static_cast<float*>(rs.dev);
        b.zero_points[t] = static_cast<uint8_t*>(rz.dev);
        b.numel[t] = static_cast<int64_t>(numels[i]);
        if (!grouped_f32r_aligned(rin.dev, rres.dev, rout.dev)) {   // the guarded kernel, same bytes
            launch_quantize_grouped_ef_f32r_guarded(b, t, ctx->stream, ctx->num_cu);
            continue;
        }
        if (++b.count == kGroupedBatchMaxTensors) {
            launch_quantize_grouped_ef_f32r_batch(b, ctx->stream);
            b.count = 0;
        }
    }
    launch_quantize_grouped_ef_f32r_batch(b, ctx->stream);
    if (ctx->blocking) wait_stream(ctx);
}

void piquant_hip_quantize_grouped_ef_mixed(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* residual, piquant_dtype_t dtype_residual,
                                           void* out, piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                           piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_quantize_grouped_ef_mixed: context is NULL");
    check_dynamic_types(dtype_in, dtype_out, mode);
    if (!grouped_ef_f32_residual("piquant_hip_quantize_grouped_ef_mixed", dtype_in, dtype_residual)) {
        piquant_hip_quantize_grouped_ef(ctx, in, dtype_in, residual, out, dtype_out, numel, group_size, scales, zero_points, mode);
        return;
    }
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    piquant_hip_quantize_grouped_ef_mixed_batch(ctx, &in, dtype_in, &residual, dtype_residual, &out, dtype_out, &numel, group_size, &scales, &zero_points, 1,
                                                mode);
}

// A bfloat16 accumulator with a float32 residual runs as the composition that defines the call: every term by grouped dequantize ADD into acc, in
// order, then the mixed single call on (acc, residual) with the call's one threshold (a fused mixed reduce kernel: DESIGN.md 10).
void piquant_hip_reduce_quantize_grouped_ef_mixed(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, void* residual,
                                                  piquant_dtype_t dtype_residual, const void* const* inputs, const float* const* input_scales,
                                                  const uint8_t* const* input_zero_points, size_t count, void* out, piquant_dtype_t dtype_out, size_t numel,
                                                  size_t group_size, float* scales, uint8_t* zero_points, piquant_round_mode_t mode) {
    if (!ctx) panic("piquant_hip_reduce_quantize_grouped_ef_mixed: context is NULL");
    check_dynamic_types(dtype_acc, dtype_out, mode);
    if (!grouped_ef_f32_residual("piquant_hip_reduce_quantize_grouped_ef_mixed", dtype_acc, dtype_residual)) {
        piquant_hip_reduce_quantize_grouped_ef(ctx, acc, dtype_acc, residual, inputs, input_scales, input_zero_points, count, out, dtype_out, numel, group_size,
                                               scales, zero_points, mode);
        return;
    }
    check_group_size(group_size);
    if (numel == 0) return;   // before a stochastic threshold would be drawn
    if (!acc || !residual || !out || !scales || !zero_points) panic("reduce_quantize_grouped_ef_mixed: NULL buffer");
    if (count != 0 && (!inputs || !input_scales || !input_zero_points)) panic("piquant_hip_reduce_quantize_grouped_ef_mixed: NULL argument");
    if (reinterpret_cast<uintptr_t>(scales) % 4 != 0) panic("reduce_quantize_grouped_ef_mixed: scales must be 4-byte aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const Resolved racc = ctx->resolve_ptr(acc), rres = ctx->resolve_ptr(residual), rout = ctx->resolve_ptr(out), rs = resolve(scales), rz = resolve(zero_points);
    if (racc.pageable || rres.pageable || rout.pageable || rs.pageable || rz.pageable)
        panic("piquant_hip_reduce_quantize_grouped_ef_mixed needs device (or pinned) buffers");
    if (reinterpret_cast<uintptr_t>(racc.dev) % 2 != 0 || reinterpret_cast<uintptr_t>(rres.dev) % 4 != 0)
        panic("reduce_quantize_grouped_ef_mixed: acc or the residual is not aligned to its element size");
    std::vector<GroupedDequantLaunch> adds(count);
    for (size_t i = 0; i < count; ++i) {
        if (!inputs[i] || !input_scales[i] || !input_zero_points[i]) panic("reduce_quantize_grouped_ef_mixed: NULL input %zu", i);
        if (reinterpret_cast<uintptr_t>(input_scales[i]) % 4 != 0) panic("reduce_quantize_grouped_ef_mixed: input scales %zu must be 4-byte aligned", i);
        const Resolved ri = ctx->resolve_ptr(inputs[i]), rsi = resolve(input_scales[i]), rzi = resolve(input_zero_points[i]);
        if (ri.pageable || rsi.pageable || rzi.pageable) panic("piquant_hip_reduce_quantize_grouped_ef_mixed needs device (or pinned) buffers");
        GroupedDequantLaunch& d = adds[i];
        d.in = ri.dev;
        d.out = racc.dev;
        d.numel = static_cast<int64_t>(numel);
        d.group_size = static_cast<int64_t>(group_size);
        d.scales = static_cast<const float*>(rsi.dev);
        d.zero_points = static_cast<const uint8_t*>(rzi.dev);
        d.dt_in = dtype_out;
        d.dt_out = dtype_acc;
        d.op = OP_ADD;
    }
    QuantLaunch rm {};
    fill_round_mode(ctx, rm, mode);   // the call's one threshold
    StopEventScope completion(ctx);
    IndependentCallScope independent(ctx, true);   // terms, parameters and residual are written by what was enqueued before: always behind it
    for (size_t i = 0; i < count; ++i) launch_dequantize_grouped(adds[i], ctx->stream, ctx->num_cu);
    GroupedEfBatchLaunch b {};
    b.in[0] = racc.dev;
    b.residual[0] = rres.dev;
    b.out[0] = rout.dev;
    b.scales[0] = static_cast<float*>(rs.dev);
    b.zero_points[0] = static_cast<uint8_t*>(rz.dev);
    b.numel[0] = static_cast<int64_t>(numel);
    b.group_size = static_cast<int64_t>(group_size);
    b.dt_in = dtype_acc;
    b.dt_out = dtype_out;
    b.round_mode = rm.round_mode;
    b.threshold = rm.threshold;
    b.seed = rm.seed;
    b.index_base = rm.index_base;
    if (grouped_f32r_aligned(racc.dev, rres.dev, rout.dev)) {
        b.count = 1;
        launch_quantize_grouped_ef_f32r_batch(b, ctx->stream);
    } else {
        launch_quantize_grouped_ef_f32r_guarded(b, 0, ctx->stream, ctx->num_cu);
    }
    if (ctx->blocking) wait_stream(ctx);
}

}  // extern "C"
