/* piquant_hip.h -- additive, optional entry points of the MI355X-native libpiquant.so.
 *
 * Nothing here exists in the reference; a caller that only knows piquant.h never needs it.  These
 * functions expose what a GPU data path needs and the reference's synchronous host-only API cannot
 * express: the HIP stream to enqueue on, asynchronous completion, a reproducible stochastic threshold,
 * and the two halves of compute_quant_params (device-side min/max scan, host-side epilogue) between which
 * a multi-GPU caller performs its one collective (an 8-byte MIN all-reduce over RCCL/xGMI).
 */
#ifndef PIQUANT_HIP_H
#define PIQUANT_HIP_H

#include "piquant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HIP stream (a hipStream_t passed as void*) that the context enqueues its kernels on from now on.  As in every
 * HIP API, NULL names the legacy default stream -- which is what PyTorch-ROCm's default stream is, so PyTorch
 * callers simply pass torch.cuda.current_stream().cuda_stream and the work is ordered with the tensors' producers
 * and consumers.  A new context enqueues on a private non-blocking stream; piquant_hip_reset_stream returns to it. */
PIQUANT_EXPORT void piquant_hip_set_stream(piquant_context_t* ctx, void* hip_stream);
PIQUANT_EXPORT void piquant_hip_reset_stream(piquant_context_t* ctx);

/* blocking != 0 (default): every piquant.h call returns after its work has completed on the GPU -- the
 * reference's semantics (its calls join the thread pool before returning, src/piquant.cpp:210,237).
 * blocking == 0: piquant_quantize / piquant_dequantize on DEVICE pointers only enqueue; completion follows
 * stream order.  Host-pointer calls and compute_quant_params always complete before returning. */
PIQUANT_EXPORT void piquant_hip_set_blocking(piquant_context_t* ctx, int blocking);

/* How a blocking call waits for the GPU: 0 = hipStreamSynchronize; 1 = the command processor writes the call's sequence number
 * into a pinned host word behind the kernel (hipStreamWriteValue32) and the host spins on it; 2 = the same word written by a
 * one-thread kernel; 3 = the work kernel is launched with a stop event (its dispatch packet's own completion signal) that the host polls
 * with hipEventQuery -- nothing is enqueued behind it (piquant_quantize / piquant_dequantize on device buffers; other calls wait as 2).
 * All four return after the work has completed; they differ in latency only.  The
 * environment variable PIQUANT_HIP_BLOCKING_WAIT = sync | write32 | kernel | event sets it at context creation. */
PIQUANT_EXPORT void piquant_hip_set_blocking_wait(piquant_context_t* ctx, int mode);

/* What serves calls whose buffers are pageable HOST memory (the reference's own calling convention, src/capi.cpp:28-54).
 *   PIQUANT_HIP_HOST_PATH_AUTO (2, default): host tensors stay on the host -- the call is handed to libpiquant_cpu.so when that library loads
 *       and the host has AVX-512 (the same arithmetic on the host cores, at host-memory bandwidth: what the reference does with such a
 *       call); otherwise, and for everything the companion does not implement (below), PIQUANT_HIP_HOST_PATH_STAGE.  Which of the two a
 *       context resolved to: piquant_hip_host_path_in_effect.
 *   PIQUANT_HIP_HOST_PATH_STAGE (0): chunks of 2^24 elements cross PCIe into device scratch, the HIP kernels process them, the
 *       results cross back -- every element is computed by the GPU, at ~40 GiB/s of fp32 input (PCIe bound).
 *   PIQUANT_HIP_HOST_PATH_CPU (1): always libpiquant_cpu.so (include/piquant_cpu.h; loaded from the directory of this library on first
 *       use, ABORT if it is missing; its scalar form on hosts without AVX-512).
 * Only calls whose input AND output are pageable host memory go to the companion; device, pinned and managed pointers always run the HIP
 * kernels, and so does the per-element stochastic extension, which the companion does not implement (staged).  Reference-layout mode on host
 * buffers is the companion's too since round 5 (piquant_cpu_*_reference_layout: the head of a partition placed by the CALLER's output pointer).
 * The environment variable PIQUANT_HIP_HOST_PATH = auto | stage | cpu sets it at context creation. */
#define PIQUANT_HIP_HOST_PATH_STAGE 0
#define PIQUANT_HIP_HOST_PATH_CPU 1
#define PIQUANT_HIP_HOST_PATH_AUTO 2
PIQUANT_EXPORT void piquant_hip_set_host_path(piquant_context_t* ctx, int path);
/* STAGE or CPU: what pageable host buffers of this context get right now (AUTO resolved) */
PIQUANT_EXPORT int piquant_hip_host_path_in_effect(piquant_context_t* ctx);

/* Pointer classification.  By default every buffer is classified with hipPointerGetAttributes (device / pinned: used in
 * place; pageable host: the host path above -- companion library or staging over PCIe).  A binding that already knows its buffers are device memory (PyTorch device
 * tensors) sets assume != 0 to skip the two runtime queries per call -- they are a visible share of the ~10 us a small
 * call costs.  With assume set, passing a pageable host pointer is undefined behaviour. */
PIQUANT_EXPORT void piquant_hip_assume_device_pointers(piquant_context_t* ctx, int assume);

/* Stochastic rounding control.  The reference draws ONE threshold in [0,1) per call from an unseeded
 * thread-local mt19937_64 (src/piquant.cpp:194-201) and compares every element's fractional part with it
 * (src/kernels/quantize.inl:8-19).  Default here: the same, drawn per call from a context-owned
 * mt19937_64.
 *   piquant_hip_set_stochastic_threshold(ctx, t): 0 <= t < 1 pins the per-call threshold (reproducible,
 *       bit-comparable with the reference kernels driven with the same threshold); t < 0 restores drawing.
 *   piquant_hip_set_stochastic_seed(ctx, seed): reseeds the context's generator.
 *   piquant_hip_set_stochastic_per_element(ctx, on, seed, index_base): opt-in extension -- an independent
 *       threshold per element from a counter hash of (seed, index_base + element index); shard-invariant
 *       when each shard passes its global element offset as index_base.
 * Under hipGraph capture the threshold (or seed / index_base) drawn at capture time is part of the recorded launch and is
 * replayed unchanged. */
PIQUANT_EXPORT void piquant_hip_set_stochastic_threshold(piquant_context_t* ctx, float threshold);
PIQUANT_EXPORT void piquant_hip_set_stochastic_seed(piquant_context_t* ctx, uint64_t seed);
PIQUANT_EXPORT void piquant_hip_set_stochastic_per_element(piquant_context_t* ctx, int enabled, uint64_t seed,
                                                           uint64_t index_base);

/* Reference layout (ON by default for piquant_quantize and piquant_dequantize since round 6).  The reference's output depends on WHERE an
 * element sits: a reference context of T pool threads splits a call into T partitions (src/piquant.cpp:145-157), every partition runs one
 * kernel call, and that call's scalar head (fp32 -> uint8 only: elements before the partition's output pointer is 16-byte aligned,
 * kernels_specialized.inl:52) and scalar tail (what is left of the last SIMD block: numel mod 64 / 16 elements when quantizing, mod 64 / 128 /
 * 256 when dequantizing to bf16) use std::round and a second bf16 rounding, which differ from the SIMD body on a few inputs (|x/scale| =
 * 0.49999997, odd |x/scale| >= 2^23, bf16 ADD ties -- 22 of 10^6 ordinary elements with 3 threads), and the 1-3 element
 * tail of uint2 -> f32 ADD stores instead of adding (dequantize.inl:72-86).  The two plain calls reproduce exactly that: every output byte
 * equals what the reference's AVX-512 build writes from a context created with the same num_threads (T = the num_threads of
 * piquant_context_create, or whatever piquant_hip_set_reference_threads says), for device, pinned and host buffers alike.  It costs nothing:
 * a wave tile that a partition's head or tail reaches into handles those positions itself, in registers, before its one store.
 *   piquant_hip_set_reference_layout(ctx, 0), or PIQUANT_HIP_REFERENCE_LAYOUT=0 in the environment at context creation, turns it off: the
 *       SIMD-body formula at every element, independent of pointer alignment, length and thread count.
 * Position-independent BY CONSTRUCTION, whatever the mode: piquant_hip_quantize_uniform / piquant_hip_dequantize_uniform (the plain calls in
 * the SIMD-body form -- what a shard of a larger tensor must be computed with, piquant.distributed), the device-parameter twins (*_dp), the
 * one-launch calls (piquant_hip_quantize_dynamic, its batch and reduce variants) and piquant_hip_dequantize_sum / _dp_batch. */
PIQUANT_EXPORT void piquant_hip_set_reference_layout(piquant_context_t* ctx, int enabled);
PIQUANT_EXPORT void piquant_hip_set_reference_threads(piquant_context_t* ctx, int threads);
PIQUANT_EXPORT void piquant_hip_quantize_uniform(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out,
                                                 size_t numel, float scale, int64_t zero_point, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_dequantize_uniform(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out,
                                                   size_t numel, float scale, int64_t zero_point, piquant_reduce_op_t op);

/* Fused quantize -> dequantize: out[i] (op)= dequantize(quantize(in[i])) without materialising the quantized tensor;
 * dtype_in_out (F32 or BF16) is the type of BOTH buffers, quant_dtype (UINT2/4/8) the type passed through; `out` may
 * alias `in`.  This is the reference's C++-only context::quantize_dequantize_fused (include/piquant.hpp:276-285,
 * src/piquant.cpp:342-369, kernels src/kernels/kernels.inl:30-52), which its C ABI does not export.  Device pointers
 * only.  Every element takes the reference's generic scalar steps (there is no SIMD fast path for this command). */
PIQUANT_EXPORT void piquant_hip_quantize_dequantize(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in_out, void* out,
                                                    piquant_dtype_t quant_dtype, size_t numel, float scale, int64_t zero_point,
                                                    piquant_round_mode_t mode, piquant_reduce_op_t op);

/* First half of compute_quant_params: scan n elements of x (dtype F32 or BF16, device or host pointer)
 * and fold {min, -max} into two order-preserving int32 keys in DEVICE memory with atomic MIN, enqueued on
 * the context's stream (asynchronous).  init != 0 first resets both keys to the identity (+FLT_MAX), so
 * several scans with init == 0 accumulate into one result.  Because both keys reduce with MIN, a
 * multi-GPU caller needs exactly one MIN all-reduce of 2 x int32 (torch.distributed / RCCL) between this
 * call and the epilogue.  Restates reference src/kernels/kernels_specialized.inl:1418-1607 + the block fold
 * of src/piquant.cpp:230-244. */
PIQUANT_EXPORT void piquant_hip_minmax_keys(piquant_context_t* ctx, const void* x, piquant_dtype_t dtype, size_t n,
                                            int32_t* device_keys, int init);

/* Device-resident quantization parameters ("dynamic" path): (scale, zero_point) are derived on the GPU and consumed by
 * the next kernels without visiting the host, so compute-params -> quantize -> (send) -> dequantize is one asynchronous
 * stream of launches (capturable in a hipGraph).  The record is 16 bytes of device memory, e.g. the header of a wire
 * buffer.  piquant_hip_compute_quant_params_device = min/max scan + a one-wave kernel running the reference's
 * double-precision epilogue (src/piquant.cpp:245-258; results are bit-identical to piquant_compute_quant_params_*,
 * except that the device cannot abort: where the synchronous call would -- nothing scanned, i.e. an empty tensor or one made
 * of NaNs only, max < min -- the record is the degenerate one, scale 1.0 and zero point qmax >> 1).  The *_dp calls are piquant_quantize /
 * piquant_dequantize with scale and zero_point read from the record.  Device (or pinned) buffers only. */
typedef struct piquant_hip_params_t {
    float scale;
    float inv_scale;    /* 1.0f / scale */
    int64_t zero_point;
} piquant_hip_params_t;

PIQUANT_EXPORT void piquant_hip_compute_quant_params_device(piquant_context_t* ctx, const void* x, piquant_dtype_t dtype, size_t n,
                                                            piquant_dtype_t target_quant_dtype, piquant_hip_params_t* device_params);
PIQUANT_EXPORT void piquant_hip_quantize_dp(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out,
                                            piquant_dtype_t dtype_out, size_t numel, const piquant_hip_params_t* device_params,
                                            piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_dequantize_dp(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out,
                                              piquant_dtype_t dtype_out, size_t numel, const piquant_hip_params_t* device_params,
                                              piquant_reduce_op_t op);

/* compute_quant_params + quantize as ONE call: out = quantize(in) with (scale, zero_point) computed from `in` itself (the
 * reference's Python flow piquant.torch.compute_quant_params -> quantize, python/src/piquant/torch.py:54-100), the
 * parameters left in *device_params (16-byte record in device memory) for the dequantizing side.  Stream-ordered, no host
 * round trip, hipGraph-capturable.  When the tensor fits on the chip (<= ~113 MB of fp32 / bf16 input on a 256-CU MI355X,
 * 16-byte aligned buffers) this is a single kernel launch that reads the tensor ONCE: every CU keeps its share in vector
 * registers and LDS between the min/max pass and the quantization pass (5 B/elem of HBM traffic for fp32 -> uint8 instead
 * of 9).  Up to ~268 MB the same launch keeps 113 MB on chip and streams the remainder twice.  Larger or misaligned tensors take a scan (its last block writes the parameters) + quantize (two launches); the output bytes and the
 * record are identical either way.  piquant_hip_set_fusion(ctx, 0), or PIQUANT_HIP_FUSION=0 in the environment when the
 * context is created, forces the two-launch form.  The one-launch kernel synchronises its blocks with a grid barrier (one
 * block per CU) whose waits are bounded (piquant_hip_set_barrier_timeout_us below): it cannot deadlock or abort whatever else
 * runs on the GPU; the library additionally orders such launches from different streams of one process behind one another. */
PIQUANT_EXPORT void piquant_hip_quantize_dynamic(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out,
                                                 piquant_dtype_t dtype_out, size_t numel, piquant_hip_params_t* device_params,
                                                 piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_set_fusion(piquant_context_t* ctx, int enabled);

/* Group-wise quantization: one (scale, zero_point) per run of group_size contiguous elements instead of one per tensor, so that an
 * outlier stretches the range of its own group only.  group_size is a power of two in [32, 4096] (128 is the usual choice); the tensor
 * is cut into ngroups = ceil(numel / group_size) groups, the last one possibly partial.  Parameters live in two device arrays:
 * float scales[ngroups] and uint8_t zero_points[ngroups] (a computed zero point lies in [0, 2^bits - 1]: 5 bytes per group).
 *   piquant_hip_quantize_grouped, params_given == 0: group g's (scales[g], zero_points[g]) are written, bit-identical to what
 *       piquant_hip_compute_quant_params_device writes for that slice alone (NaNs ignored; a group of nothing but NaNs gets the
 *       degenerate (1.0, qmax >> 1)), and group g's bytes are piquant_hip_quantize_uniform of the slice with them.  ONE launch that reads
 *       the input once (no scan, no atomics, no grid barrier).
 *   params_given != 0: scales / zero_points are read instead ("quantize with these per-group parameters").
 *   piquant_hip_dequantize_grouped: group g of `out` (op)= piquant_hip_dequantize_uniform of group g of `in` with its parameters.
 * The position-independent form everywhere (the reference has no grouped call whose partition heads and tails could be mimicked);
 * because group_size >= 32 is a power of two every group starts on a whole packed byte, so the output is the per-group outputs laid end
 * to end.  Stochastic rounding draws ONE threshold per call (piquant_hip_set_stochastic_threshold pins it); in per-element mode the element
 * index is the global index in the tensor.  Device (or pinned) buffers only; stream-ordered on the context's stream, no host
 * synchronisation, no allocation (hipGraph-capturable).  numel == 0 is a no-op. */
PIQUANT_EXPORT void piquant_hip_quantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out,
                                                 size_t numel, size_t group_size, float* scales, uint8_t* zero_points, int params_given,
                                                 piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_dequantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out,
                                                   size_t numel, size_t group_size, const float* scales, const uint8_t* zero_points,
                                                   piquant_reduce_op_t op);
/* Batches of the group-wise calls: tensor i has its own input, output, scales, zero_points and numels[i]; all share the dtype pair, group_size,
 * params_given / op and the round mode.  Tensor i's results are those of the single call on it; a stochastic batch draws ONE threshold (in
 * per-element mode every tensor indexes its own elements from 0).  Up to 16 tensors per launch (more: one launch per 16); empty tensors are
 * skipped, and a tensor whose input or output is not 16-byte aligned goes through the single call.
 * piquant_hip_reduce_quantize_grouped: (out, scales, zero_points) = quantize_grouped(acc + dequantize_grouped(inputs[0]) + ... +
 *       dequantize_grouped(inputs[count - 1])), term i with its own per-group parameters input_scales[i] / input_zero_points[i] (the same
 *       group_size; every term has numel elements of type dtype_out).  The terms are added in order and the running sum is rounded to dtype_acc
 *       after each one: bit for bit piquant_hip_dequantize_grouped(inputs[i], ..., PIQUANT_REDUCE_OP_ADD) into acc for i = 0 .. count - 1 followed
 *       by piquant_hip_quantize_grouped(acc) with computed parameters -- in ONE launch that keeps the sum on chip (no scan, no atomics, no grid
 *       barrier).  More than 16 terms: the surplus is first added into acc by grouped dequantize ADD launches and the last 16 are fused; buffers
 *       that are not 16-byte aligned take that two-step form for every term.  count == 0 is piquant_hip_quantize_grouped(acc).  The contents of
 *       acc afterwards are unspecified.  The owner's step of a grouped mesh all-reduce (count = world - 1) and every hop of a grouped ring (count = 1).
 * Device (or pinned) buffers only; stream-ordered on the context's stream, no host synchronisation, no allocation (hipGraph-capturable). */
PIQUANT_EXPORT void piquant_hip_quantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                                       piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, float* const* scales,
                                                       uint8_t* const* zero_points, size_t count, int params_given, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_dequantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in, void* const* outputs,
                                                         piquant_dtype_t dtype_out, const size_t* numels, size_t group_size, const float* const* scales,
                                                         const uint8_t* const* zero_points, size_t count, piquant_reduce_op_t op);
PIQUANT_EXPORT void piquant_hip_reduce_quantize_grouped(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, const void* const* inputs,
                                                        const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count, void* out,
                                                        piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                                        piquant_round_mode_t mode);
/* Grouped dequantize-sum: out (op)= dequantize_grouped(inputs[0]) + ... + dequantize_grouped(inputs[count - 1]) in ONE pass over out -- the
 * group-wise piquant_hip_dequantize_sum, and piquant_hip_reduce_quantize_grouped's sum stored instead of re-quantized: the owner's step of a grouped
 * reduce-scatter.  Term i is a packed tensor of numel elements of dtype_in with its own per-group parameters input_scales[i] /
 * input_zero_points[i] (one group_size for all).  The call writes to out exactly the bytes that this composition of public calls writes:
 *   ADD: piquant_hip_dequantize_grouped(inputs[i], ..., out, ..., PIQUANT_REDUCE_OP_ADD) for i = 0 .. count - 1 in order;
 *   SET: that call with PIQUANT_REDUCE_OP_SET for i = 0, then with PIQUANT_REDUCE_OP_ADD for i = 1 .. count - 1.
 * The running sum is rounded to dtype_out after every term: float32 with a separately rounded addition per term; bfloat16 with each term's
 * float32 sum rounded to bfloat16 before the next term is added (SET: the first term rounded once, then the second added).  Every dequantized
 * value is formed in the pair's own dequantize form.  All six dtype pairs, all eight group sizes.  SET never reads out.  NaN payloads are not
 * specified.  count >= 1 is required: count == 0 aborts like a NULL argument.  numel == 0 is a no-op.
 * out and every term's packed bytes 16-byte aligned: ONE launch for up to 16 terms (no scan, no atomics, no grid barrier; the sum stays in
 * registers: with seven uint8 terms into float32, 15 bytes of memory traffic per element against the composition's 63); more than 16 terms run as
 * successive launches of up to 16 in order, the first with the call's op and the others ADD (the same bytes).  With anything misaligned the
 * composition itself runs through the guarded grouped dequantize, count launches.  An out that is not aligned to its element aborts.
 * Nothing at or past the tensor's end is read or written in any buffer; out must not overlap a term.  Device (or pinned) buffers only;
 * stream-ordered on the context's stream, always behind the previous call whatever piquant_hip_set_independent_calls says; no host
 * synchronisation, no allocation on the device (hipGraph-capturable). */
PIQUANT_EXPORT void piquant_hip_dequantize_sum_grouped(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                       const float* const* input_scales, const uint8_t* const* input_zero_points, size_t count,
                                                       void* out, piquant_dtype_t dtype_out, size_t numel, size_t group_size, piquant_reduce_op_t op);

/* piquant_hip_reduce_quantize_grouped with error feedback (piquant_hip_quantize_grouped_ef below) on the re-quantization: the owner's step of a
 * grouped mesh all-reduce and every hop of a grouped ring, compensated.  T is dtype_acc (float32 or bfloat16); `residual` has type T and numel
 * elements and is read AND written.  The call writes exactly the bytes that this composition of two public calls writes to out, scales,
 * zero_points and residual:
 *   1. for i = 0 .. count - 1 in order: piquant_hip_dequantize_grouped(inputs[i], ..., input_scales[i], input_zero_points[i],
 *      PIQUANT_REDUCE_OP_ADD) into acc -- the running sum is rounded to T after each term;
 *   2. piquant_hip_quantize_grouped_ef(acc, residual, out, ..., scales, zero_points, mode): y = rn_T(acc + residual), quantize_grouped(y) with
 *      computed parameters, residual <- rn_T(y - d) with d the value a grouped dequantize SET stores (bfloat16: rounded first; the subtraction is
 *      never contracted).
 * The residual is added AFTER the terms.  Every buffer 16-byte aligned: ONE launch for up to 16 terms (no scan, no atomics, no grid barrier; the
 * sum never leaves the registers); with more than 16 the surplus is first added into acc by grouped dequantize ADD launches and the last 16 are
 * fused.  If acc, residual, out or a term is not 16-byte aligned the call runs as the composition above (same bytes).  count == 0 is
 * piquant_hip_quantize_grouped_ef(acc, residual).  The contents of acc afterwards are unspecified; nothing at or past the tensor's end is
 * touched in any buffer; acc, residual, out and the terms must not overlap.  Stochastic rounding draws ONE threshold per call; per-element mode
 * indexes the global element.  Device (or pinned) buffers only; stream-ordered on the context's stream, always behind the previous call whatever
 * piquant_hip_set_independent_calls says; no host synchronisation, no allocation (hipGraph-capturable).  numel == 0 is a no-op. */
PIQUANT_EXPORT void piquant_hip_reduce_quantize_grouped_ef(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, void* residual,
                                                           const void* const* inputs, const float* const* input_scales,
                                                           const uint8_t* const* input_zero_points, size_t count, void* out, piquant_dtype_t dtype_out,
                                                           size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                                           piquant_round_mode_t mode);

/* Error feedback for the group-wise wire: a lossy gradient / pseudo-gradient all-reduce keeps the rounding error of every step and adds it to the
 * next step's input instead of throwing it away.  `residual` has the input's type (dtype_in: float32 or bfloat16) and numel elements; it is read
 * AND written.  With T that type, for every element i < numel:
 *   1. y[i] = x[i] + residual[i], rounded to nearest in T (bfloat16: both widened to float32, added, rounded to nearest even);
 *   2. (out, scales, zero_points) = piquant_hip_quantize_grouped(y) with computed parameters (params_given == 0), bit for bit: every group size,
 *      every dtype pair, nearest and stochastic (ONE threshold per call; per-element mode indexes the global element), the NaN rule and the
 *      degenerate groups included;
 *   3. d[i] = element i of piquant_hip_dequantize_grouped(out, scales, zero_points, dtype T, PIQUANT_REDUCE_OP_SET), bit for bit (for
 *      bfloat16 the value that call stores: rounded to bfloat16 before step 4);
 *   4. residual[i] = y[i] - d[i], rounded to nearest in T (a subtraction of its own, never contracted with step 3 into an fma).
 * The bytes of add -> quantize_grouped -> dequantize_grouped -> subtract (four launches, 34 bytes of memory traffic per float32 element with a
 * uint8 wire) in ONE launch that moves 13: the sum never leaves the registers (no scan, no atomics, no grid barrier).  `in` is not written;
 * nothing at or past the tensor's end is touched in any buffer.  A NaN in y stays a NaN in the residual (its payload and sign are not
 * specified).  Two properties of the parameter epilogue carry over: a constant group gets the degenerate (1.0, qmax >> 1), and a group whose
 * range lies far from zero has its zero point clamped, so most of its mass goes to the residual -- error feedback conserves that mass, it does
 * not make such a group representable.  `in`, `residual` and `out` must not overlap.
 * piquant_hip_quantize_grouped_ef_batch: tensor i has its own input, residual, output, scales, zero_points and numels[i]; the rules of
 * piquant_hip_quantize_grouped_batch (one threshold per batch, up to 16 tensors per launch and one launch per 16 beyond, empty tensors skipped,
 * a tensor whose input, residual or output is not 16-byte aligned goes through a guarded element-by-element launch that writes the same bytes).
 * Device (or pinned) buffers only; stream-ordered on the context's stream (always behind the previous call,
 * whatever piquant_hip_set_independent_calls says: the residual is the previous step's output), no host synchronisation, no allocation
 * (hipGraph-capturable).  numel == 0 is a no-op. */
PIQUANT_EXPORT void piquant_hip_quantize_grouped_ef(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* residual, void* out,
                                                    piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales, uint8_t* zero_points,
                                                    piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_quantize_grouped_ef_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                          void* const* residuals, void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                          size_t group_size, float* const* scales, uint8_t* const* zero_points, size_t count,
                                                          piquant_round_mode_t mode);

/* The three error-feedback calls with the residual's type named: a FLOAT32 residual for a BFLOAT16 tensor.  A bfloat16 residual rounds y = x + r
 * and r <- y - d to bfloat16, each by up to 2^-9 |y| -- as much as the half step of a uint8 wire it is there to keep; a float32 residual keeps
 * what the wire loses to float32 precision while the tensor (and the wire, and what receivers decode into) stay as they are.
 * dtype_residual == dtype_in (dtype_acc): the call IS its counterpart above.  (dtype_in, dtype_residual) == (BF16, F32): `residual` holds numel
 * float32 elements and the call writes exactly the bytes of piquant_hip_quantize_grouped_ef(widen(x), F32, residual, ...), widen(x) being x
 * converted to float32 (exact):
 *   1. y[i] = rn_f32(widen(x[i]) + residual[i]);
 *   2. (out, scales, zero_points) = piquant_hip_quantize_grouped(y) in the float32 pipeline with computed parameters;
 *   3. d[i] = element i of piquant_hip_dequantize_grouped(out, scales, zero_points, dtype F32, PIQUANT_REDUCE_OP_SET);
 *   4. residual[i] = rn_f32(y[i] - d[i]), a subtraction of its own, never contracted into an fma.
 * The NaN rule, degenerate and clamped groups, one stochastic threshold per call (per batch) and the per-element mode indexing the global element
 * are the float32 call's.  x is never written; nothing at or past the tensor's end is touched.  ONE launch per call and per 16 tensors of a batch,
 * 11 bytes of memory traffic per element with a uint8 wire, against 19 for the widened copy plus the float32 call.  The streaming kernels need
 * residual and out 16-byte aligned and x 8-byte aligned; anything else goes through a guarded element-by-element launch that writes the same bytes.
 * A receiver that decodes the wire into bfloat16 forms d in the bfloat16 dequantize form, which before its rounding to bfloat16 may differ from
 * the sender's float32-form d by at most one float32 ulp.
 * piquant_hip_reduce_quantize_grouped_ef_mixed with (BF16, F32) writes the bytes of the composition that defines it:
 * piquant_hip_dequantize_grouped(..., PIQUANT_REDUCE_OP_ADD) of every term into the bfloat16 acc, in order (acc <- rn_bf16(widen(acc) + d_i), one
 * rounding to bfloat16 per term), then piquant_hip_quantize_grouped_ef_mixed(acc, residual) with the call's one threshold.  ONE launch for up to
 * 16 terms (the surplus is added into acc by grouped dequantize ADD launches first) when the terms, residual and out are 16-byte aligned and acc
 * 8-byte aligned: the accumulator is read once (12 bytes of memory traffic per element with one uint8 term, against 16 for the composition; 18
 * against 46 with seven); with any buffer misaligned the composition itself runs, count + 1 launches.  acc is unspecified afterwards.
 * Any other pair of types aborts.  Device (or pinned) buffers only; stream-ordered on the context's stream, always behind the previous call; no
 * host synchronisation, no allocation (hipGraph-capturable); empty tensors are skipped. */
PIQUANT_EXPORT void piquant_hip_quantize_grouped_ef_mixed(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* residual,
                                                          piquant_dtype_t dtype_residual, void* out, piquant_dtype_t dtype_out, size_t numel,
                                                          size_t group_size, float* scales, uint8_t* zero_points, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_quantize_grouped_ef_mixed_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                                void* const* residuals, piquant_dtype_t dtype_residual, void* const* outputs,
                                                                piquant_dtype_t dtype_out, const size_t* numels, size_t group_size,
                                                                float* const* scales, uint8_t* const* zero_points, size_t count,
                                                                piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_reduce_quantize_grouped_ef_mixed(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc, void* residual,
                                                                 piquant_dtype_t dtype_residual, const void* const* inputs,
                                                                 const float* const* input_scales, const uint8_t* const* input_zero_points,
                                                                 size_t count, void* out, piquant_dtype_t dtype_out, size_t numel, size_t group_size,
                                                                 float* scales, uint8_t* zero_points, piquant_round_mode_t mode);

/* Group-wise quantize-dequantize ("fake quantization"): out (op)= dequantize_grouped(quantize_grouped(in)) -- what the tensor looks like after a
 * group-wise round trip -- in ONE launch that reads `in` once and never writes the packed tensor.  dtype_in_out (float32 or bfloat16) is the type
 * of both `in` and `out`; quant_dtype is the quantized type passed through (uint8, uint4 or uint2); group_size as above.  The call writes to out,
 * scales and zero_points exactly the bytes that this composition of two public calls writes, tmp being a packed scratch tensor:
 *   1. piquant_hip_quantize_grouped(in, dtype_in_out, tmp, quant_dtype, numel, group_size, scales, zero_points, params_given, mode);
 *   2. piquant_hip_dequantize_grouped(tmp, quant_dtype, out, dtype_in_out, numel, group_size, scales, zero_points, op).
 * Nearest and stochastic rounding as piquant_hip_quantize_grouped (ONE threshold per call, which piquant_hip_set_stochastic_threshold pins; the
 * per-element mode indexes the global element).  params_given == 0: the group parameters are computed by piquant_hip_quantize_grouped's rules and
 * written -- or scales and zero_points are BOTH NULL, and nothing is written for them (one NULL and one non-NULL aborts).  params_given != 0: both
 * arrays are read and required.  The dequantized value is the pair's own dequantize form; SET stores it (bfloat16: rounded once), ADD is the grouped
 * dequantize ADD (the float32 sum rounded separately, a bfloat16 result rounded once).  NaN payloads are not specified.
 * `out` may be exactly `in` (in place), for SET and for ADD; any other overlap of the two is the caller's error.  `in` is never written unless it is
 * `out`; nothing at or past the tensor's end is touched in any buffer.  Buffers that are not 16-byte aligned take a guarded element-by-element
 * launch that writes the same bytes; a buffer that is not aligned to its element aborts.
 * piquant_hip_quantize_dequantize_grouped_batch: tensor i has its own input, output, scales, zero_points and numels[i], with the rules of
 * piquant_hip_quantize_grouped_batch (one threshold per batch, up to 16 tensors per launch and one launch per 16 beyond, empty tensors skipped, a
 * misaligned tensor runs alone in its place in the sequence).  With params_given == 0 the lists scales and zero_points may both be NULL.
 * Device (or pinned) buffers only; stream-ordered on the context's stream -- always behind the previous call when op is ADD or the parameters are
 * given, otherwise as piquant_hip_quantize_grouped is -- no host synchronisation, no allocation (hipGraph-capturable).  numel == 0 is a no-op
 * that draws no threshold. */
PIQUANT_EXPORT void piquant_hip_quantize_dequantize_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in_out, void* out,
                                                            piquant_dtype_t quant_dtype, size_t numel, size_t group_size, float* scales,
                                                            uint8_t* zero_points, int params_given, piquant_round_mode_t mode,
                                                            piquant_reduce_op_t op);
PIQUANT_EXPORT void piquant_hip_quantize_dequantize_grouped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in_out,
                                                                  void* const* outputs, piquant_dtype_t quant_dtype, const size_t* numels,
                                                                  size_t group_size, float* const* scales, uint8_t* const* zero_points, size_t count,
                                                                  int params_given, piquant_round_mode_t mode, piquant_reduce_op_t op);

/* RANDOMIZED HADAMARD ROTATION of the groups (opt-in; no other call changes).  A group is quantized against its own min and max, so one large
 * element stretches the step of its whole group; rotating every group by a random-sign diagonal and a normalised Walsh-Hadamard matrix before it is
 * quantized spreads such an element over the group, and the rotation is undone after dequantizing.  It is orthogonal: the L2 error is the same in
 * both domains.  Heavy-tailed data gains (DESIGN.md 4d has the ratios), Gaussian data is unaffected, flat data gets worse.
 * THE ROTATION of group size G = 2^k (one of the eight group sizes) with a 64-bit seed acts on float32 values, one FULL group at a time:
 *   signs        d[j], j in [0, G), is -1 if bit (j mod 16) of floor(t * 2^24) is set, t the per-element counter-hash threshold
 *                (piquant_hip_set_stochastic_per_element) of seed `seed` and index j div 16; otherwise +1.  The signs depend on the position inside
 *                the group only: every group uses the same d, so a shard that starts on a group boundary rotates exactly as the whole tensor does.
 *   butterflies  fwht(v): for h = 1, 2, 4, ..., G / 2 in this order and every pair (i, i + h) with bit h of i clear,
 *                (v[i], v[i + h]) <- (v[i] + v[i + h], v[i] - v[i + h]), each sum and difference ONE float32 operation.  The stage order is part of
 *                the contract: it fixes every rounding, so the result is bit-reproducible.
 *   constant     c_G = 2^(-k / 2) as a float32: the exact power of two for even k, float32(sqrt 2) (bits 0x3FB504F3) * 2^(-(k + 1) / 2) for odd k
 *   forward      y = c_G * fwht(d * x)            inverse      x = d * (c_G * fwht(y))          (one multiply per element behind the last stage)
 * A ragged last group (numel % G != 0; a tensor shorter than G is one) is NOT rotated: forward and inverse are the identity on it.  Non-finite
 * inputs propagate as IEEE says (one NaN makes its whole group NaN); NaN payloads are not specified.
 * piquant_hip_hadamard_grouped: each full group of out is the forward (inverse == 0) or inverse rotation of that group of in; `dtype` (float32 or
 *   bfloat16) is the type of both, and out may be exactly in.  bfloat16 is widened, transformed in float32 and rounded to bfloat16 (nearest even)
 *   on store.
 * piquant_hip_quantize_grouped_rotated: bit for bit piquant_hip_quantize_grouped(y, float32, ..., params_given = 0, mode), y the float32 forward
 *   rotation of the widened tensor -- a bfloat16 tensor is never rounded back before it is quantized.  Packed bytes, scales[ngroups] and
 *   zero_points[ngroups] are written as piquant_hip_quantize_grouped writes them; all three rounding modes (the per-element mode indexes the
 *   global element); the parameters are always computed.  One launch that never writes y.
 * piquant_hip_dequantize_grouped_rotated: z = the float32 inverse rotation of piquant_hip_dequantize_grouped(in, ..., float32, SET); SET stores z
 *   converted to dtype_out, ADD stores convert(widen(out) + z) with one float32 add and one rounding.  One launch that never writes the
 *   un-rotated intermediate.
 * All six dtype pairs, all eight group sizes.  Buffers that are not 16-byte aligned take guarded one-wave-per-group launches that write the same
 * bytes; a float buffer that is not aligned to its element aborts.  Nothing outside the tensors is read or written.  Device (or pinned) buffers
 * only; stream-ordered on the context's stream -- the first two as piquant_hip_quantize_grouped is, the dequantize always behind the previous call
 * -- no host synchronisation, no allocation, the seed travels by value (hipGraph-capturable).  numel == 0 is a no-op that draws no threshold. */
PIQUANT_EXPORT void piquant_hip_hadamard_grouped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype, void* out, size_t numel,
                                                 size_t group_size, uint64_t seed, int inverse);
PIQUANT_EXPORT void piquant_hip_quantize_grouped_rotated(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out,
                                                         piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales,
                                                         uint8_t* zero_points, uint64_t seed, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_dequantize_grouped_rotated(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out,
                                                           piquant_dtype_t dtype_out, size_t numel, size_t group_size, const float* scales,
                                                           const uint8_t* zero_points, uint64_t seed, piquant_reduce_op_t op);

/* THE GROUPED COLLECTIVES' STEPS IN THE ROTATED DOMAIN.  The rotation is linear and the same on every rank for the same seed, so records made by
 * piquant_hip_quantize_grouped_rotated are summed as they are: only the local accumulator is rotated forward (reduce), or only the finished sum is
 * rotated back (dequantize-sum) -- ONE rotation a call, whatever the number of terms.  Both calls work in float32 whatever the tensor's type.
 * Term i is a packed tensor of numel elements with its own per-group parameters input_scales[i] / input_zero_points[i] (one group_size for all).
 * piquant_hip_reduce_quantize_grouped_rotated writes to out, scales and zero_points exactly the bytes of this composition of public calls:
 *   1. y = piquant_hip_hadamard_grouped(widen(acc) as float32, forward, seed): a float32 tensor; a bfloat16 acc is widened and never rounded back;
 *   2. piquant_hip_dequantize_grouped(inputs[i], dtype_out -> float32, ..., PIQUANT_REDUCE_OP_ADD) into y for i = 0 .. count - 1 in order: one
 *      separately rounded float32 add per term;
 *   3. piquant_hip_quantize_grouped(y, float32 -> dtype_out, params_given = 0, mode): all three rounding modes, the per-element mode indexing the
 *      global element.
 *   acc is const and is NOT written (piquant_hip_reduce_quantize_grouped leaves its accumulator unspecified).  That call rounds the running sum to
 *   bfloat16 after every term of a bfloat16 accumulator; this one never does: the sum stays float32 until it is quantized.  count == 0 is bit for
 *   bit piquant_hip_quantize_grouped_rotated.  Every hop of a rotated grouped ring (count = 1); a mesh owner that needs the sum itself takes the call
 *   below.
 * piquant_hip_dequantize_sum_grouped_rotated: s = piquant_hip_dequantize_grouped(inputs[0] -> float32, SET) -- the first term is stored, not added
 *   to zero --, s += piquant_hip_dequantize_grouped(inputs[i] -> float32) for i = 1 .. count - 1 in order, in float32;
 *   z = piquant_hip_hadamard_grouped(s, inverse, seed).  SET stores convert(z) and never reads out; ADD stores convert(widen(out) + z) with one
 *   float32 add and one rounding.  count == 1 is bit for bit piquant_hip_dequantize_grouped_rotated; count == 0 aborts like a NULL argument.  The
 *   owner's step of a rotated grouped reduce-scatter and, followed by piquant_hip_quantize_grouped_rotated, of a rotated grouped mesh all-reduce.
 * Both: at most 16 terms -- more abort with a message: there is no scratch to spill a float32 running sum into, and the library never allocates.
 * All six dtype pairs, all eight group sizes; a ragged last group is not rotated (its terms are still added); NaN payloads are not specified.
 * acc / out and every term's packed bytes 16-byte aligned: ONE streaming launch (no LDS traffic for the butterflies, no scan, no atomics, no grid
 * barrier); anything else element-aligned: ONE guarded one-wave-per-group launch that writes the same bytes; a float buffer that is not aligned to
 * its element aborts.  Nothing at or past a tensor's end is read or written; out must not overlap a term or acc.  Device (or pinned) buffers only;
 * stream-ordered on the context's stream, always behind the previous call whatever piquant_hip_set_independent_calls says; no host
 * synchronisation, no allocation on the device, the seed travels by value (hipGraph-capturable).  numel == 0 is a no-op that draws no threshold. */
PIQUANT_EXPORT void piquant_hip_reduce_quantize_grouped_rotated(piquant_context_t* ctx, const void* acc, piquant_dtype_t dtype_acc,
                                                                const void* const* inputs, const float* const* input_scales,
                                                                const uint8_t* const* input_zero_points, size_t count, void* out,
                                                                piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales,
                                                                uint8_t* zero_points, uint64_t seed, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_dequantize_sum_grouped_rotated(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                               const float* const* input_scales, const uint8_t* const* input_zero_points,
                                                               size_t count, void* out, piquant_dtype_t dtype_out, size_t numel, size_t group_size,
                                                               uint64_t seed, piquant_reduce_op_t op);

/* ERROR FEEDBACK IN THE ROTATED DOMAIN.  The rotation is orthogonal and linear, and for one seed it is the same on every step and every rank, so
 * the residual of error feedback need never leave the rotated domain: sum_t D_t = sum_t H(x_t) + R_0 - R_K holds there and maps back through the
 * inverse rotation unchanged.  `residual` is numel float32 values -- float32 also for a bfloat16 tensor -- that belong to ONE (seed, group size):
 * a record of rotated values, not interchangeable with the residual of piquant_hip_quantize_grouped_ef.
 * piquant_hip_quantize_grouped_rotated_ef writes exactly the packed bytes, scales, zero points and residual of this composition of public calls:
 *   1. Y = piquant_hip_hadamard_grouped(widen(in) as float32, forward, seed): a bfloat16 tensor is widened and never rounded back; a ragged last
 *      group is not rotated;
 *   2. piquant_hip_quantize_grouped_ef(Y, float32, residual, ...): per element y = rn_f32(Y + R); quantize_grouped(y) with computed parameters;
 *      d = the float32 SET dequantize; R <- rn_f32(y - d).
 *   It never writes Y, and `in` is only read.
 * piquant_hip_reduce_quantize_grouped_rotated_ef writes exactly what this sequence writes:
 *   1. steps 1 and 2 of piquant_hip_reduce_quantize_grouped_rotated: Y = the rotation of widen(acc), then one separately rounded float32
 *      dequantize ADD per term, in order;
 *   2. piquant_hip_quantize_grouped_ef(Y, float32, residual, ...): the residual is added BEHIND the terms, as in
 *      piquant_hip_reduce_quantize_grouped_ef.
 *   acc is const and only read.  count == 0 is bit for bit the first call; more than 16 terms abort with a message.
 * Both: all six dtype pairs, all eight group sizes, all three rounding modes -- one threshold per call, which
 * piquant_hip_set_stochastic_threshold pins; the per-element mode indexes the global element.  in / acc 16-byte (float32) or 8-byte (bfloat16)
 * aligned and residual, out and every term's packed bytes 16-byte aligned: ONE streaming launch (no scan, no atomics, no grid barrier, no LDS
 * traffic for the butterflies); anything else element-aligned: ONE guarded one-wave-per-group launch that writes the same bytes; a float buffer
 * that is not aligned to its element aborts.  Nothing at or past a tensor's end is read or written; the buffers must not overlap.  Device (or
 * pinned) buffers only; stream-ordered on the context's stream, always behind the previous call whatever piquant_hip_set_independent_calls
 * says; no host synchronisation, no allocation, the seed travels by value (hipGraph-capturable).  numel == 0 is a no-op that draws no threshold.
 * QUIRKS.  One NaN in a full group makes the whole rotated group NaN, so that group's residual is NaN from then on: it stays NaN until the caller
 * zeroes it (the un-rotated calls lose one element only).  A group of nothing but NaNs gets the parameters (1.0, qmax >> 1) as everywhere.
 * LEAVING THE ROTATED DOMAIN.  piquant_hip_hadamard_grouped(residual, float32, inverse = 1, seed) gives the residual of the original domain up to
 * float32 rounding, and the forward call takes it back: that is the way to change the seed or to stop rotating without dropping what is owed. */
PIQUANT_EXPORT void piquant_hip_quantize_grouped_rotated_ef(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, float* residual,
                                                            void* out, piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales,
                                                            uint8_t* zero_points, uint64_t seed, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_reduce_quantize_grouped_rotated_ef(piquant_context_t* ctx, const void* acc, piquant_dtype_t dtype_acc,
                                                                   float* residual, const void* const* inputs, const float* const* input_scales,
                                                                   const uint8_t* const* input_zero_points, size_t count, void* out,
                                                                   piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales,
                                                                   uint8_t* zero_points, uint64_t seed, piquant_round_mode_t mode);

/* BATCHES OF THE ROTATED CALLS: what piquant_hip_quantize_grouped_batch, piquant_hip_dequantize_grouped_batch and
 * piquant_hip_quantize_grouped_ef_batch are to their single calls.  Tensor i has its own input, output, scales, zero_points and numels[i] (and
 * residuals[i]: numels[i] float32 values, float32 also for bfloat16 tensors); all share the dtype pair, group_size, the rotation's seed and the
 * round mode / op.  The bytes each call writes are those of this composition of public calls, for i = 0 .. count - 1 in order:
 *   piquant_hip_quantize_grouped_rotated_batch     piquant_hip_quantize_grouped_rotated(inputs[i], ..., outputs[i], numels[i], scales[i],
 *                                                  zero_points[i], seed, mode)
 *   piquant_hip_dequantize_grouped_rotated_batch   piquant_hip_dequantize_grouped_rotated(inputs[i], ..., outputs[i], numels[i], scales[i],
 *                                                  zero_points[i], seed, op)
 *   piquant_hip_quantize_grouped_rotated_ef_batch  piquant_hip_quantize_grouped_rotated_ef(inputs[i], ..., residuals[i], outputs[i], numels[i],
 *                                                  scales[i], zero_points[i], seed, mode)
 *   with ONE stochastic threshold (or per-element seed and base) for the whole batch where the loop of single calls would draw one per call: the
 *   batch draws once whenever count > 0, also when every member is empty; count == 0 returns before anything is drawn.  In per-element mode every
 *   member indexes its own elements from 0.  A batch is its members, not their concatenation: the ragged last group of EACH member is not rotated.
 * The parameters are always computed.  Empty members are skipped; up to 16 members go out in ONE streaming launch (more: one launch per 16); a
 * member that fails the single call's alignment rule (quantize and dequantize: in and out 16-byte aligned; error feedback: in 16-byte, or 8-byte
 * for bfloat16, residual and out 16-byte aligned) runs alone, in its place in the sequence, through the guarded one-wave-per-group launch of the
 * single call: the same bytes.  A float buffer that is not aligned to its element aborts with the member's index.  Nothing outside a member's
 * buffers is read or written; the buffers must not overlap.  Device (or pinned) buffers only; stream-ordered on the context's stream -- the
 * quantize as piquant_hip_quantize_grouped_batch with computed parameters, the dequantize and the error-feedback batch always behind the previous
 * call whatever piquant_hip_set_independent_calls says --; no host synchronisation, no allocation, the seed travels by value
 * (hipGraph-capturable).  One encode and one decode launch is what a rotated grouped mesh all-reduce of up to 17 ranks makes of them. */
PIQUANT_EXPORT void piquant_hip_quantize_grouped_rotated_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                               void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                               size_t group_size, float* const* scales, uint8_t* const* zero_points, size_t count,
                                                               uint64_t seed, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_dequantize_grouped_rotated_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                                 void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                                 size_t group_size, const float* const* scales, const uint8_t* const* zero_points,
                                                                 size_t count, uint64_t seed, piquant_reduce_op_t op);
PIQUANT_EXPORT void piquant_hip_quantize_grouped_rotated_ef_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                                  float* const* residuals, void* const* outputs, piquant_dtype_t dtype_out,
                                                                  const size_t* numels, size_t group_size, float* const* scales,
                                                                  uint8_t* const* zero_points, size_t count, uint64_t seed,
                                                                  piquant_round_mode_t mode);

/* PER-GROUP CLIP SEARCH.  piquant_hip_quantize_grouped takes a group's step from its min and max, which on a narrow wire spends most codes on the
 * tails.  piquant_hip_quantize_grouped_clipped tries, for every group on its own, `steps` (1 .. 12) ranges shrunk towards zero and keeps the one
 * whose round trip loses the least squared error -- in ONE launch that reads `in` once.  A searched group is an ordinary group with other
 * parameters: the wire format and every dequantizing call are untouched.  The parameters are always computed.
 * THE DEFINITION, every step float32 unless it says otherwise.  xf is `in` widened to float32.  For every FULL group g, with lo, hi the min and
 * max piquant_hip_quantize_grouped finds (NaNs ignored):
 *   1. candidate k, 0 <= k < steps: lo_k = lo * r_k, hi_k = hi * r_k, one multiplication each, r_k = 1 - k / 16 (exact); (scale_k, zp_k) is
 *      piquant_hip_quant_params_from_minmax(lo_k, hi_k), the zero point clamped to [0, qmax] as everywhere.  Candidate 0 is exactly the pair of
 *      piquant_hip_quantize_grouped.  A candidate with not hi_k > lo_k is skipped;
 *   2. its error, ALWAYS with nearest rounding whatever `mode` is: q = the position-independent quantize of the group with (scale_k, zp_k);
 *      d = what piquant_hip_dequantize_grouped(q, ..., float32, PIQUANT_REDUCE_OP_SET) stores -- float32 also for a bfloat16 `in`;
 *      e_i = xf_i - d_i and s_i = e_i * e_i, two roundings, never an fma; s_i = +0 where xf_i is a NaN; E_k = the sum of s_0 .. s_{G-1} by the
 *      adjacent-pair tree (replace s by s[2j] + s[2j+1] until one value is left), nothing fused;
 *   3. best = 0; for k = 1 .. steps - 1 in order: if E_k < E_best then best = k.  Strict: a NaN E_k never wins, a tie keeps the smaller k, and
 *      an E_0 that is NaN or +inf is never beaten;
 *   4. NOT searched (best = 0): a degenerate group (not hi > lo: constant, all NaN), the ragged last group, every group when steps == 1;
 *   5. the bytes of `out` are those of piquant_hip_quantize_grouped(in, ..., scales, zero_points, params_given = 1, mode) with the chosen pairs,
 *      in every rounding mode (ONE threshold per call; the per-element mode indexes the global element); scales[g] / zero_points[g] hold the
 *      chosen pair and choices[g] -- uint8[ngroups], device, may be NULL -- receives best.
 * steps == 1 is piquant_hip_quantize_grouped with computed parameters, bit for bit.  steps outside [1, 12] aborts.
 * Buffers that are not 16-byte aligned take a guarded one-wave-per-group launch that writes the same bytes; `in` not aligned to its element aborts.
 * piquant_hip_quantize_grouped_clipped_batch: tensor i has its own input, output, scales, zero_points, numels[i] and choices[i] (the list, or any
 * entry of it, may be NULL), with the rules of piquant_hip_quantize_grouped_batch: member i gets the bytes, parameters and choices of the single
 * call on it, one threshold per batch, up to 16 tensors per launch and one launch per 16 beyond, empty tensors skipped, a misaligned member runs
 * alone in its place in the sequence.
 * Device (or pinned) buffers only; stream-ordered on the context's stream as piquant_hip_quantize_grouped with computed parameters is; no scan, no
 * atomics, no grid barrier, no host synchronisation, no allocation (hipGraph-capturable).  numel == 0 is a no-op that draws no threshold. */
PIQUANT_EXPORT void piquant_hip_quantize_grouped_clipped(piquant_context_t* ctx, const void* in, piquant_dtype_t dtype_in, void* out,
                                                         piquant_dtype_t dtype_out, size_t numel, size_t group_size, float* scales,
                                                         uint8_t* zero_points, uint8_t* choices, int steps, piquant_round_mode_t mode);
PIQUANT_EXPORT void piquant_hip_quantize_grouped_clipped_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                               void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                               size_t group_size, float* const* scales, uint8_t* const* zero_points,
                                                               uint8_t* const* choices, size_t count, int steps, piquant_round_mode_t mode);

/* HISTOGRAM CLIP SEARCH for per-tensor parameters.  piquant_hip_compute_quant_params_device takes the step from the tensor's min and max; on a
 * tensor of 10^6 .. 10^8 elements the extremes lie 5 sigma and more out, and a narrow wire spends most codes on empty range.
 * piquant_hip_compute_quant_params_clipped_device judges `steps` (1 .. PIQUANT_HIP_CLIP_MAX_STEPS) ranges shrunk towards zero on a histogram of the
 * tensor -- one more streaming pass, whatever the number of candidates -- and writes the record of the one with the smallest estimated squared error.
 * The record is an ordinary record: piquant_hip_quantize_dp, piquant_hip_dequantize_dp and every wire take it as it is.
 * The counts are integers: exact in any order, in any grid and across ranks (a sharded caller adds ONE SUM all-reduce of the counts to the scan's
 * MIN all-reduce of the keys), so the whole search is reproducible bit for bit.
 * THE DEFINITION.  x is float32, or bfloat16 widened exactly; qmax = 2^bits - 1 of the target type; B = PIQUANT_HIP_CLIP_BINS.
 *   1. RANGE.  (lo, hi) is the scan's float32 minimum and maximum, NaNs ignored: the pair behind piquant_hip_compute_quant_params_device and
 *      piquant_hip_minmax_keys.  If nothing was scanned, or not hi > lo, the counts stay zero, no candidate is evaluated, and the result is that
 *      call's record with choice 0 -- decided on the device, the call stays stream-ordered.  steps == 1 searches nothing either: that call's record,
 *      choice 0, no error evaluated (piquant_hip_compute_quant_params_clipped_device decides this on the host and forwards to that call).
 *   2. COUNTS.  Only non-NaN elements are counted.  In float32, each operation rounded on its own: wf = hi - lo (may be +inf); inv = B / wf (may be
 *      0 or +inf); t = (x - lo) * inv; bin = int(min(max(t, 0), B - 1)) with a NaN t giving 0 (the fmaxf(NaN, 0) = 0 rule: +-inf inputs and an
 *      overflowing range are defined).  c[j], uint64, is the number of elements in bin j.
 *   3. CANDIDATES.  r_k = 1 - k / 64 (exact), lo_k = fl32(lo * r_k), hi_k = fl32(hi * r_k), 0 <= k < steps.  Candidate k is evaluated iff k == 0 or
 *      hi_k > lo_k; (s_k, z_k) is the ordinary epilogue on (lo_k, hi_k), 0 <= z_k <= qmax; candidate 0 is piquant_hip_compute_quant_params_device's
 *      pair.  Its error, in binary64, every operation rounded once, nothing fused:  W = (double(hi) - double(lo)) / B;  m_j = double(lo) + (j + 0.5) * W;
 *      u = floor(m_j / double(s_k) + 0.5) + z_k, clamped to [0, qmax], a NaN giving 0;  d = (u - z_k) * double(s_k);  e = m_j - d;
 *      term_j = double(c_j) * (e * e), and exactly +0 where c_j == 0;  E_k = the sum of the B terms by the adjacent-pair tree (replace t by
 *      t[2j] + t[2j+1] until one value is left).  An E_k that is NaN is stored as the one pattern 0x7ff8000000000000.
 *   4. CHOICE.  best = 0; for k = 1 .. steps - 1 in order: if E_k < E_best then best = k.  Strict: a tie or a NaN keeps the smaller k.
 * RESULT: the record {s_best, fl32(1 / s_best), z_best} and the choice.
 * The search ESTIMATES the error: bin centres stand for the elements, and the rounding mode of the quantizing call plays no part.  The definition is
 * the histogram's, not the round trip's.  r_k >= 1/32: an outlier beyond 32 x the bulk is out of reach, the bulk then shares a few bins.
 *
 * piquant_hip_clip_histogram: device_hist (uint64[PIQUANT_HIP_CLIP_BINS]) receives the counts of x against the range in device_keys (int32[2], as
 *   piquant_hip_minmax_keys leaves them -- or as a MIN all-reduce over ranks does); init != 0 zeroes the counts first, several calls with init == 0
 *   accumulate (shards, parts).  n == 0 with init == 0 does nothing.
 * piquant_hip_quant_params_from_histogram: steps 3 and 4 on given keys and counts.  device_choice (int32) and device_errors (double[63]; entry k is
 *   E_k, NaN where candidate k was not evaluated or k >= steps) may be NULL.
 * piquant_hip_compute_quant_params_clipped_device: keys (init), histogram (init), search, on scratch of the context.
 * x not aligned to 16 bytes is counted like the scan scans it (a few leading elements one by one; not even element-aligned: element by element);
 * nothing outside the tensor is read.  Device (or pinned) buffers only.  Stream-ordered on the context's stream, no host synchronisation, no float
 * atomics, no grid barrier.  The scratch is allocated by the context's first such call; from the second on a call allocates nothing and can be
 * captured into a hipGraph.  A wrong dtype or steps outside [1, PIQUANT_HIP_CLIP_MAX_STEPS] aborts. */
#define PIQUANT_HIP_CLIP_BINS 8192
#define PIQUANT_HIP_CLIP_MAX_STEPS 63
PIQUANT_EXPORT void piquant_hip_clip_histogram(piquant_context_t* ctx, const void* x, piquant_dtype_t dtype, size_t n, const int32_t* device_keys,
                                               uint64_t* device_hist, int init);
PIQUANT_EXPORT void piquant_hip_quant_params_from_histogram(piquant_context_t* ctx, const int32_t* device_keys, const uint64_t* device_hist,
                                                            piquant_dtype_t target_quant_dtype, int steps, piquant_hip_params_t* device_params,
                                                            int32_t* device_choice, double* device_errors);
PIQUANT_EXPORT void piquant_hip_compute_quant_params_clipped_device(piquant_context_t* ctx, const void* x, piquant_dtype_t dtype, size_t n,
                                                                    piquant_dtype_t target_quant_dtype, int steps,
                                                                    piquant_hip_params_t* device_params, int32_t* device_choice,
                                                                    double* device_errors);

/* INDEPENDENT CALLS (opt-in, off by default).  Calls on a stream run one after the other: the dispatch packet of every kernel carries a barrier
 * bit, the next kernel starts when the previous one has drained, and the ~2 us in which a launch ramps up and drains move no bytes (9 % of a
 * 23 us quantize at numel 27 264 000, a third of a 5 us shard).  A caller that quantizes or dequantizes tensor after tensor -- the gradients of a
 * data-parallel step -- knows what the library cannot: that each call depends on nothing still in flight.  With enabled != 0 the context's
 * stream-ordered piquant_quantize / piquant_dequantize launches (and their *_dp twins) go out WITHOUT that barrier bit (hipExtAnyOrderLaunch):
 * a call's ramp runs under the drain of whatever precedes it in the queue.  fp32 -> uint8 at numel 27 264 000: 22.9 -> 21.6 us per call, 0.745 ->
 * 0.789 of the HBM peak; same bytes (profiles/r05_split_call_ab.csv).
 * THE PROMISE the caller makes while it is on: a call's input was not written, and its output is neither read nor written, by any work
 * enqueued on the stream that may still be running when the call is made -- the previous calls of this context included.  Everything enqueued
 * AFTER such a call (other kernels, event records, hipStreamSynchronize, this context's calls with the mode off) still waits for it: ordinary
 * packets wait for all packets in front of them.  Blocking contexts and calls inside a hipGraph capture ignore the mode. */
PIQUANT_EXPORT void piquant_hip_set_independent_calls(piquant_context_t* ctx, int enabled);

/* The one-launch kernel's grid barrier never waits without bound: a block that has waited `microseconds` (default 1000) for the
 * rest of its grid -- which on an idle GPU arrives within a few microseconds -- assumes that the missing blocks cannot start
 * because something else holds their CUs (a kernel of another stream or process, an RCCL kernel waiting for a peer), hands its
 * share over and exits, freeing its CU.  The barrier still opens when the last block has arrived; the blocks resident then also
 * quantize the shares that were handed over, from HBM.  Results are identical; only the time differs.  0 restores the default.
 * piquant_hip_barrier_bailouts returns how many blocks ever left a barrier of this context early (0 in normal operation;
 * synchronises the context's stream).  PIQUANT_HIP_BARRIER_HAND_OVER_ALWAYS as the limit is for tests of that path: every block
 * of a launch except the last one of each tensor hands its share over without waiting at all, whatever the GPU's scheduling does
 * (bailouts grows by blocks - 1 per tensor per launch; same bytes, same record). */
#define PIQUANT_HIP_BARRIER_HAND_OVER_ALWAYS 0xffffffffu
PIQUANT_EXPORT void piquant_hip_set_barrier_timeout_us(piquant_context_t* ctx, uint32_t microseconds);
PIQUANT_EXPORT uint64_t piquant_hip_barrier_bailouts(piquant_context_t* ctx);

/* piquant_hip_quantize_dynamic for `count` independent tensors of the same dtype pair, each with its own parameters and its own
 * 16-byte record: outputs[i] = quantize(inputs[i]) with (scale, zero_point) from inputs[i].  Up to 16 tensors share ONE kernel
 * launch (the grid is cut into one sub-grid per tensor, each with its own barrier), which is what a rank of a mesh all-reduce
 * needs when it quantizes one chunk per peer, or a trainer with many small gradient tensors.  PIQUANT_STOCHASTIC draws one
 * threshold for the whole batch.  Results are identical to `count` single calls. */
PIQUANT_EXPORT void piquant_hip_quantize_dynamic_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                       void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                       piquant_hip_params_t* const* device_params, size_t count,
                                                       piquant_round_mode_t mode);

/* piquant_hip_dequantize_dp for `count` independent tensors of the same dtype pair in one launch per 16 tensors:
 * outputs[i] (op)= dequantize(inputs[i]) with the parameters of tensor i read from its device record. */
PIQUANT_EXPORT void piquant_hip_dequantize_dp_batch(piquant_context_t* ctx, const void* const* inputs, piquant_dtype_t dtype_in,
                                                    void* const* outputs, piquant_dtype_t dtype_out, const size_t* numels,
                                                    const piquant_hip_params_t* const* device_params, size_t count,
                                                    piquant_reduce_op_t op);

/* The owner's step of a mesh all-reduce in one call: out = quantize(acc + dequantize(inputs[0]) + dequantize(inputs[1]) + ...)
 * with the parameters computed from that sum and left in *device_params.  `inputs` are `count` quantized tensors of type
 * dtype_out (the type being produced), each with its device record; terms are added in order, the running sum rounded to
 * dtype_acc after each.  When everything stays on chip (a chunk of an all-reduce always does) this is ONE launch that never
 * writes the sum to memory; otherwise it is piquant_hip_dequantize_sum into `acc` followed by piquant_hip_quantize_dynamic.
 * The output bytes and the record are identical either way; the contents of `acc` afterwards are unspecified (unchanged by
 * the one-launch form, the sum after the two-step form). */
PIQUANT_EXPORT void piquant_hip_reduce_quantize_dynamic(piquant_context_t* ctx, void* acc, piquant_dtype_t dtype_acc,
                                                        const void* const* inputs,
                                                        const piquant_hip_params_t* const* input_params, size_t count, void* out,
                                                        piquant_dtype_t dtype_out, size_t numel,
                                                        piquant_hip_params_t* device_params, piquant_round_mode_t mode);

/* out (op)= dequantize(inputs[0]) + dequantize(inputs[1]) + ... : `count` quantized tensors of the same dtype and length, each
 * with its own 16-byte parameter record in device memory, summed into one float tensor in a single pass -- the reduction
 * step of a quantized all-reduce in which a rank receives one chunk from every peer (xGMI is a point-to-point mesh: all
 * peers send at once).  Bit-identical to `count` piquant_hip_dequantize_dp calls in order (the first with `op`, the others
 * with ADD), but the accumulator is read and written once instead of `count` times.  Device (or pinned) buffers only. */
PIQUANT_EXPORT void piquant_hip_dequantize_sum(piquant_context_t* ctx, const void* const* inputs,
                                               const piquant_hip_params_t* const* device_params, size_t count,
                                               piquant_dtype_t dtype_in, void* out, piquant_dtype_t dtype_out, size_t numel,
                                               piquant_reduce_op_t op);

/* compute_quant_params of a tensor whose shards live on several GPUs, for C / C++ hosts (one process per GPU): every
 * rank passes its local shard and its RCCL communicator (an ncclComm_t as void*).  Local HIP scan -> {key(min), key(-max)}
 * -> ONE ncclAllReduce(2 x int32, ncclMin) over xGMI on the context's stream -> identical double-precision epilogue on
 * every rank.  RCCL is resolved at run time from the copy already loaded in the process (the symbol ncclAllReduce), so
 * libpiquant.so does not link it; the call aborts with a message if no RCCL is loaded.  Synchronous like
 * piquant_compute_quant_params_*. */
PIQUANT_EXPORT void piquant_hip_compute_quant_params_dist(piquant_context_t* ctx, const void* local_shard, piquant_dtype_t dtype,
                                                          size_t n_local, piquant_dtype_t target_quant_dtype, void* nccl_comm,
                                                          float* out_scale, int64_t* out_zero_point);

/* Device memory that other GPUs of the node -- or other processes on this GPU -- may map into their address space (HIP IPC), the ground the
 * peer-to-peer schedules below stand on.  piquant_hip_peer_alloc allocates `bytes` (a multiple of 4) on the context's device, fills them with
 * fill_word, and writes the allocation's 64-byte IPC handle to out_ipc_handle -- to be carried to the peers by whatever the caller has (a
 * torch.distributed all_gather, MPI, a socket).  fine_grained != 0 gives memory that stays coherent with other agents WHILE kernels run: flags
 * and mailboxes that another GPU writes and a kernel of this one polls; payload buffers that are consumed by a LATER launch may be ordinary
 * (coarse-grained) memory, which is faster.  piquant_hip_peer_open maps a peer's allocation for this context's device (peer access is enabled
 * on the way) and returns the local address; close before the owner frees.  Abort with a message on any HIP error, as everywhere. */
#define PIQUANT_HIP_IPC_HANDLE_BYTES 64
PIQUANT_EXPORT void* piquant_hip_peer_alloc(piquant_context_t* ctx, size_t bytes, int fine_grained, uint32_t fill_word, void* out_ipc_handle);
PIQUANT_EXPORT void* piquant_hip_peer_open(piquant_context_t* ctx, const void* ipc_handle);
PIQUANT_EXPORT void piquant_hip_peer_close(piquant_context_t* ctx, void* mapped);
PIQUANT_EXPORT void piquant_hip_peer_free(piquant_context_t* ctx, void* allocated);

/* Flags for peer-to-peer schedules between GPUs (or between processes on one GPU): sequence numbers in device memory that a peer
 * writes and the owner polls -- what lets a quantize kernel store its bytes straight into a peer's receive buffer (an address obtained from
 * hipIpcOpenMemHandle or a peer-accessible allocation) instead of local write -> collective -> local read (piquant.distributed,
 * quantized_all_reduce(transport='p2p'); the use-case of reference README.md:29).  Both calls are stream-ordered on the context's stream:
 *   piquant_hip_signal_flags  stores `value` into every flags[i] (system-scope release) once everything enqueued before it has completed;
 *   piquant_hip_wait_flags    holds the stream until every flags[i] (an array in THIS device's memory) has reached `value` (serial-number
 *                             compare, so a 32-bit counter may wrap); a peer that has not arrived after timeout_us (0 = 10 minutes, what
 *                             torch.distributed gives a collective; at most ~71 minutes) is REPORTED, see piquant_hip_peer_timeout.  Not
 *                             capturable into a hipGraph. */
PIQUANT_EXPORT void piquant_hip_signal_flags(piquant_context_t* ctx, uint32_t* const* flags, size_t count, uint32_t value);
PIQUANT_EXPORT void piquant_hip_wait_flags(piquant_context_t* ctx, const uint32_t* flags, size_t count, uint32_t value, uint32_t timeout_us);

/* compute_quant_params of a sharded tensor WITHOUT a collective library, for GPUs of one node: the MIN all-reduce of the ranks' {key(min),
 * key(-max)} pairs (the path's only exchange, 8 bytes) done by ONE one-wave kernel over peer-mapped mailboxes -- lane j stores this rank's
 * pair into its slot of rank j's mailbox (an xGMI store) and polls slot j of the own mailbox until rank j's pair is there; the folded pair goes
 * to out_keys (device or pinned host memory).  A collective of this size is all latency: the launch and protocol of an all-reduce against
 * one store and one poll per peer.  Stream-ordered on the context's stream.
 *   device_keys  this rank's int32[2] pair in device memory (piquant_hip_minmax_keys);
 *   my_slots     `count` 8-byte words in THIS device's memory, all holding 0x7fffffff7fffffff when first used (the kernel empties what it
 *                reads); a caller alternates between TWO such mailboxes from one exchange to the next (see piquant.distributed);
 *   peer_slots   peer_slots[j] = the address of slot [this rank] in rank j's mailbox of the same parity (peer-mapped; j = this rank: own).
 * A peer that has not arrived after timeout_us (0 = 10 minutes) is reported (piquant_hip_peer_timeout).  Not capturable into a hipGraph.  count <= 64. */
PIQUANT_EXPORT void piquant_hip_exchange_minmax_keys(piquant_context_t* ctx, const int32_t* device_keys, uint64_t* const* peer_slots, uint64_t* my_slots,
                                                     size_t count, int32_t* out_keys, uint32_t timeout_us);

/* A wait of the two calls above that ran out does NOT fault the GPU queue (round 4 trapped, which killed this process and, through the mapped
 * memory, its peers): the waiting wave writes what it was missing into a pinned record of the context, the stream goes on -- whatever was enqueued
 * behind the wait consumes stale bytes -- and the host finds out here.  Returns 0 (nothing happened), 1 (piquant_hip_wait_flags: flag *out_rank of
 * the array waited on read *out_seen instead of *out_expected) or 2 (piquant_hip_exchange_minmax_keys: rank *out_rank never delivered its pair),
 * and clears the record.  Reads host memory only; synchronise the stream first to be sure the wait in question is over.  A record nobody fetched
 * makes the context's NEXT peer-to-peer call abort with a message naming the rank, so a host that never asks still fails loudly, one call late.
 * While a record is pending (round 6): the FIRST failure is the one kept -- a later wait that also runs out does not overwrite it --, further
 * waits on this context return at once instead of spinning out their own timeouts, and piquant_hip_signal_flags signals NOTHING: a rank that gave
 * up does not tell its peers that its step is finished (they time out on it and name it, instead of consuming bytes it never wrote).  After a
 * kind-2 timeout the mailboxes are in an unknown state (pairs may arrive late into either parity): free them and exchange handles again before
 * the next exchange.  piquant.distributed asks after every exchange it synchronises on and before every new one, raises RuntimeError, and marks
 * the peer mesh of that kind as poisoned: its next use is refused until piquant.distributed.release_peer_meshes() has let it be rebuilt. */
PIQUANT_EXPORT int piquant_hip_peer_timeout(piquant_context_t* ctx, uint32_t* out_rank, uint32_t* out_expected, uint32_t* out_seen);

/* Host helpers: key <-> float, and the (min,max) -> (scale, zero_point) epilogue in double precision
 * (reference src/piquant.cpp:213-220, 245-258).  keys[0] encodes min, keys[1] encodes -max. */
PIQUANT_EXPORT void piquant_hip_decode_minmax_keys(const int32_t keys[2], float* out_min, float* out_max);
PIQUANT_EXPORT void piquant_hip_quant_params_from_minmax(float min, float max, piquant_dtype_t target_quant_dtype,
                                                         float* out_scale, int64_t* out_zero_point);

/* HIP device ordinal the context is bound to. */
PIQUANT_EXPORT int piquant_hip_device(const piquant_context_t* ctx);

/* "piquant-hip <version> gfx950" */
PIQUANT_EXPORT const char* piquant_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PIQUANT_HIP_H */
