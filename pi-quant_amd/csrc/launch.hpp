// Host-visible launch interface of the HIP kernels (implemented in kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace pq {

struct QuantLaunch {
    const void* in;        // device-accessible
    void* out;             // device-accessible
    int64_t numel;
    int dt_in;             // DT_F32 / DT_BF16
    int dt_out;            // DT_UINT2/4/8
    int round_mode;        // RM_* (device_math.hpp)
    float inv_scale;
    int64_t zero_point;
    float threshold;
    uint64_t seed;
    uint64_t index_base;
    const void* dyn_params;   // nullable: 16-byte device ParamRecord overriding inv_scale / zero_point
    bool ref_layout;          // reference-layout mode (see QuantParams)
    int64_t ref_total;
    int64_t ref_index0;
    int ref_threads;          // pool threads of the reference context being reproduced (0 / 1: one partition)
    int ref_out_align;        // (out as the caller passed it) & 15 for fp32 -> uint8 nearest, -1 otherwise
    uint32_t barrier_timeout_us;   // fused launches: longest wait at the grid barrier before a block gives up its share (0 = 1 ms)
};

struct DequantLaunch {
    const void* in;
    void* out;
    int64_t numel;
    int dt_in;             // DT_UINT2/4/8
    int dt_out;            // DT_F32 / DT_BF16
    int op;                // OP_SET / OP_ADD
    float scale;
    float bias;
    int64_t zero_point;
    const void* dyn_params;   // nullable: 16-byte device ParamRecord overriding scale / bias / zero_point
    bool ref_layout;
    int64_t ref_total;
    int64_t ref_index0;
    int ref_threads;
};

struct RequantLaunch {
    const void* in;        // may equal out (in-place)
    void* out;
    int64_t numel;
    int dt_inout;          // DT_F32 / DT_BF16 (input and output type)
    int quant_dtype;       // DT_UINT2/4/8 (the type passed through)
    int round_mode;        // RM_*
    int op;                // OP_SET / OP_ADD
    float scale;
    float scale_bf16;      // scale rounded to bf16 and widened back (bf16 path multiplies by this)
    float inv_scale;
    int64_t zero_point;
    float threshold;
    uint64_t seed;
    uint64_t index_base;
};

// out (op)= sum of `count` quantized inputs of type dt_in, input i with its own 16-byte device ParamRecord (dequant_kernels.hpp)
constexpr int kDequantSumMaxInputs = 16;
struct DequantSumLaunch {
    const void* in[kDequantSumMaxInputs];
    const void* params[kDequantSumMaxInputs];
    int count;
    void* out;
    int64_t numel;
    int dt_in;
    int dt_out;
    int op;
};
void launch_dequantize_sum(const DequantSumLaunch& d, hipStream_t stream, int num_cu);

// out[g] (op)= dequantize(in[g]) for up to kDequantBatchMaxInputs independent tensors in one launch, parameters of tensor g from
// its 16-byte device ParamRecord (dequant_kernels.hpp)
constexpr int kDequantBatchMaxInputs = 16;
struct DequantBatchLaunch {
    const void* in[kDequantBatchMaxInputs];
    void* out[kDequantBatchMaxInputs];
    const void* params[kDequantBatchMaxInputs];
    int64_t numel[kDequantBatchMaxInputs];
    int count;
    int dt_in;
    int dt_out;
    int op;
};
void launch_dequantize_batch(const DequantBatchLaunch& d, hipStream_t stream);

// Group-wise quantization (grouped_kernels.hpp): one (scale, zero point) per run of group_size contiguous elements, group_size a power of
// two in [32, 4096].  Quantize computes the parameters (written to scales / zero_points) or, with params_given, reads them; either way ONE
// launch.  Buffers 16-byte aligned take the streaming kernels, anything else the guarded one-wave-per-group kernel.
// Every grouped descriptor is made of the same three pieces: what one tensor brings (GroupedTensor), what the members of a call share
// (GroupedQuantCall / GroupedDequantCall) and, in the former, the call's round-mode fields.  A single launch is {tensor, call}, a batch is the call
// plus up to kGroupedBatchMaxTensors tensors, so "run member i alone" is GroupedQuantLaunch {b.t[i], b}.
constexpr int kGroupedMinG = 32, kGroupedMaxG = 4096;
struct RoundModeFields {   // context.hpp, round_mode_fields
    int round_mode;        // RM_* (device_math.hpp)
    float threshold;
    uint64_t seed;
    uint64_t index_base;
};
struct GroupedTensor {
    const void* in;        // the tensor; the accumulator of a reduce
    void* residual;        // error feedback only: numel elements, read and written
    void* out;
    float* scales;         // float32[ngroups], device (dequantize only reads the parameters)
    uint8_t* zero_points;  // uint8[ngroups], device
    int64_t numel;
    uint8_t* choices = nullptr;   // clip search only: uint8[ngroups], device, written; may stay NULL
};
struct GroupedQuantCall {
    int64_t group_size;
    int dt_in;             // DT_F32 / DT_BF16
    int dt_out;            // DT_UINT2/4/8
    bool params_given;     // plain quantize only
    RoundModeFields rm;
};
struct GroupedDequantCall {
    int64_t group_size;
    int dt_in;             // DT_UINT2/4/8
    int dt_out;            // DT_F32 / DT_BF16
    int op;                // OP_SET / OP_ADD
};
struct GroupedQuantLaunch : GroupedTensor, GroupedQuantCall {};
struct GroupedDequantLaunch : GroupedTensor, GroupedDequantCall {};

// Batches (up to kGroupedBatchMaxTensors tensors of one dtype pair, group size and round mode in ONE launch, every buffer 16-byte aligned and every
// tensor non-empty: the caller sends anything else through the single calls) and the fused reduce + quantize (every buffer 16-byte aligned, at
// most kGroupedReduceMaxInputs terms: the caller adds the surplus first, or runs the two-step form for misaligned buffers).
constexpr int kGroupedBatchMaxTensors = 16;
template <class Call>
struct GroupedBatch : Call {
    GroupedTensor t[kGroupedBatchMaxTensors];
    int count;
};
using GroupedQuantBatchLaunch = GroupedBatch<GroupedQuantCall>;
using GroupedDequantBatchLaunch = GroupedBatch<GroupedDequantCall>;

// out, scales, zero_points = quantize_grouped(in + sum_i dequantize_grouped(term[i])), terms added in order; dt_out is the terms' type too.
// Error feedback on the re-quantized partial sum (grouped_kernels.hpp, reduce_quantize_grouped_ef_kernel) is the same descriptor with the residual,
// of dt_in and numel elements, 16-byte aligned: y = in + terms + residual, (out, scales, zero_points) = quantize_grouped(y),
// residual <- y - dequantize_grouped(out), in ONE launch.
constexpr int kGroupedReduceMaxInputs = 16;
struct GroupedReduceLaunch : GroupedTensor, GroupedQuantCall {
    GroupedTensor term[kGroupedReduceMaxInputs];   // in, scales and zero_points are read
    int count;
};

// out (op)= sum_i dequantize_grouped(term[i]), terms added in order, the running sum rounded to dt_out after each one (grouped_kernels.hpp,
// dequantize_sum_grouped_kernel): ONE launch for 1 .. kGroupedReduceMaxInputs terms.  `out` (numel elements of dt_out) and every term's packed
// bytes 16-byte aligned: the caller sends anything else through launch_dequantize_grouped, term by term (the same bytes).
struct GroupedDequantSumLaunch : GroupedDequantCall {
    void* out;
    int64_t numel;
    GroupedTensor term[kGroupedReduceMaxInputs];   // in, scales and zero_points are read
    int count;
};

// Error feedback (grouped_kernels.hpp, quantize_grouped_ef_batch_kernel): per tensor y = in + residual, (out, scales, zero_points) =
// quantize_grouped(y) with computed parameters, residual <- y - dequantize_grouped(out), in ONE launch for up to kGroupedBatchMaxTensors tensors
// (every buffer 16-byte aligned, every tensor non-empty; a batch of one launches quantize_grouped_ef_kernel, whose arguments are leading scalars).
// launch_quantize_grouped_ef_guarded runs one tensor alone through the element-by-element kernel: the same bytes for buffers of any alignment.
using GroupedEfBatchLaunch = GroupedQuantBatchLaunch;   // every t[i].residual set; params_given unused
using GroupedEfLaunch = GroupedQuantLaunch;

// Quantize-dequantize (kernels_grouped_requant.hip): per tensor out (op)= dequantize_grouped(quantize_grouped(in)) in ONE launch that never writes
// the packed tensor.  in and out have type dt_in and may be the same buffer; dt_out is the quantized type passed through.  scales / zero_points are
// read with params_given, written otherwise -- or both NULL then: no parameters wanted.  The batch takes tensors whose in and out are 16-byte
// aligned (a batch of one launches the single-tensor kernel); the guarded launch runs one tensor of any element alignment, the same bytes.
struct GroupedRequantCall : GroupedQuantCall {
    int op;                // OP_SET / OP_ADD
};
struct GroupedRequantLaunch : GroupedTensor, GroupedRequantCall {};
using GroupedRequantBatchLaunch = GroupedBatch<GroupedRequantCall>;

// All launches are asynchronous on `stream`; num_cu sizes capped grids.
void launch_quantize(const QuantLaunch& q, hipStream_t stream, int num_cu);
void launch_dequantize(const DequantLaunch& d, hipStream_t stream, int num_cu);
void launch_requantize(const RequantLaunch& r, hipStream_t stream, int num_cu);
void launch_quantize_grouped(const GroupedQuantLaunch& q, hipStream_t stream, int num_cu);
void launch_dequantize_grouped(const GroupedDequantLaunch& d, hipStream_t stream, int num_cu);
void launch_quantize_grouped_batch(const GroupedQuantBatchLaunch& b, hipStream_t stream);
void launch_dequantize_grouped_batch(const GroupedDequantBatchLaunch& b, hipStream_t stream);
void launch_reduce_quantize_grouped(const GroupedReduceLaunch& r, hipStream_t stream);
void launch_quantize_grouped_ef_batch(const GroupedEfBatchLaunch& b, hipStream_t stream);
void launch_reduce_quantize_grouped_ef(const GroupedReduceLaunch& r, hipStream_t stream);
void launch_quantize_grouped_ef_guarded(const GroupedEfLaunch& q, hipStream_t stream, int num_cu);
// The same two for bfloat16 tensors (b.dt_in == DT_BF16) whose residuals are float32 (kernels_grouped_ef_f32r.hip): the bytes of the float32 call
// on the widened tensor.  The streaming launch needs residual and out 16-byte aligned and the tensor 8-byte aligned; the guarded one takes anything.
void launch_quantize_grouped_ef_f32r_batch(const GroupedEfBatchLaunch& b, hipStream_t stream);
void launch_quantize_grouped_ef_f32r_guarded(const GroupedEfLaunch& q, hipStream_t stream, int num_cu);
// The fused reduce with error feedback for that pair (kernels_grouped_reduce_ef_f32r.hip): r.dt_in == DT_BF16, r.residual float32.  Terms, residual
// and out 16-byte aligned, the accumulator 8-byte aligned (its lane-row is four elements), at most kGroupedReduceMaxInputs terms.
void launch_reduce_quantize_grouped_ef_f32r(const GroupedReduceLaunch& r, hipStream_t stream);
void launch_dequantize_sum_grouped(const GroupedDequantSumLaunch& d, hipStream_t stream);   // kernels_grouped_dequant_sum.hip
void launch_quantize_dequantize_grouped_batch(const GroupedRequantBatchLaunch& b, hipStream_t stream);
void launch_quantize_dequantize_grouped_guarded(const GroupedRequantLaunch& q, hipStream_t stream, int num_cu);
// The randomized Hadamard rotation of whole groups (grouped_rot_kernels.hpp; kernels_grouped_rot.hip, kernels_grouped_rot_quant.hip).  The three
// streaming launches need in and out 16-byte aligned; `guarded` runs the one-wave-per-group kernels instead: any element alignment, the same bytes.
struct GroupedHadamardLaunch {
    const void* in;
    void* out;             // same type; may be in
    int64_t numel;
    int64_t group_size;
    int dt;                // DT_F32 / DT_BF16
    uint64_t seed;
    bool inverse;
};
void launch_hadamard_grouped(const GroupedHadamardLaunch& h, bool guarded, hipStream_t stream, int num_cu);
// quantize_grouped (computed parameters; params_given is not used) of the float32 forward rotation of the widened tensor, which is never written
void launch_quantize_grouped_rotated(const GroupedQuantLaunch& q, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu);
// out (op)= the inverse rotation of the float32 grouped dequantize of in, which is never written
void launch_dequantize_grouped_rotated(const GroupedDequantLaunch& d, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu);
// The two steps of a grouped collective in the rotated domain (kernels_grouped_rot_reduce.hip, kernels_grouped_rot_dequant_sum.hip), ONE launch
// each for at most kGroupedReduceMaxInputs terms (the dequantize-sum: at least one); the streaming launches need the accumulator / out and every
// term's packed bytes 16-byte aligned, `guarded` takes any element alignment: the same bytes.
// out, scales, zero_points = quantize_grouped(rotate(widen(in)) + sum_i dequantize_grouped(term[i] -> float32)), in float32; in is only read
void launch_reduce_quantize_grouped_rotated(const GroupedReduceLaunch& r, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu);
// out (op)= the inverse rotation of the float32 sum of the terms' grouped dequantizes
void launch_dequantize_sum_grouped_rotated(const GroupedDequantSumLaunch& d, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu);
// Error feedback in the rotated domain (grouped_rot_ef_kernels.hpp; kernels_grouped_rot_ef_quant.hip, kernels_grouped_rot_ef_reduce.hip): the two
// rotated quantizing launches above with `residual` set -- numel float32 values of the ROTATED domain whatever dt_in is, read and written:
// y = rotate(widen(in)) [+ terms] + residual, (out, scales, zero_points) = quantize_grouped(y), residual <- y - dequantize_grouped(out), ONE launch.
// Streaming: residual, out and every term's packed bytes 16-byte aligned, in 16-byte (float32) or 8-byte (bfloat16) aligned; `guarded`: anything
// element-aligned, the same bytes.
void launch_quantize_grouped_rotated_ef(const GroupedEfLaunch& q, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu);
void launch_reduce_quantize_grouped_rotated_ef(const GroupedReduceLaunch& r, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu);
// The batched rotated launches (kernels_grouped_rot_batch*.hip): up to kGroupedBatchMaxTensors tensors of one dtype pair, group size, round mode and
// rotation seed in ONE launch of the streaming kernel -- every member non-empty and aligned as the single streaming launch needs it (the caller
// sends anything else through the guarded single launches); member i gets the bytes of the single launch on member i.  A batch of one launches the
// single-tensor kernel.  Every t[i].residual of the error-feedback batch is float32.
void launch_quantize_grouped_rotated_batch(const GroupedQuantBatchLaunch& b, uint64_t rot_seed, hipStream_t stream);
void launch_dequantize_grouped_rotated_batch(const GroupedDequantBatchLaunch& b, uint64_t rot_seed, hipStream_t stream);
void launch_quantize_grouped_rotated_ef_batch(const GroupedEfBatchLaunch& b, uint64_t rot_seed, hipStream_t stream);
// quantize_grouped with a per-group clip search (grouped_clip_kernels.hpp; kernels_grouped_clip.hip): every full, non-degenerate group tries `steps`
// (1 .. 12) shrunk ranges and is quantized with the one whose nearest round trip loses least; parameters always computed (params_given is not
// used), t.choices -- where not NULL -- receives the winners' indices.  The batch takes members whose in and out are 16-byte aligned, ONE launch (a
// batch of one launches the single-tensor kernel); the guarded launch runs one tensor of any element alignment, the same bytes.
void launch_quantize_grouped_clipped_batch(const GroupedQuantBatchLaunch& b, int steps, hipStream_t stream);
void launch_quantize_grouped_clipped_guarded(const GroupedQuantLaunch& q, int steps, hipStream_t stream, int num_cu);
// Histogram clip search for per-tensor parameters (clip_params_kernels.hpp; kernels_clip_params.hip).  `keys` is the scan's device {key(min), key(-max)}.
// launch_clip_histogram: hist (uint64[8192], device) = or += the counts of `in` against the keys' range -- one streaming launch that leaves one
// uint32[8192] row per block in `partials` (clip_partial_bytes(num_cu) of device scratch, clip_partial_rows(num_cu) rows) and a fold launch; numel == 0
// zeroes (init) or does nothing.  launch_clip_search: steps blocks judge the candidates from `hist` into errors_scratch (double[63], device), one wave
// chooses and writes the 16-byte record and, where not NULL, the choice and the 63 errors (NaN: not evaluated).  steps == 1 launches the wave alone.
// launch_clip_unsearched: choice 0 and 63 NaNs, what a call that forwards to the plain scan still owes its caller.
size_t clip_partial_rows(int num_cu);
size_t clip_partial_bytes(int num_cu);
void launch_clip_histogram(const void* in, int dt_in, int64_t numel, const int32_t* keys, uint32_t* partials, size_t partial_rows, uint64_t* hist, bool init,
                           hipStream_t stream);
void launch_clip_search(const int32_t* keys, const uint64_t* hist, int bits, int steps, double* errors_scratch, void* device_param_record, int32_t* device_choice,
                        double* device_errors, hipStream_t stream);
void launch_clip_unsearched(int32_t* device_choice, double* device_errors, hipStream_t stream);
// Min/max scan.  `state` is a minmax_state_ints() int32 device buffer armed once with launch_arm_slots: one 8-byte result word
// per block (the "gather" end: every block stores its word, the highest block folds them) and, for scans that accumulate
// into one state (MM_NONE), 64 slot key pairs on separate 128-byte lines plus arrival counters.  Either way the block that finishes
// the scan re-arms what it read and runs the epilogue inside the SAME launch, so a scan is one kernel and always leaves `state` armed:
//   MM_KEYS_SET / MM_KEYS_MIN  dst = int32[2] device {key(min), key(-max)}, overwritten / accumulated with MIN
//   MM_PUBLISH                 dst = device-visible address of a MinmaxMailboxHost in pinned fine-grained host memory
//   MM_PARAMS                  dst = 16-byte device ParamRecord (scale, 1/scale, zero point) for `bits`-wide quantization
//   MM_NONE                    keys stay in the slots (several scans into one buffer); finish with launch_minmax_epilogue
enum : int { MM_NONE = 0, MM_KEYS_SET = 1, MM_KEYS_MIN = 2, MM_PUBLISH = 3, MM_PARAMS = 4 };
struct MinmaxAction {
    int action = MM_NONE;
    int bits = 0;
    uint32_t seq = 0;
    void* dst = nullptr;
};
struct MinmaxMailboxHost {
    int32_t keys[2];
    uint32_t seq;
    uint32_t pad;
};
void launch_minmax(const void* in, int dt_in, int64_t numel, int32_t* state, const MinmaxAction& action, hipStream_t stream, int num_cu);
// Fold + epilogue as a launch of its own (after MM_NONE scans, or on an armed buffer for an empty input: identities).
void launch_minmax_epilogue(int32_t* state, const MinmaxAction& action, bool rearm, hipStream_t stream);
void launch_arm_slots(int32_t* state, hipStream_t stream, bool scan_state = true);   // scan_state: a minmax_state_ints() buffer (slots + per-block words)
int minmax_state_ints();
// compute_quant_params + quantize in one launch with the tensor resident on chip between the two passes (fused_kernels.hpp).
// q.inv_scale / q.zero_point / q.dyn_params are ignored: the parameters come from the data and are also written to
// device_param_record.  `state` is a fused_state_bytes() device buffer prepared once with init_fused_state().  Returns false
// without launching when the call does not qualify (tensor larger than the chip holds, misaligned buffers, reference-layout
// mode): the caller then runs the scan (parameter epilogue in its last block) and the quantize kernel, with identical results.
bool launch_fused_params_quantize(const QuantLaunch& q, void* state, void* device_param_record, hipStream_t stream, int num_cu);
// The same for up to kFusedBatchMax independent tensors in ONE launch (dtype pair and rounding mode from `q`, whose buffers are
// ignored): the grid is cut into one sub-grid per tensor, each with its own barrier and parameters.  false when the batch does
// not qualify (a misaligned buffer, an empty tensor, a tensor too large for its sub-grid): launch them one by one instead.
constexpr int kFusedBatchMax = 16;
struct FusedBatch {
    const void* in[kFusedBatchMax];
    void* out[kFusedBatchMax];
    int64_t numel[kFusedBatchMax];
    void* params[kFusedBatchMax];   // 16-byte device ParamRecord per tensor
    int count;
};
bool launch_fused_params_quantize_batch(const QuantLaunch& q, const FusedBatch& b, void* state, hipStream_t stream, int num_cu);
bool fused_launch_applies(const QuantLaunch& q, int num_cu);   // the test launch_fused_params_quantize makes, without launching
// The same kernel fed with in + sum of dequantized `terms` (dt_in of the terms == q.dt_out; terms.out / terms.op unused): the
// owner's step of a mesh all-reduce.  false when it does not qualify -- then dequantize_sum into `in` followed by the plain
// fused call gives the same bytes.  Declared after DequantSumLaunch.
bool launch_fused_reduce_quantize(const QuantLaunch& q, const DequantSumLaunch& terms, void* state, void* device_param_record, hipStream_t stream,
                                  int num_cu);
// one-thread kernel: system-scope store of `seq` into a host-visible word, behind everything enqueued on `stream` so far
void launch_publish_seq(uint32_t* host_visible_word, uint32_t seq, hipStream_t stream);
// peer-to-peer schedules: `value` into every flags[i] (addresses other devices / processes poll), and the wait for every flags[i] to reach it
constexpr int kFlagListMax = 32;
void launch_signal_flags(uint32_t* const* flags, int count, uint32_t value, const uint32_t* timeout_record, hipStream_t stream);   // record set (a wait gave up): signals nothing
// A peer that does not arrive within the limit is REPORTED, not trapped on: {kind, index of the missing rank, value waited for, value seen} in
// `timeout_record` (4 pinned host-coherent words; nullptr: trap) and the stream goes on (kernels.hip, report_peer_timeout)
constexpr uint32_t kPeerTimeoutDefaultUs = 600000000u;   // 10 minutes
enum : uint32_t { kPeerTimeoutNone = 0, kPeerTimeoutFlags = 1, kPeerTimeoutKeys = 2 };
void launch_wait_flags(const uint32_t* flags, int count, uint32_t value, uint32_t timeout_us, uint32_t* timeout_record, hipStream_t stream);
// MIN all-reduce of one {key(min), key(-max)} word per rank through peer-mapped mailboxes (kernels.hip, exchange_keys_kernel)
constexpr int kKeyExchangeMaxRanks = 64;
constexpr unsigned long long kKeyWordEmpty = 0x7fffffff7fffffffull;
void launch_exchange_keys(const int32_t* my_keys, unsigned long long* const* peer_slots, unsigned long long* my_slots, int count, int32_t* out_keys, uint32_t timeout_us,
                          uint32_t* timeout_record, hipStream_t stream);
size_t fused_state_bytes();
void init_fused_state(void* state, hipStream_t stream);
// blocks of fused launches on `state` that left their grid barrier early so far (synchronises `stream`)
uint64_t fused_state_bailouts(const void* state, hipStream_t stream);

// Aborts with the reference's panic convention (red message on stderr, abort()) on a HIP error.
void check_hip(hipError_t e, const char* what, const char* file, int line);
[[noreturn]] void panic(const char* fmt, ...);

#define PQ_HIP(expr) ::pq::check_hip((expr), #expr, __FILE__, __LINE__)

}  // namespace pq
