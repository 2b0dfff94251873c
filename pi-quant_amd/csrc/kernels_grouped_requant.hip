// Group-wise quantize-dequantize (grouped_requant_kernels.hpp): the float32 kernels, and the two launchers of launch.hpp, which pick the half by
// the tensor's type.  A translation unit of its own, as kernels_grouped_requant_bf16.hip is for the bfloat16 kernels.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "grouped_requant_kernels.hpp"

namespace pq {

void launch_quantize_dequantize_grouped_batch_f32(const GroupedRequantBatchLaunch& b, hipStream_t stream) { requant_batch<DT_F32>(b, stream); }

void launch_quantize_dequantize_grouped_guarded_f32(const GroupedRequantLaunch& q, hipStream_t stream, int num_cu) {
    requant_guarded<DT_F32>(q, stream, num_cu);
}

void launch_quantize_dequantize_grouped_batch(const GroupedRequantBatchLaunch& b, hipStream_t stream) {
    switch (b.dt_in) {
        case DT_F32: launch_quantize_dequantize_grouped_batch_f32(b, stream); return;
        case DT_BF16: launch_quantize_dequantize_grouped_batch_bf16(b, stream); return;
        default: panic("quantize_dequantize_grouped: invalid float type %d", b.dt_in);
    }
}

void launch_quantize_dequantize_grouped_guarded(const GroupedRequantLaunch& q, hipStream_t stream, int num_cu) {
    switch (q.dt_in) {
        case DT_F32: launch_quantize_dequantize_grouped_guarded_f32(q, stream, num_cu); return;
        case DT_BF16: launch_quantize_dequantize_grouped_guarded_bf16(q, stream, num_cu); return;
        default: panic("quantize_dequantize_grouped: invalid float type %d", q.dt_in);
    }
}

}  // namespace pq
