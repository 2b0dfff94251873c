// Group-wise quantize-dequantize (grouped_requant_kernels.hpp): the bfloat16 kernels.  A translation unit of its own; the launchers that pick it are
// in kernels_grouped_requant.hip.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "grouped_requant_kernels.hpp"

namespace pq {

void launch_quantize_dequantize_grouped_batch_bf16(const GroupedRequantBatchLaunch& b, hipStream_t stream) { requant_batch<DT_BF16>(b, stream); }

void launch_quantize_dequantize_grouped_guarded_bf16(const GroupedRequantLaunch& q, hipStream_t stream, int num_cu) {
    requant_guarded<DT_BF16>(q, stream, num_cu);
}

}  // namespace pq
