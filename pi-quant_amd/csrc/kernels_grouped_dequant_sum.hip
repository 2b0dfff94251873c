// Instantiation and launch of the grouped dequantize-sum (grouped_kernels.hpp: dequantize_sum_grouped_kernel).  A translation unit of its own: its
// 96 instances (six dtype pairs, eight group sizes, SET and ADD) compile next to the other kernel units.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

struct DequantSumFamily {
    static constexpr const char* name = "dequantize_sum_grouped";
    template <int DT_OUT, int BITS, int OP, int G>
    static auto kernel() {
        return &dequantize_sum_grouped_kernel<DT_OUT, BITS, OP, G>;
    }
};

}  // namespace

void launch_dequantize_sum_grouped(const GroupedDequantSumLaunch& d, hipStream_t stream) { launch_grouped_dequant_sum<DequantSumFamily>(d, stream); }

}  // namespace pq
