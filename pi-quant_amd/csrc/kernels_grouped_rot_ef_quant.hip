// Instantiation and launch of the rotated grouped quantize with error feedback (grouped_rot_ef_kernels.hpp: quantize_grouped_rotated_ef_kernel):
// its 144 streaming instances (two tensor types, three widths, three rounding modes, eight group sizes) compile next to the other kernel units,
// on the same flags.  The guarded launch is the reduce's without terms (kernels_grouped_rot_ef_reduce.hip).
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_rot_ef_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

// The pipeline is the float32 one whatever the tensor's type, and the residual is float32.
void launch_quantize_grouped_rotated_ef(const GroupedEfLaunch& q, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu) {
    const char* name = "quantize_grouped_rotated_ef";
    if (q.numel <= 0) return;
    if (guarded) {
        launch_reduce_quantize_grouped_rotated_ef(GroupedReduceLaunch {q, q, {}, 0}, rot_seed, true, stream, num_cu);
        return;
    }
    const QuantParams p = grouped_call_params(q.rm);
    const int64_t ngroups = (q.numel + q.group_size - 1) / q.group_size;
    const uint32_t lo = static_cast<uint32_t>(rot_seed), hi = static_cast<uint32_t>(rot_seed >> 32);
    uint8_t* out = static_cast<uint8_t*>(q.out);
    float* residual = static_cast<float*>(q.residual);
    with_float_type(q.dt_in, [&](auto di) {
        constexpr int DT_IN = decltype(di)::value;
        with_quant_bits(q.dt_out, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            with_round_mode<DT_F32, BITS>(q.rm.round_mode, [&](auto mi) {
                constexpr int MODE = decltype(mi)::value;
                with_group_size(q.group_size, name, [&](auto gi) {
                    constexpr int G = decltype(gi)::value;
                    constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                    const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, name));
                    PQ_LAUNCH((quantize_grouped_rotated_ef_kernel<DT_IN, BITS, MODE, G>), grid, dim3(kGroupedBlock), 0, stream, q.in, residual, out, q.numel,
                              q.scales, q.zero_points, ngroups, lo, hi, p);
                });
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
