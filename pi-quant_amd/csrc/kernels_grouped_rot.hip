// Instantiation and launch of the stand-alone grouped Hadamard rotation and of the rotated grouped dequantize (grouped_rot_kernels.hpp).  A
// translation unit of its own, on the flags of the other kernel units (-ffp-contract=off: every butterfly is a separately rounded operation); the
// rotated quantize is kernels_grouped_rot_quant.hip.
#define PQ_MINMAX_HELPERS_ONLY   // the scan state kernels are defined in kernels.hip
#include "launch.hpp"

#include "grouped_dispatch.hpp"
#include "grouped_rot_kernels.hpp"
#include "stop_event.hpp"

namespace pq {

namespace {

// grid of the guarded rotation kernels: one wave (one block) per group, grid-stride beyond 64 blocks per CU (256 CUs when num_cu is not known)
unsigned rot_guarded_blocks(int64_t ngroups, int num_cu) {
    const int64_t cap = static_cast<int64_t>(64) * (num_cu > 0 ? num_cu : 256);
    return static_cast<unsigned>(ngroups < cap ? ngroups : cap);
}

}  // namespace

void launch_hadamard_grouped(const GroupedHadamardLaunch& h, bool guarded, hipStream_t stream, int num_cu) {
    const char* name = "hadamard_grouped";
    if (h.numel <= 0) return;
    const int64_t ngroups = (h.numel + h.group_size - 1) / h.group_size;
    const uint32_t lo = static_cast<uint32_t>(h.seed), hi = static_cast<uint32_t>(h.seed >> 32);
    with_float_type(h.dt, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        if (guarded) {
            if (h.group_size < kGroupedMinG || h.group_size > kGroupedMaxG || (h.group_size & (h.group_size - 1)) != 0)
                panic("%s: group size %lld", name, static_cast<long long>(h.group_size));
            const dim3 grid(rot_guarded_blocks(ngroups, num_cu));
            if (h.inverse) PQ_LAUNCH((hadamard_grouped_scalar_kernel<DT, true>), grid, dim3(kGroupedRotGuardedBlock), 0, stream, h.in, h.out, h.numel,
                                     h.group_size, ngroups, lo, hi);
            else PQ_LAUNCH((hadamard_grouped_scalar_kernel<DT, false>), grid, dim3(kGroupedRotGuardedBlock), 0, stream, h.in, h.out, h.numel, h.group_size,
                           ngroups, lo, hi);
            return;
        }
        with_group_size(h.group_size, name, [&](auto gi) {
            constexpr int G = decltype(gi)::value;
            constexpr int NG = GroupedQuantTile<DT_F32, 8, G>::NG;
            const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, name));
            if (h.inverse) PQ_LAUNCH((hadamard_grouped_kernel<DT, G, true>), grid, dim3(kGroupedBlock), 0, stream, h.in, h.out, h.numel, ngroups, lo, hi);
            else PQ_LAUNCH((hadamard_grouped_kernel<DT, G, false>), grid, dim3(kGroupedBlock), 0, stream, h.in, h.out, h.numel, ngroups, lo, hi);
        });
    });
    PQ_HIP(hipGetLastError());
}

void launch_dequantize_grouped_rotated(const GroupedDequantLaunch& d, uint64_t rot_seed, bool guarded, hipStream_t stream, int num_cu) {
    const char* name = "dequantize_grouped_rotated";
    if (d.numel <= 0) return;
    const int64_t ngroups = (d.numel + d.group_size - 1) / d.group_size;
    const uint32_t lo = static_cast<uint32_t>(rot_seed), hi = static_cast<uint32_t>(rot_seed >> 32);
    const uint8_t* in = static_cast<const uint8_t*>(d.in);
    with_float_type(d.dt_out, [&](auto di) {
        constexpr int DT = decltype(di)::value;
        with_quant_bits(d.dt_in, [&](auto bi) {
            constexpr int BITS = decltype(bi)::value;
            if (guarded) {
                if (d.group_size < kGroupedMinG || d.group_size > kGroupedMaxG || (d.group_size & (d.group_size - 1)) != 0)
                    panic("%s: group size %lld", name, static_cast<long long>(d.group_size));
                const dim3 grid(rot_guarded_blocks(ngroups, num_cu));
                if (d.op == OP_ADD) PQ_LAUNCH((dequantize_grouped_rotated_scalar_kernel<DT, BITS, OP_ADD>), grid, dim3(kGroupedRotGuardedBlock), 0, stream, in,
                                              d.out, d.numel, d.group_size, d.scales, d.zero_points, ngroups, lo, hi);
                else PQ_LAUNCH((dequantize_grouped_rotated_scalar_kernel<DT, BITS, OP_SET>), grid, dim3(kGroupedRotGuardedBlock), 0, stream, in, d.out, d.numel,
                               d.group_size, d.scales, d.zero_points, ngroups, lo, hi);
                return;
            }
            with_group_size(d.group_size, name, [&](auto gi) {
                constexpr int G = decltype(gi)::value;
                constexpr int NG = GroupedQuantTile<DT_F32, BITS, G>::NG;
                const dim3 grid(grouped_blocks((ngroups + NG - 1) / NG, name));
                if (d.op == OP_ADD) PQ_LAUNCH((dequantize_grouped_rotated_kernel<DT, BITS, OP_ADD, G>), grid, dim3(kGroupedBlock), 0, stream, in, d.out, d.numel,
                                              d.scales, d.zero_points, ngroups, lo, hi);
                else PQ_LAUNCH((dequantize_grouped_rotated_kernel<DT, BITS, OP_SET, G>), grid, dim3(kGroupedBlock), 0, stream, in, d.out, d.numel, d.scales,
                               d.zero_points, ngroups, lo, hi);
            });
        });
    });
    PQ_HIP(hipGetLastError());
}

}  // namespace pq
