#!/usr/bin/env python3
"""A fixed number of batched rotated calls and of the loops of single calls they replace, for a profiler (rocprofv3 --kernel-trace --stats): the
cases of `tools/grouped_bench.py --rows rot_batch` (G = 128; fp32 -> uint8 and bf16 -> uint4: the 7 peer chunks of an 8-way mesh quantized, and
quantized with error feedback, its 8 chunks dequantized; cold rotating buffers), per iteration ONE batched call and ONE loop of single calls of
each, and one rank's 8-way rotated mesh (fp32 -> uint4) once through piquant.distributed._DeviceOps and once through the loops.  The trace should
show one dispatch of a *_batch_kernel per batched call, and 7 (8) dispatches of the single-tensor kernel per loop.

    rocprofv3 --kernel-trace --stats -f csv -d out -o grouped_rot_batch -- python tools/grouped_rot_batch_workload.py [--iters 20]

`tools/grouped_bench.py --rows rot_batch --kernel-stats out/.../grouped_rot_batch_kernel_stats.csv` puts the sums of the kernel times next to its
stream times.
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import grouped_bench as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rotate-gb", type=float, default=3.3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    ctx = B.piquant.Context.get(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    ctx.assume_device_pointers(True)
    calls = 0
    for kind, pair, m, nbuf, nbytes, batch, loop in B.rot_batch_cases(ctx, dev, args.rotate_gb):
        for i in range(args.iters):
            batch(i % nbuf)
            loop((i + nbuf // 2) % nbuf)
        torch.cuda.synchronize()
        calls += args.iters
        print(f"{kind} {pair}: {args.iters} batches of {m} and {args.iters} loops of {m} single calls", flush=True)
    meshes = B.rot_batch_mesh(ctx, dev)
    for _ in range(args.iters):
        meshes["batched"]()
        meshes["loop"]()
    torch.cuda.synchronize()
    print(f"{calls} batched calls, as many loops, and {args.iters} rotated meshes each way")


if __name__ == "__main__":
    main()
