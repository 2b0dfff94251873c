#!/usr/bin/env python3
"""A fixed number of grouped mesh steps for a profiler (rocprofv3 --kernel-trace --stats): per iteration ONE fused reduce_quantize_grouped call
(fp32 acc, 7 uint8 terms, G = 128, numel 27 264 000 / 8), ONE batched grouped quantize of 7 chunks and ONE batched grouped dequantize of 8 chunks.
The trace should show one dispatch per call.

    rocprofv3 --kernel-trace --stats -f csv -d out -o grouped -- python tools/grouped_reduce_workload.py [--iters 50]
"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pi-quant_amd"))

import piquant  # noqa: E402
import piquant.torch as pt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    G, world, per = 128, 8, 27_264_000 // 8
    xs = [torch.empty(per, device="cuda").uniform_(-1, 1) for _ in range(world)]
    qs, ss, zs = pt.quantize_grouped_batch(xs[1:], dtype=torch.uint8, group_size=G)
    ys = [torch.empty(per, device="cuda") for _ in range(world)]
    all_q, all_s, all_z = [qs[0]] + qs, [ss[0]] + ss, [zs[0]] + zs
    torch.cuda.synchronize()
    for _ in range(args.iters):
        pt.quantize_grouped_batch(xs[1:], dtype=torch.uint8, group_size=G, outs=qs)
        out, s, z = pt.reduce_quantize_grouped(xs[0], qs, ss, zs, dtype=torch.uint8, group_size=G)
        pt.dequantize_grouped_batch(all_q, all_s, all_z, dtype=torch.float32, group_size=G, outs=ys)
    torch.cuda.synchronize()
    print(f"{args.iters} iterations: {3 * args.iters} grouped calls ({piquant.__name__})")


if __name__ == "__main__":
    main()
