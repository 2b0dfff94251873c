#!/usr/bin/env python3
"""A fixed number of fused reduce + error-feedback calls of a bfloat16 accumulator with a FLOAT32 residual for a profiler
(rocprofv3 --kernel-trace --stats): per iteration ONE reduce_quantize_grouped_ef call with 1 term, ONE with 7 terms (the owner's step of an 8-way
mesh) and ONE with 0 terms (bf16 acc, float32 residual, uint8 terms, G = 128, numel 27 264 000 / 8).  The trace should show one dispatch of
reduce_quantize_grouped_ef_f32r_kernel per call with terms -- 2 per iteration -- and one of quantize_grouped_ef_f32r_kernel for the call without,
and no dequantize_grouped_kernel at all.

    rocprofv3 --kernel-trace --stats -f csv -d out -o grouped_reduce_ef_f32r -- python tools/grouped_reduce_ef_f32r_workload.py [--iters 20]
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
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    G, n = 128, 27_264_000 // 8
    acc = torch.empty(n, device="cuda").uniform_(-1, 1).to(torch.bfloat16)
    r = torch.zeros(n, dtype=torch.float32, device="cuda")
    terms = [pt.quantize_grouped(torch.empty(n, device="cuda").uniform_(-1, 1).to(torch.bfloat16), dtype=torch.uint8, group_size=G) for _ in range(7)]
    qs, ss, zs = [t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms]
    q, s, z = pt.reduce_quantize_grouped_ef(acc, r, qs[:1], ss[:1], zs[:1], dtype=torch.uint8, group_size=G)
    torch.cuda.synchronize()
    for _ in range(args.iters):
        for k in (1, 7, 0):
            pt.reduce_quantize_grouped_ef(acc, r, qs[:k], ss[:k], zs[:k], dtype=torch.uint8, group_size=G, out=q, out_scales=s, out_zero_points=z)
    torch.cuda.synchronize()
    print(f"{args.iters} iterations: {3 * args.iters} calls, {2 * args.iters + 1} dispatches of reduce_quantize_grouped_ef_f32r_kernel and {args.iters} of "
          f"quantize_grouped_ef_f32r_kernel expected ({piquant.__name__})")


if __name__ == "__main__":
    main()
