#!/usr/bin/env python3
"""A fixed number of error-feedback calls for a profiler (rocprofv3 --kernel-trace --stats): per iteration ONE quantize_grouped_ef call
(fp32 -> uint8, G = 128, numel 27 264 000), ONE quantize_grouped_ef_batch call of 16 tensors (numel / 16 each) and ONE batched call of the 7
peer chunks of an 8-way mesh.  The trace should show one dispatch of quantize_grouped_ef_batch_kernel per call: 3 per iteration.

    rocprofv3 --kernel-trace --stats -f csv -d out -o grouped_ef -- python tools/grouped_ef_workload.py [--iters 20]
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
    G, n = 128, 27_264_000
    x = torch.empty(n, device="cuda").uniform_(-1, 1)
    r = torch.zeros(n, device="cuda")
    xs16, rs16 = list(x.split(n // 16)), list(r.split(n // 16))
    xs7, rs7 = list(x.split(n // 8))[1:], list(r.split(n // 8))[1:]
    assert len(xs16) == 16 and len(xs7) == 7
    q, s, z = pt.quantize_grouped_ef(x, r, dtype=torch.uint8, group_size=G)
    q16, s16, z16 = pt.quantize_grouped_ef_batch(xs16, rs16, dtype=torch.uint8, group_size=G)
    q7, s7, z7 = pt.quantize_grouped_ef_batch(xs7, rs7, dtype=torch.uint8, group_size=G)
    torch.cuda.synchronize()
    for _ in range(args.iters):
        pt.quantize_grouped_ef(x, r, dtype=torch.uint8, group_size=G, out=q, out_scales=s, out_zero_points=z)
        pt.quantize_grouped_ef_batch(xs16, rs16, dtype=torch.uint8, group_size=G, outs=q16, out_scales=s16, out_zero_points=z16)
        pt.quantize_grouped_ef_batch(xs7, rs7, dtype=torch.uint8, group_size=G, outs=q7, out_scales=s7, out_zero_points=z7)
    torch.cuda.synchronize()
    print(f"{args.iters} iterations: {3 * args.iters} error-feedback calls, {3 * (args.iters + 1)} dispatches expected ({piquant.__name__})")


if __name__ == "__main__":
    main()
