#!/usr/bin/env python3
"""The MX block-format calls at the headline size (numel 27 264 000), each next to the grouped call of the same width at G = 32 and the uniform call
of that width, in the same run with alternating windows.

Protocol (tools/grouped_bench.py's): float buffers rotated over >= 3.3 GB so that no call finds its input in the 256 MiB Infinity Cache, HIP events
around windows of back-to-back calls, the median over the windows.  One round times a window of the MX call, then of the grouped call, then of the
uniform call; the rounds repeat.  Rows: quantize_mx {float32, bfloat16} x {FP4, FP8} against quantize_grouped -> uint4 / uint8 (G = 32) and
quantize_uniform; dequantize_mx SET likewise.  Each row gives us per call, the algorithmic bytes (fp32 -> FP4: 4 + 1/2 + 1/32 per element; grouped:
5 parameter bytes per group) and the share of 8 TB/s; an MX row also says whether it took no longer than its grouped comparator plus that
comparator's own spread (max - min over its windows).  Writes profiles/mx_bench.json.

    python tools/mx_bench.py [--windows 7] [--rotate-gb 3.3] [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pi-quant_amd"))

import piquant  # noqa: E402
import piquant.torch as pt  # noqa: E402

NUMEL = 27_264_000
HBM_PEAK_TBS = 8.0
G = 32
FLOAT = {"f32": (piquant.DataType.F32, torch.float32, 4), "bf16": (piquant.DataType.BF16, torch.bfloat16, 2)}
WIDTH = {"fp4_e2m1": ("uint4", piquant.DataType.UINT4), "fp8_e4m3": ("uint8", piquant.DataType.UINT8)}


def timed_alternating(calls, nbuf, windows, per_window, stream):
    """{name: (median us per call, samples)}: every round times one window of each call in turn, buffer i % nbuf for call i"""
    for call in calls.values():
        for i in range(min(nbuf, 8)):
            call(i)
    torch.cuda.synchronize()
    samples, k = {name: [] for name in calls}, 0
    for _ in range(windows):
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(per_window):
                call(k % nbuf)
                k += 1
            b.record(stream)
            b.synchronize()
            samples[name].append(a.elapsed_time(b) * 1000.0 / per_window)
    return {name: (statistics.median(s), s) for name, s in samples.items()}


def row(kind, pair, us, nbytes, samples):
    r = {"kind": kind, "pair": pair, "us": round(us, 3), "bytes": int(nbytes), "tb_s": round(nbytes / us / 1e6, 3),
         "frac_8tbs": round(nbytes / us / 1e6 / HBM_PEAK_TBS, 4), "windows_us": [round(s, 3) for s in samples]}
    print(f"{kind:20s} {pair:18s} {us:8.2f} us  {nbytes / 1e6:8.1f} MB  {r['frac_8tbs']:.3f} of 8 TB/s", flush=True)
    return r


def judge(rows, res, mx_row, comparator):
    us_c, s_c = res[comparator]
    mx_row["over_grouped"] = round(mx_row["us"] / us_c, 3)
    mx_row["grouped_spread_us"] = round(max(s_c) - min(s_c), 3)
    mx_row["no_longer_than_grouped"] = bool(mx_row["us"] <= us_c + (max(s_c) - min(s_c)))
    print(f"    MX / grouped = {mx_row['over_grouped']:.3f}: {'met' if mx_row['no_longer_than_grouped'] else 'MISSED'}", flush=True)
    rows.append(mx_row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rotate-gb", type=float, default=3.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mx_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = piquant.Context.get(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    ng, nblocks = pt.num_groups(NUMEL, G), pt.mx_nbytes(NUMEL, "fp8_e4m3")[1]
    rows = []
    for fname, (fdt, tdt, esize) in FLOAT.items():
        nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * esize)) + 1)
        per_window = max(2 * nbuf, 32)
        xs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=gen).to(tdt) for _ in range(nbuf)]
        ys = [torch.empty(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
        for fmt, (qname, qdt) in WIDTH.items():
            f, ncodes = pt.MX_FORMATS[fmt], pt.mx_nbytes(NUMEL, fmt)[0]
            codes = [torch.empty(ncodes, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            mxs = [torch.empty(nblocks, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
            zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            quant = {
                "mx": lambda i: ctx.quantize_mx_ptr(xs[i].data_ptr(), fdt, codes[i].data_ptr(), mxs[i].data_ptr(), NUMEL, f, _device_ptrs=True),
                "grouped": lambda i: ctx.quantize_grouped_ptr(xs[i].data_ptr(), fdt, codes[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                                              piquant.RoundMode.NEAREST, _device_ptrs=True),
                "uniform": lambda i: ctx.quantize_ptr(xs[i].data_ptr(), fdt, codes[i].data_ptr(), qdt, NUMEL, 0.01, 7, piquant.RoundMode.NEAREST, _device_ptrs=True,
                                                      uniform=True),
            }
            res = timed_alternating(quant, nbuf, args.windows, per_window, stream)
            base = NUMEL * esize + ncodes
            rows.append(row("quantize_grouped", f"{fname}->{qname} G=32", *res["grouped"][:1], base + 5 * ng, res["grouped"][1]))
            rows.append(row("quantize_uniform", f"{fname}->{qname}", *res["uniform"][:1], base, res["uniform"][1]))
            judge(rows, res, row("quantize_mx", f"{fname}->{fmt}", res["mx"][0], base + nblocks, res["mx"][1]), "grouped")
            # dequantize SET: the codes quantize_mx left (valid MX bytes), and for the comparators the parameters quantize_grouped left
            dequant = {
                "mx": lambda i: ctx.dequantize_mx_ptr(codes[i].data_ptr(), mxs[i].data_ptr(), ys[i].data_ptr(), fdt, NUMEL, f, piquant.ReduceOp.SET, _device_ptrs=True),
                "grouped": lambda i: ctx.dequantize_grouped_ptr(codes[i].data_ptr(), qdt, ys[i].data_ptr(), fdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                                                piquant.ReduceOp.SET, _device_ptrs=True),
                "uniform": lambda i: ctx.dequantize_ptr(codes[i].data_ptr(), qdt, ys[i].data_ptr(), fdt, NUMEL, 0.01, 7, piquant.ReduceOp.SET, _device_ptrs=True,
                                                        uniform=True),
            }
            res = timed_alternating(dequant, nbuf, args.windows, per_window, stream)
            rows.append(row("dequantize_grouped", f"{qname}->{fname} G=32", *res["grouped"][:1], base + 5 * ng, res["grouped"][1]))
            rows.append(row("dequantize_uniform", f"{qname}->{fname}", *res["uniform"][:1], base, res["uniform"][1]))
            judge(rows, res, row("dequantize_mx", f"{fmt}->{fname}", res["mx"][0], base + nblocks, res["mx"][1]), "grouped")
            del codes, mxs, sc, zs
        del xs, ys
        torch.cuda.empty_cache()
    out = {"numel": NUMEL, "device": torch.cuda.get_device_name(0), "windows": args.windows, "rotate_gb": args.rotate_gb, "group_size": G,
           "protocol": "alternating windows of back-to-back calls, HIP events, median over windows; rotated float buffers", "rows": rows}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
