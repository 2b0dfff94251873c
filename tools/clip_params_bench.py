#!/usr/bin/env python3
"""The histogram clip search for per-tensor parameters at the headline size (numel 27 264 000), next to the plain scan of the same run.

Protocol (tools/grouped_bench.py's): input buffers rotated over >= 3.3 GB (no call finds its input in the 256 MiB Infinity Cache), HIP events
around windows of back-to-back calls, the median of several windows.  For float32 and bfloat16 input, in ONE run:
  scan                  compute_quant_params_device: the parent's path, reading the same bytes -- the reference point of every ratio here
  histogram             clip_histogram alone (streaming pass + fold) against keys computed once
  search                quant_params_from_histogram alone (63 candidates, uint4)
  clipped               compute_quant_params_clipped_device: scan + histogram + search
  clipped+quantize_dp   the whole call followed by quantize_dp (uint4)
  quantize_dynamic      the one-call min/max path of the same pair, next to it
Data: N(0,1), and the adverse input -- everything but the two extremes in ONE bin, i.e. every lane of every LDS add on one address.
Reports histogram / scan per row.  Writes profiles/clip_params_bench.json.

    python tools/clip_params_bench.py [--windows 7] [--rotate-gb 3.3] [--out FILE]
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
STEPS = 63
FLOAT = {"f32": (piquant.DataType.F32, torch.float32, 4), "bf16": (piquant.DataType.BF16, torch.bfloat16, 2)}


def timed(call, nbuf, windows, per_window, stream):
    """median us per call over `windows` windows of `per_window` calls, buffer i % nbuf for call i"""
    for i in range(min(nbuf, 8)):
        call(i)
    torch.cuda.synchronize()
    res, k = [], 0
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(per_window):
            call(k % nbuf)
            k += 1
        b.record(stream)
        b.synchronize()
        res.append(a.elapsed_time(b) * 1000.0 / per_window)
    return statistics.median(res), res


def inputs(name, data, nbuf, dev):
    _, tdt, _ = FLOAT[name]
    g = torch.Generator(device=dev).manual_seed(1)
    xs = []
    for _ in range(nbuf):
        if data == "gaussian":
            x = torch.randn(NUMEL, generator=g, device=dev, dtype=torch.float32)
        else:   # one bin: the bulk at 0.5, the extremes -1 and 3 once each
            x = torch.full((NUMEL,), 0.5, device=dev, dtype=torch.float32)
            x[0], x[-1] = -1.0, 3.0
        xs.append(x.to(tdt))
    return xs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--per-window", type=int, default=40)
    ap.add_argument("--rotate-gb", type=float, default=3.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip_params_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = piquant.Context.get(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    qdt, tq = piquant.DataType.UINT4, torch.quint4x2
    rows = []
    for name, (fdt, tdt, esize) in FLOAT.items():
        nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * esize)) + 1)
        for data in ("gaussian", "one_bin"):
            xs = inputs(name, data, nbuf, dev)
            params = torch.empty(16, dtype=torch.uint8, device=dev)
            keys = torch.empty(2, dtype=torch.int32, device=dev)
            hist = torch.empty(pt.CLIP_BINS, dtype=torch.int64, device=dev)
            out = torch.empty(NUMEL // 2, dtype=torch.uint8, device=dev)
            ctx.minmax_keys_ptr(xs[0].data_ptr(), fdt, NUMEL, keys.data_ptr(), init=True, _device_ptrs=True)
            ctx.clip_histogram_ptr(xs[0].data_ptr(), fdt, NUMEL, keys.data_ptr(), hist.data_ptr(), init=True, _device_ptrs=True)
            torch.cuda.synchronize()
            calls = {
                "scan": lambda i: ctx.compute_quant_params_device_ptr(xs[i].data_ptr(), fdt, NUMEL, qdt, params.data_ptr(), _device_ptrs=True),
                "histogram": lambda i: ctx.clip_histogram_ptr(xs[i].data_ptr(), fdt, NUMEL, keys.data_ptr(), hist.data_ptr(), init=True, _device_ptrs=True),
                "search": lambda i: ctx.quant_params_from_histogram_ptr(keys.data_ptr(), hist.data_ptr(), qdt, STEPS, params.data_ptr()),
                "clipped": lambda i: ctx.compute_quant_params_clipped_device_ptr(xs[i].data_ptr(), fdt, NUMEL, qdt, STEPS, params.data_ptr(), _device_ptrs=True),
            }

            def clipped_quantize(i):
                calls["clipped"](i)
                ctx.quantize_dp_ptr(xs[i].data_ptr(), fdt, out.data_ptr(), qdt, NUMEL, params.data_ptr(), piquant.RoundMode.NEAREST, _device_ptrs=True)

            calls["clipped+quantize_dp"] = clipped_quantize
            calls["quantize_dynamic"] = lambda i: ctx.quantize_dynamic_ptr(xs[i].data_ptr(), fdt, out.data_ptr(), qdt, NUMEL, params.data_ptr(),
                                                                         piquant.RoundMode.NEAREST, _device_ptrs=True)
            us = {}
            for kind, call in calls.items():
                med, samples = timed(call, nbuf, args.windows, args.per_window, stream)
                us[kind] = med
                rows.append({"kind": kind, "input": name, "data": data, "us": round(med, 3), "windows_us": [round(s, 3) for s in samples]})
                print(f"{name:5s} {data:9s} {kind:20s} {med:8.2f} us", flush=True)
            ratio = us["histogram"] / us["scan"]
            rows.append({"kind": "histogram / scan", "input": name, "data": data, "ratio": round(ratio, 3),
                         "clipped / scan": round(us["clipped"] / us["scan"], 3)})
            print(f"{name:5s} {data:9s} histogram / scan = {ratio:.3f}, clipped / scan = {us['clipped'] / us['scan']:.3f}", flush=True)
            del xs
            torch.cuda.empty_cache()
    props = torch.cuda.get_device_properties(0)
    doc = {"numel": NUMEL, "steps": STEPS, "wire": "uint4", "device": props.name, "compute_units": props.multi_processor_count,
           "protocol": f"cold rotating inputs over {args.rotate_gb} GB, HIP events around windows of {args.per_window} calls, median of {args.windows}",
           "rows": rows}
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
