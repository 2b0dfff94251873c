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

--rows wire measures the MX wire's fused calls instead, each next to its composition of public calls in the same run (same protocol; the terms'
records rotate too) and writes profiles/mx_wire_bench.json: reduce_quantize_mx (float32 + 1 / 7 terms -> FP8 and FP4, bfloat16 + 1 / 7 terms -> FP4)
against dequantize_mx ADD per term + quantize_mx, dequantize_sum_mx (float32 = / += 1 / 7 terms in both formats, bfloat16 += 7 FP4 terms) against
dequantize_mx per term, the 7-member quantize batch and the 8-member dequantize batch of numel / 8 against loops of single launches, and the
same-width grouped fused call at G = 32 as comparator.  A row gives fused and composition us, their ratio, the ratio of their algorithmic bytes and
whether fused / composition <= 1.15 x byte ratio ("met" / "missed"), with the windows of both.

    python tools/mx_bench.py --rows wire [--windows 7] [--rotate-gb 3.3] [--out FILE]

--rows ef measures the error-feedback calls the same way and writes profiles/mx_ef_bench.json: quantize_mx_ef {float32, bfloat16} x {FP4, FP8}
against torch.add -> quantize_mx -> dequantize_mx -> torch.sub, the 7-member batch of numel / 8 against 7 single launches of the fused call, and
reduce_quantize_mx_ef (float32 / bfloat16 + 1 / 7 FP4 terms) against a copy of acc, dequantize_mx ADD per term and that composition.  The residuals
rotate like the floats.

    python tools/mx_bench.py --rows ef [--windows 7] [--rotate-gb 3.3] [--out FILE]

--rows fp6 measures quantize_mx, dequantize_mx SET and dequantize_mx ADD in FP6 E2M3 and E3M2 for both float types, each next to the FP4 and the
FP8 call of the same shape in the same run (the four formats in turn, same protocol) and writes profiles/mx_fp6_bench.json: an FP6 row says
whether its time is within 1.15 x the FP8 time x the ratio of their algorithmic bytes ("met" / "missed") and whether it is below the FP8 time.

    python tools/mx_bench.py --rows fp6 [--windows 7] [--rotate-gb 3.3] [--out FILE]

--rows sr measures quantize_mx with stochastic rounding (piquant_hip_quantize_mx_sr) in the four formats for both float types, each next to the
nearest call of the same pair in the same run (nearest window, stochastic window, in turn; same protocol) and writes profiles/mx_sr_bench.json: a
row gives both times, their windows and the ratio stochastic / nearest.  No ratio is fixed in advance.

    python tools/mx_bench.py --rows sr [--windows 7] [--rotate-gb 3.3] [--out FILE]
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


def wire_row(rows, kind, pair, res, fused_bytes, comp_bytes):
    (us_f, s_f), (us_c, s_c) = res["fused"], res["composition"]
    ratio, byte_ratio = us_f / us_c, fused_bytes / comp_bytes
    r = {"kind": kind, "pair": pair, "fused_us": round(us_f, 3), "composition_us": round(us_c, 3), "ratio": round(ratio, 3), "byte_ratio": round(byte_ratio, 3),
         "target": "met" if ratio <= 1.15 * byte_ratio else "missed", "fused_bytes": int(fused_bytes), "composition_bytes": int(comp_bytes),
         "fused_windows_us": [round(v, 3) for v in s_f], "composition_windows_us": [round(v, 3) for v in s_c]}
    if "grouped" in res:
        r["grouped_us"], r["grouped_windows_us"] = round(res["grouped"][0], 3), [round(v, 3) for v in res["grouped"][1]]
    print(f"{kind:20s} {pair:26s} fused {us_f:8.2f} us  composition {us_c:8.2f} us  ratio {ratio:.3f}  bytes {byte_ratio:.3f}  {r['target']}", flush=True)
    rows.append(r)


def wire_main(args):
    """The fused calls of the MX wire against their compositions (module docstring)."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = piquant.Context.get(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    SET, ADD, NEAREST = piquant.ReduceOp.SET, piquant.ReduceOp.ADD, piquant.RoundMode.NEAREST
    ng = pt.num_groups(NUMEL, G)
    rows = []
    reduce_rows = [("f32", "fp8_e4m3", 1), ("f32", "fp8_e4m3", 7), ("f32", "fp4_e2m1", 1), ("f32", "fp4_e2m1", 7), ("bf16", "fp4_e2m1", 1), ("bf16", "fp4_e2m1", 7)]
    sum_rows = [("f32", fmt, op, k) for fmt in WIDTH for op in (SET, ADD) for k in (1, 7)] + [("bf16", "fp4_e2m1", ADD, 7)]
    for fname, (fdt, tdt, esize) in FLOAT.items():
        nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * esize)) + 1)
        per_window = max(nbuf, 16)
        xs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=gen).to(tdt) for _ in range(nbuf)]
        ys = [torch.empty(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
        for fmt, (qname, qdt) in WIDTH.items():
            f, (ncodes, nblocks) = pt.MX_FORMATS[fmt], pt.mx_nbytes(NUMEL, fmt)
            counts = sorted({k for fn, fm, k in reduce_rows if (fn, fm) == (fname, fmt)} | {k for fn, fm, _, k in sum_rows if (fn, fm) == (fname, fmt)})
            if not counts:
                continue
            nset = max(3, int(args.rotate_gb * 1e9 / (max(counts) * ncodes)) + 1)   # term sets: rotated like the floats
            tc = [[torch.empty(ncodes, dtype=torch.uint8, device=dev) for _ in range(max(counts))] for _ in range(nset)]
            ts = [[torch.empty(nblocks, dtype=torch.uint8, device=dev) for _ in range(max(counts))] for _ in range(nset)]
            gs = [[torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(max(counts))] for _ in range(nset)]
            gz = [[torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(max(counts))] for _ in range(nset)]
            for j in range(nset):   # valid records of both wires in the same code buffers' width: MX records for the MX calls, parameters for the grouped
                for t in range(max(counts)):
                    ctx.quantize_mx_ptr(xs[(j + t) % nbuf].data_ptr(), fdt, tc[j][t].data_ptr(), ts[j][t].data_ptr(), NUMEL, f, _device_ptrs=True)
                    gs[j][t].fill_(0.01)
                    gz[j][t].fill_(7)
            oc, os_ = torch.empty(ncodes, dtype=torch.uint8, device=dev), torch.empty(nblocks, dtype=torch.uint8, device=dev)
            osc, ozp = torch.empty(ng, dtype=torch.float32, device=dev), torch.empty(ng, dtype=torch.uint8, device=dev)
            ptrs = lambda bufs, k: [b.data_ptr() for b in bufs[:k]]   # noqa: E731

            def composition_reduce(i, k):
                ys[i % nbuf].copy_(xs[i % nbuf])                      # the composition's copy of acc: acc itself is not written
                for t in range(k):
                    ctx.dequantize_mx_ptr(tc[i % nset][t].data_ptr(), ts[i % nset][t].data_ptr(), ys[i % nbuf].data_ptr(), fdt, NUMEL, f, ADD, _device_ptrs=True)
                ctx.quantize_mx_ptr(ys[i % nbuf].data_ptr(), fdt, oc.data_ptr(), os_.data_ptr(), NUMEL, f, _device_ptrs=True)

            def composition_sum(i, k, op):
                for t in range(k):
                    ctx.dequantize_mx_ptr(tc[i % nset][t].data_ptr(), ts[i % nset][t].data_ptr(), ys[i % nbuf].data_ptr(), fdt, NUMEL, f, op if t == 0 else ADD,
                                          _device_ptrs=True)

            term = ncodes + nblocks
            for k in [k for fn, fm, k in reduce_rows if (fn, fm) == (fname, fmt)]:
                calls = {
                    "fused": lambda i, k=k: ctx.reduce_quantize_mx_ptr(xs[i % nbuf].data_ptr(), fdt, ptrs(tc[i % nset], k), ptrs(ts[i % nset], k), oc.data_ptr(),
                                                                      os_.data_ptr(), NUMEL, f, _device_ptrs=True),
                    "composition": lambda i, k=k: composition_reduce(i, k),
                    "grouped": lambda i, k=k: ctx.reduce_quantize_grouped_ptr(ys[i % nbuf].data_ptr(), fdt, ptrs(tc[i % nset], k), ptrs(gs[i % nset], k),
                                                                            ptrs(gz[i % nset], k), oc.data_ptr(), qdt, NUMEL, G, osc.data_ptr(), ozp.data_ptr(),
                                                                            NEAREST, _device_ptrs=True),
                }
                res = timed_alternating(calls, nbuf * nset, args.windows, per_window, stream)
                fl = NUMEL * esize
                wire_row(rows, "reduce_quantize_mx", f"{fname} + {k} -> {fmt}", res, fl + (k + 1) * term, 2 * fl + k * (term + 2 * fl) + fl + term)
            for op, k in [(op, k) for fn, fm, op, k in sum_rows if (fn, fm) == (fname, fmt)]:
                calls = {
                    "fused": lambda i, k=k, op=op: ctx.dequantize_sum_mx_ptr(ptrs(tc[i % nset], k), ptrs(ts[i % nset], k), ys[i % nbuf].data_ptr(), fdt, NUMEL, f, op,
                                                                             _device_ptrs=True),
                    "composition": lambda i, k=k, op=op: composition_sum(i, k, op),
                    "grouped": lambda i, k=k, op=op: ctx.dequantize_sum_grouped_ptr(ptrs(tc[i % nset], k), qdt, ptrs(gs[i % nset], k), ptrs(gz[i % nset], k),
                                                                                   ys[i % nbuf].data_ptr(), fdt, NUMEL, G, op, _device_ptrs=True),
                }
                res = timed_alternating(calls, nbuf * nset, args.windows, per_window, stream)
                fl, add = NUMEL * esize, op == ADD
                wire_row(rows, "dequantize_sum_mx", f"{fmt} x {k} {'+=' if add else '='} {fname}", res, k * term + (2 if add else 1) * fl,
                         k * term + (2 * k - (0 if add else 1)) * fl)
            if fname == "f32":   # the batches: 7 / 8 members of numel / 8 against loops of single launches
                m = NUMEL // 8
                mc, mb = pt.mx_nbytes(m, fmt)
                stride = -(-mb // 16) * 16                              # every member's scale bytes on a 16-byte boundary, in a buffer of their own
                bsc = torch.empty(8 * stride, dtype=torch.uint8, device=dev)
                cut = lambda t, n, k: [t[j * n:(j + 1) * n] for j in range(k)]   # noqa: E731
                q = {
                    "fused": lambda i: ctx.quantize_mx_batch_ptr(ptrs(cut(xs[i % nbuf], m, 7), 7), fdt, ptrs(cut(tc[i % nset][0], mc, 7), 7),
                                                                 ptrs(cut(bsc, stride, 7), 7), [m] * 7, f, _device_ptrs=True),
                    "composition": lambda i: [ctx.quantize_mx_ptr(x.data_ptr(), fdt, c.data_ptr(), sc.data_ptr(), m, f, _device_ptrs=True)
                                              for x, c, sc in zip(cut(xs[i % nbuf], m, 7), cut(tc[i % nset][0], mc, 7), cut(bsc, stride, 7))],
                }
                res = timed_alternating(q, nbuf * nset, args.windows, per_window, stream)
                wire_row(rows, "quantize_mx_batch", f"7 x {fname} -> {fmt}", res, 7 * (m * esize + mc + mb), 7 * (m * esize + mc + mb))
                d = {
                    "fused": lambda i: ctx.dequantize_mx_batch_ptr(ptrs(cut(tc[i % nset][0], mc, 8), 8), ptrs(cut(bsc, stride, 8), 8),
                                                                   ptrs(cut(ys[i % nbuf], m, 8), 8), fdt, [m] * 8, f, SET, _device_ptrs=True),
                    "composition": lambda i: [ctx.dequantize_mx_ptr(c.data_ptr(), sc.data_ptr(), y.data_ptr(), fdt, m, f, SET, _device_ptrs=True)
                                              for c, sc, y in zip(cut(tc[i % nset][0], mc, 8), cut(bsc, stride, 8), cut(ys[i % nbuf], m, 8))],
                }
                res = timed_alternating(d, nbuf * nset, args.windows, per_window, stream)
                wire_row(rows, "dequantize_mx_batch", f"8 x {fmt} -> {fname}", res, 8 * (m * esize + mc + mb), 8 * (m * esize + mc + mb))
            del tc, ts, gs, gz
        del xs, ys
        torch.cuda.empty_cache()
    out = {"numel": NUMEL, "device": torch.cuda.get_device_name(0), "windows": args.windows, "rotate_gb": args.rotate_gb, "group_size": G,
           "command": "python tools/mx_bench.py --rows wire",
           "protocol": "alternating windows of back-to-back calls, HIP events, median over windows; rotated float buffers and term sets; target: fused / "
                       "composition <= 1.15 x byte ratio",
           "not_measured": "other sizes, the guarded kernels, more than one GPU", "rows": rows}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


def ef_main(args):
    """The error-feedback calls of the MX wire against their compositions of public calls (module docstring)."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = piquant.Context.get(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    SET, ADD, F32 = piquant.ReduceOp.SET, piquant.ReduceOp.ADD, piquant.DataType.F32
    rows = []
    reduce_rows = [("f32", "fp4_e2m1"), ("bf16", "fp4_e2m1")]
    nres = max(3, int(args.rotate_gb * 1e9 / (NUMEL * 4)) + 1)
    rs = [torch.empty(NUMEL, device=dev).uniform_(-0.1, 0.1, generator=gen) for _ in range(nres)]   # the residuals, and the composition's y and d
    ys = [torch.empty(NUMEL, device=dev) for _ in range(nres)]
    ds = [torch.empty(NUMEL, device=dev) for _ in range(nres)]
    for fname, (fdt, tdt, esize) in FLOAT.items():
        nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * esize)) + 1)
        per_window = max(nbuf, 16)
        xs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=gen).to(tdt) for _ in range(nbuf)]
        accs = [torch.empty(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]                       # the reduce composition's copy of acc
        for fmt in WIDTH:
            f, (ncodes, nblocks) = pt.MX_FORMATS[fmt], pt.mx_nbytes(NUMEL, fmt)
            oc, os_ = torch.empty(ncodes, dtype=torch.uint8, device=dev), torch.empty(nblocks, dtype=torch.uint8, device=dev)
            fl, term = NUMEL * esize, ncodes + nblocks
            comp_bytes = (fl + 8 * NUMEL) + (4 * NUMEL + term) + (term + 4 * NUMEL) + 12 * NUMEL   # add, quantize_mx, dequantize_mx, sub

            def composition(i, x, n=NUMEL, r=None, c=oc, s=os_):
                r = rs[i % nres] if r is None else r
                y, d = ys[i % nres][:n], ds[i % nres][:n]
                torch.add(x, r, out=y)
                ctx.quantize_mx_ptr(y.data_ptr(), F32, c.data_ptr(), s.data_ptr(), n, f, _device_ptrs=True)
                ctx.dequantize_mx_ptr(c.data_ptr(), s.data_ptr(), d.data_ptr(), F32, n, f, SET, _device_ptrs=True)
                torch.sub(y, d, out=r)

            calls = {
                "fused": lambda i: ctx.quantize_mx_ef_ptr(xs[i % nbuf].data_ptr(), fdt, rs[i % nres].data_ptr(), oc.data_ptr(), os_.data_ptr(), NUMEL, f,
                                                          _device_ptrs=True),
                "composition": lambda i: composition(i, xs[i % nbuf]),
            }
            res = timed_alternating(calls, nbuf * nres, args.windows, per_window, stream)
            wire_row(rows, "quantize_mx_ef", f"{fname} -> {fmt}", res, fl + 8 * NUMEL + term, comp_bytes)
            if fname == "f32":   # the batch: 7 members of numel / 8 against 7 single launches of the fused call
                m = NUMEL // 8
                mc, mb = pt.mx_nbytes(m, fmt)
                stride = -(-mb // 16) * 16
                bsc = torch.empty(7 * stride, dtype=torch.uint8, device=dev)
                cut = lambda t, n: [t[j * n:(j + 1) * n] for j in range(7)]   # noqa: E731
                ptrs = lambda ts: [t.data_ptr() for t in ts]                  # noqa: E731
                q = {
                    "fused": lambda i: ctx.quantize_mx_ef_batch_ptr(ptrs(cut(xs[i % nbuf], m)), fdt, ptrs(cut(rs[i % nres], m)), ptrs(cut(oc, mc)),
                                                                    ptrs(cut(bsc, stride)), [m] * 7, f, _device_ptrs=True),
                    "composition": lambda i: [ctx.quantize_mx_ef_ptr(x.data_ptr(), fdt, r.data_ptr(), c.data_ptr(), s.data_ptr(), m, f, _device_ptrs=True)
                                              for x, r, c, s in zip(cut(xs[i % nbuf], m), cut(rs[i % nres], m), cut(oc, mc), cut(bsc, stride))],
                }
                res = timed_alternating(q, nbuf * nres, args.windows, per_window, stream)
                wire_row(rows, "quantize_mx_ef_batch", f"7 x {fname} -> {fmt}", res, 7 * (m * esize + 8 * m + mc + mb), 7 * (m * esize + 8 * m + mc + mb))
            if (fname, fmt) in reduce_rows:
                nset = max(3, int(args.rotate_gb * 1e9 / (7 * ncodes)) + 1)
                tc = [[torch.empty(ncodes, dtype=torch.uint8, device=dev) for _ in range(7)] for _ in range(nset)]
                ts = [[torch.empty(nblocks, dtype=torch.uint8, device=dev) for _ in range(7)] for _ in range(nset)]
                for j in range(nset):
                    for t in range(7):
                        ctx.quantize_mx_ptr(xs[(j + t) % nbuf].data_ptr(), fdt, tc[j][t].data_ptr(), ts[j][t].data_ptr(), NUMEL, f, _device_ptrs=True)

                def composition_reduce(i, k):
                    acc = accs[i % nbuf]
                    acc.copy_(xs[i % nbuf])                             # the composition's copy of acc: acc itself is not written
                    for t in range(k):
                        ctx.dequantize_mx_ptr(tc[i % nset][t].data_ptr(), ts[i % nset][t].data_ptr(), acc.data_ptr(), fdt, NUMEL, f, ADD, _device_ptrs=True)
                    composition(i, acc)

                for k in (1, 7):
                    calls = {
                        "fused": lambda i, k=k: ctx.reduce_quantize_mx_ef_ptr(xs[i % nbuf].data_ptr(), fdt, rs[i % nres].data_ptr(),
                                                                             [c.data_ptr() for c in tc[i % nset][:k]], [s.data_ptr() for s in ts[i % nset][:k]],
                                                                             oc.data_ptr(), os_.data_ptr(), NUMEL, f, _device_ptrs=True),
                        "composition": lambda i, k=k: composition_reduce(i, k),
                    }
                    res = timed_alternating(calls, nbuf * nres * nset, args.windows, per_window, stream)
                    wire_row(rows, "reduce_quantize_mx_ef", f"{fname} + {k} -> {fmt}", res, fl + k * term + 8 * NUMEL + term,
                             2 * fl + k * (term + 2 * fl) + comp_bytes)
                del tc, ts
        del xs, accs
        torch.cuda.empty_cache()
    out = {"numel": NUMEL, "device": torch.cuda.get_device_name(0), "windows": args.windows, "rotate_gb": args.rotate_gb,
           "command": "python tools/mx_bench.py --rows ef",
           "protocol": "alternating windows of back-to-back calls, HIP events, median over windows; rotated float buffers, residuals and term sets; "
                       "composition: torch.add -> quantize_mx -> dequantize_mx -> torch.sub (the reduce: a copy of acc and dequantize_mx ADD per term in "
                       "front); target: fused / composition <= 1.15 x byte ratio",
           "spread": "run-to-run spread not measured (one run); every row carries the windows of both sides",
           "not_measured": "other sizes, the guarded kernels, more than one GPU", "rows": rows}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


def fp6_main(args):
    """quantize_mx and dequantize_mx (SET and ADD) in the two FP6 formats next to the FP4 and FP8 calls of the same shape (module docstring)."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = piquant.Context.get(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    SET, ADD = piquant.ReduceOp.SET, piquant.ReduceOp.ADD
    fmts = ("fp4_e2m1", "fp6_e2m3", "fp6_e3m2", "fp8_e4m3")
    nblocks = pt.mx_nbytes(NUMEL, "fp8_e4m3")[1]
    rows = []
    for fname, (fdt, tdt, esize) in FLOAT.items():
        nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * esize)) + 1)
        per_window = max(2 * nbuf, 32)
        xs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=gen).to(tdt) for _ in range(nbuf)]
        ys = [torch.zeros(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
        codes = {fmt: [torch.empty(pt.mx_nbytes(NUMEL, fmt)[0], dtype=torch.uint8, device=dev) for _ in range(nbuf)] for fmt in fmts}
        mxs = {fmt: [torch.empty(nblocks, dtype=torch.uint8, device=dev) for _ in range(nbuf)] for fmt in fmts}
        quant = {fmt: (lambda i, fmt=fmt: ctx.quantize_mx_ptr(xs[i].data_ptr(), fdt, codes[fmt][i].data_ptr(), mxs[fmt][i].data_ptr(), NUMEL, pt.MX_FORMATS[fmt],
                                                              _device_ptrs=True)) for fmt in fmts}
        results = [("quantize_mx", 1, timed_alternating(quant, nbuf, args.windows, per_window, stream))]
        for name, op, passes in (("dequantize_mx SET", SET, 1), ("dequantize_mx ADD", ADD, 2)):   # the codes quantize_mx left; ADD reads and writes the floats
            dequant = {fmt: (lambda i, fmt=fmt, op=op: ctx.dequantize_mx_ptr(codes[fmt][i].data_ptr(), mxs[fmt][i].data_ptr(), ys[i].data_ptr(), fdt, NUMEL,
                                                                              pt.MX_FORMATS[fmt], op, _device_ptrs=True)) for fmt in fmts}
            results.append((name, passes, timed_alternating(dequant, nbuf, args.windows, per_window, stream)))
        for kind, passes, res in results:
            nbytes = {fmt: passes * NUMEL * esize + pt.mx_nbytes(NUMEL, fmt)[0] + nblocks for fmt in fmts}
            for fmt in ("fp4_e2m1", "fp8_e4m3"):
                rows.append(row(kind, f"{fname} {fmt}", res[fmt][0], nbytes[fmt], res[fmt][1]))
            for fmt in ("fp6_e2m3", "fp6_e3m2"):
                r = row(kind, f"{fname} {fmt}", res[fmt][0], nbytes[fmt], res[fmt][1])
                r["over_fp8"], r["byte_ratio"] = round(res[fmt][0] / res["fp8_e4m3"][0], 3), round(nbytes[fmt] / nbytes["fp8_e4m3"], 3)
                r["target"] = "met" if res[fmt][0] <= 1.15 * res["fp8_e4m3"][0] * nbytes[fmt] / nbytes["fp8_e4m3"] else "missed"
                r["faster_than_fp8"] = bool(res[fmt][0] < res["fp8_e4m3"][0])
                print(f"    FP6 / FP8 = {r['over_fp8']:.3f}, bytes {r['byte_ratio']:.3f}: {r['target']}", flush=True)
                rows.append(r)
        del xs, ys, codes, mxs
        torch.cuda.empty_cache()
    out = {"numel": NUMEL, "device": torch.cuda.get_device_name(0), "windows": args.windows, "rotate_gb": args.rotate_gb,
           "command": "python tools/mx_bench.py --rows fp6",
           "protocol": "alternating windows of back-to-back calls (FP4, E2M3, E3M2, FP8 in turn), HIP events, median over windows; rotated float and code "
                       "buffers; target: FP6 us <= 1.15 x FP8 us x FP6 bytes / FP8 bytes",
           "spread": "run-to-run spread not measured (one run); every row carries its windows",
           "not_measured": "other sizes, the guarded kernels, past 2^31 elements", "rows": rows}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


def sr_main(args):
    """quantize_mx with stochastic rounding next to the nearest call of the same pair (module docstring)."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = piquant.Context.get(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    nblocks = pt.mx_nbytes(NUMEL, "fp8_e4m3")[1]
    rows = []
    for fname, (fdt, tdt, esize) in FLOAT.items():
        nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * esize)) + 1)
        per_window = max(2 * nbuf, 32)
        xs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=gen).to(tdt) for _ in range(nbuf)]
        mxs = [torch.empty(nblocks, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        for fmt, f in pt.MX_FORMATS.items():
            ncodes = pt.mx_nbytes(NUMEL, fmt)[0]
            codes = [torch.empty(ncodes, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            calls = {
                "nearest": lambda i: ctx.quantize_mx_ptr(xs[i].data_ptr(), fdt, codes[i].data_ptr(), mxs[i].data_ptr(), NUMEL, f, _device_ptrs=True),
                "stochastic": lambda i: ctx.quantize_mx_sr_ptr(xs[i].data_ptr(), fdt, codes[i].data_ptr(), mxs[i].data_ptr(), NUMEL, f, 0x9E3779B97F4A7C15,
                                                               1 << 40, _device_ptrs=True),
            }
            res = timed_alternating(calls, nbuf, args.windows, per_window, stream)
            nbytes = NUMEL * esize + ncodes + nblocks
            rows.append(row("quantize_mx", f"{fname} {fmt}", res["nearest"][0], nbytes, res["nearest"][1]))
            r = row("quantize_mx_sr", f"{fname} {fmt}", res["stochastic"][0], nbytes, res["stochastic"][1])
            r["nearest_us"], r["over_nearest"] = round(res["nearest"][0], 3), round(res["stochastic"][0] / res["nearest"][0], 3)
            print(f"    stochastic / nearest = {r['over_nearest']:.3f}", flush=True)
            rows.append(r)
            del codes
        del xs, mxs
        torch.cuda.empty_cache()
    out = {"numel": NUMEL, "device": torch.cuda.get_device_name(0), "windows": args.windows, "rotate_gb": args.rotate_gb,
           "command": "python tools/mx_bench.py --rows sr",
           "protocol": "alternating windows of back-to-back calls (nearest, stochastic in turn), HIP events, median over windows; rotated float and code "
                       "buffers; no target ratio",
           "spread": "run-to-run spread not measured (one run); every row carries its windows",
           "not_measured": "other sizes, the guarded kernels, the batch", "rows": rows}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=("calls", "wire", "ef", "fp6", "sr"), default="calls")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rotate-gb", type=float, default=3.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / {"calls": "mx_bench.json", "wire": "mx_wire_bench.json", "ef": "mx_ef_bench.json", "fp6": "mx_fp6_bench.json",
                                                  "sr": "mx_sr_bench.json"}[args.rows])
    if args.rows == "sr":
        return sr_main(args)
    if args.rows == "fp6":
        return fp6_main(args)
    if args.rows == "wire":
        return wire_main(args)
    if args.rows == "ef":
        return ef_main(args)
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
