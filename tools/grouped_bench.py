#!/usr/bin/env python3
"""Group-wise quantization at the headline size (numel 27 264 000), next to the per-tensor calls of the same pairs.

Protocol of the headline numbers: input buffers rotated over >= 3.3 GB (no call finds its input in the 256 MiB Infinity Cache), HIP events around
windows of back-to-back calls, the median of several windows.  Rows: every quantize pair at G in {32, 128, 1024, 4096} against quantize_uniform and
against scan + quantize (compute_quant_params_device -> quantize_dp, two launches); every dequantize pair at G = 128 against dequantize_uniform.
Each row gives us per call, algorithmic bytes (the 5 bytes per group included) and the fraction of 8 TB/s.  Writes profiles/grouped_bench.json.

--rows reduce: the fused reduce_quantize_grouped (fp32 acc, uint8 and uint4 terms, k = 1 and k = 7, G = 128) next to its two-step composition
(k grouped dequantize ADD launches + quantize_grouped) in the same run, and the batched grouped quantize (7 chunks) / dequantize (8 chunks) of
an 8-way mesh next to as many single calls.  Writes profiles/grouped_reduce_bench.json.

--rows ef: the error-feedback quantize (quantize_grouped_ef, G = 128, every pair) next to the four launches it replaces (torch.add ->
quantize_grouped -> dequantize_grouped -> torch.sub), to quantize_grouped alone and to torch.add / torch.sub alone, all in the same run; a batch
of one next to the single quantize_grouped call (the error-feedback single call is a batch of one); and the kernel time of one rank's replayed
8-way grouped mesh all-reduce with and without error feedback.  Writes profiles/grouped_ef_bench.json.

--rows reduce_ef: the fused reduce_quantize_grouped_ef (fp32 acc with uint8 and uint4 terms, k = 1 and k = 7; bf16 acc with uint4 terms, k = 1;
G = 128) next to the two-step composition that defines it (k grouped dequantize ADD launches + quantize_grouped_ef) in the same run, with the
byte ratio of each row and the target fused / composition <= 1.15 x that ratio; and the kernel time of one rank's replayed 8-way grouped mesh
all-reduce with error feedback, with error_feedback_requantize off and on.  Writes profiles/grouped_reduce_ef_bench.json.

--rows ef_f32r: the error-feedback quantize of a bfloat16 tensor with a FLOAT32 residual (G = 128, uint8 / uint4 / uint2 wire) next to the
composition that defines it (the tensor widened to float32, then the float32 quantize_grouped_ef) and to the existing bfloat16-residual call, all
in the same run, with the byte ratio of each row and the target fused / composition <= 1.15 x that ratio.  Writes
profiles/grouped_ef_f32r_bench.json.

--rows reduce_ef_f32r: the fused reduce_quantize_grouped_ef of a bfloat16 accumulator with a FLOAT32 residual (G = 128; uint8 and uint4 terms
with k = 1 and k = 7, uint2 with k = 1) next to the composition that defines it (k grouped dequantize ADD launches into the bfloat16 acc + the
mixed quantize_grouped_ef) in the same run, with the byte ratio of each row and the target fused / composition <= 1.15 x that ratio.  Writes
profiles/grouped_reduce_ef_f32r_bench.json; --rows all appends these rows to its table.

--rows requant: the group-wise quantize-dequantize (quantize_dequantize_grouped, G = 128: fp32 via uint8 and uint4, bf16 via uint8, uint4 and uint2
with SET, fp32 via uint8 with ADD) next to the two calls that define it (quantize_grouped into a packed scratch tensor + dequantize_grouped) in the
same run, with the byte ratio of each row (parameter bytes counted on both sides) and the target fused / composition <= 1.15 x that ratio.  Writes
profiles/grouped_requant_bench.json; --rows all appends these rows to its table.

--rows dequant_sum: the grouped dequantize-sum (dequantize_sum_grouped, G = 128: fp32 out with uint8 and uint4 terms, k = 1 and k = 7, ADD; fp32 out
with seven uint8 terms, SET; bf16 out with seven uint4 terms, ADD) next to the composition that defines it (k grouped dequantize launches) in the
same run, with the byte ratio of each row and the target fused / composition <= 1.15 x that ratio; and the per-tensor dequantize_sum of seven
uint8 terms into fp32 as a second yardstick.  Writes profiles/grouped_dequant_sum_bench.json; --rows all appends these rows to its table.

--rows rot: the randomized Hadamard rotation of whole groups (G = 128): hadamard_grouped in place (fp32, bf16) next to quantize_dequantize_grouped of
the same type, which moves the same bytes; quantize_grouped_rotated (fp32 -> uint8, fp32 -> uint4, bf16 -> uint4, bf16 -> uint2) next to
hadamard_grouped into a scratch tensor + quantize_grouped; dequantize_grouped_rotated SET (uint4 -> bf16, uint8 -> fp32) next to dequantize_grouped +
hadamard_grouped in place; all in the same run, with the byte ratio of each row and the target fused / composition <= 1.15 x that ratio.  Writes
profiles/grouped_rot_bench.json.

--rows rot_reduce: the two steps of a grouped collective in the rotated domain (G = 128), each next to the composition of public calls that defines
it, in the same run: reduce_quantize_grouped_rotated (fp32 + 1 and + 7 uint8 terms, fp32 + 7 uint4 terms, bf16 + 1 and + 7 uint4 terms) and
dequantize_sum_grouped_rotated (1 and 7 uint8 terms into fp32, SET and ADD; 7 uint4 terms into bf16, ADD).  Every fused row must be faster than its
composition; fused / composition against the byte ratio is reported as met or missed.  Writes profiles/grouped_rot_reduce_bench.json.

--rows rot_ef: error feedback in the rotated domain (G = 128), each fused call next to the composition of public calls that defines it, in the
same run: quantize_grouped_rotated_ef (fp32 -> uint8, fp32 -> uint4, bf16 -> uint4, bf16 -> uint8) against hadamard_grouped of the widened tensor
into a float32 scratch + quantize_grouped_ef; reduce_quantize_grouped_rotated_ef (fp32 + 1 uint8 term, fp32 + 7 uint4 terms, bf16 + 1 uint4 term)
against the rotation, k float32 grouped dequantize ADD launches and quantize_grouped_ef.  Every fused row must be faster than its composition;
fused / composition against the byte ratio is reported as met or missed.  Writes profiles/grouped_rot_ef_bench.json; --rows all appends these
rows to its table.

--rows rot_batch: the batched rotated launches (G = 128; fp32 -> uint8 and bf16 -> uint4): quantize_grouped_rotated_batch and
quantize_grouped_rotated_ef_batch of the 7 peer chunks of an 8-way mesh (numel / 8 each) and dequantize_grouped_rotated_batch SET of its 8 chunks,
each next to the loop of as many single calls in the same run; and one rank's replayed 8-way rotated mesh (fp32 -> uint4: encode batch,
dequantize_sum_grouped_rotated ADD + quantize_grouped_rotated, decode batch) through piquant.distributed._DeviceOps as it is, next to a local copy
of its former three loops.  Each row: stream time from HIP events around windows of whole sequences, met or missed against the loop's time plus the
loop's own spread (max - min over its windows); --kernel-stats FILE (the kernel statistics of tools/grouped_rot_batch_workload.py under
rocprofv3 --kernel-trace --stats) adds the sums of the kernel times, judged with the same spread.  Writes profiles/grouped_rot_batch_bench.json;
--rows all appends these rows to its table.

--rows clip: the per-group clip search (quantize_grouped_clipped: fp32 -> uint8 / uint4 / uint2 and bf16 -> uint4 / uint2 at 1, 5 and 9 candidates,
G = 128; fp32 -> uint4 at G = 32 and 1024 with 9), each next to quantize_grouped of the same pair and group size in the same run -- the call that
moves the same bytes.  Reports fused us, quantize_grouped us, their ratio and the marginal us per candidate.  Writes
profiles/grouped_clip_bench.json.

    python tools/grouped_bench.py [--rows all|reduce|ef|reduce_ef|ef_f32r|reduce_ef_f32r|requant|dequant_sum|rot|rot_reduce|rot_ef|rot_batch|clip] [--windows 7] [--rotate-gb 3.3] [--out FILE] [--kernel-stats FILE]
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
HBM_PEAK_GBS = 8000.0
QUANT = {"uint8": (piquant.DataType.UINT8, 8), "uint4": (piquant.DataType.UINT4, 4), "uint2": (piquant.DataType.UINT2, 2)}
FLOAT = {"f32": (piquant.DataType.F32, torch.float32, 4), "bf16": (piquant.DataType.BF16, torch.bfloat16, 2)}
GROUPS = (32, 128, 1024, 4096)


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


def row(kind, pair, g, us, nbytes, samples):
    r = {"kind": kind, "pair": pair, "group_size": g, "us": round(us, 3), "bytes": int(nbytes), "tb_s": round(nbytes / us / 1e6, 3),
         "frac_8tbs": round(nbytes / us / 1e6 / (HBM_PEAK_GBS / 1000.0), 4), "windows_us": [round(s, 3) for s in samples]}
    print(f"{kind:22s} {pair:12s} G={g if g else '-':>5} {us:8.2f} us  {nbytes / 1e6:8.1f} MB  {r['frac_8tbs']:.3f} of 8 TB/s", flush=True)
    return r


def reduce_rows(ctx, dev, stream, args, G=128, world=8):
    """fused reduce + quantize against its two-step composition, batched calls against single calls (fp32, G = 128)"""
    fdt, esize = piquant.DataType.F32, 4
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    for qname in ("uint8", "uint4"):
        qdt, bits = QUANT[qname]
        nq = qdt.packed_nbytes(NUMEL)
        for k in (1, 7):
            per_call = NUMEL * esize + k * (nq + 5 * ng) + nq + 5 * ng
            nbuf = max(3, int(args.rotate_gb * 1e9 / per_call) + 1)
            accs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g) for _ in range(nbuf)]
            terms = [[torch.randint(0, 256, (nq,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
            tsc = [[torch.empty(ng, device=dev).uniform_(1e-3, 2e-3, generator=g) for _ in range(k)] for _ in range(nbuf)]
            tzp = [[torch.randint(0, 1 << bits, (ng,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
            outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
            zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            per_window = max(2 * nbuf, 32)

            def fused(i):
                ctx.reduce_quantize_grouped_ptr(accs[i].data_ptr(), fdt, [t.data_ptr() for t in terms[i]], [t.data_ptr() for t in tsc[i]],
                                                [t.data_ptr() for t in tzp[i]], outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                                piquant.RoundMode.NEAREST, _device_ptrs=True)

            def two_step(i):
                for t, s_, z_ in zip(terms[i], tsc[i], tzp[i]):
                    ctx.dequantize_grouped_ptr(t.data_ptr(), qdt, accs[i].data_ptr(), fdt, NUMEL, G, s_.data_ptr(), z_.data_ptr(), piquant.ReduceOp.ADD,
                                               _device_ptrs=True)
                ctx.quantize_grouped_ptr(accs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                         piquant.RoundMode.NEAREST, _device_ptrs=True)

            pair = f"f32+{k}x{qname}"
            us_t, s_t = timed(two_step, nbuf, args.windows, per_window, stream)
            two = row("reduce_two_step", pair, G, us_t, NUMEL * esize * (2 * k + 1) + k * (nq + 5 * ng) + nq + 5 * ng, s_t)
            us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
            fr = row("reduce_quantize_grouped", pair, G, us_f, per_call, s_f)
            fr["over_two_step"] = round(us_f / us_t, 3)
            print(f"    fused / two-step = {fr['over_two_step']:.3f}", flush=True)
            rows += [two, fr]
            del accs, terms, tsc, tzp, outs, sc, zs
            torch.cuda.empty_cache()
        # the mesh's batches: world - 1 chunks quantized, world chunks dequantized, each of NUMEL / world elements
        per = NUMEL // world
        xs = [torch.empty(per, device=dev).uniform_(-1, 1, generator=g) for _ in range(world)]
        qs = [torch.empty(qdt.packed_nbytes(per), dtype=torch.uint8, device=dev) for _ in range(world)]
        gs = pt.num_groups(per, G)
        sc = [torch.empty(gs, dtype=torch.float32, device=dev) for _ in range(world)]
        zs = [torch.empty(gs, dtype=torch.uint8, device=dev) for _ in range(world)]
        ys = [torch.empty(per, device=dev) for _ in range(world)]
        m = world - 1

        def qbatch(_):
            ctx.quantize_grouped_batch_ptr([x.data_ptr() for x in xs[:m]], fdt, [q.data_ptr() for q in qs[:m]], qdt, [per] * m, G,
                                           [t.data_ptr() for t in sc[:m]], [t.data_ptr() for t in zs[:m]], False, piquant.RoundMode.NEAREST, _device_ptrs=True)

        def qsingles(_):
            for j in range(m):
                ctx.quantize_grouped_ptr(xs[j].data_ptr(), fdt, qs[j].data_ptr(), qdt, per, G, sc[j].data_ptr(), zs[j].data_ptr(), False,
                                         piquant.RoundMode.NEAREST, _device_ptrs=True)

        def dbatch(_):
            ctx.dequantize_grouped_batch_ptr([q.data_ptr() for q in qs], qdt, [y.data_ptr() for y in ys], fdt, [per] * world, G, [t.data_ptr() for t in sc],
                                             [t.data_ptr() for t in zs], piquant.ReduceOp.SET, _device_ptrs=True)

        def dsingles(_):
            for j in range(world):
                ctx.dequantize_grouped_ptr(qs[j].data_ptr(), qdt, ys[j].data_ptr(), fdt, per, G, sc[j].data_ptr(), zs[j].data_ptr(), piquant.ReduceOp.SET,
                                           _device_ptrs=True)

        qb = m * (per * esize + qdt.packed_nbytes(per) + 5 * gs)
        db = world * (per * esize + qdt.packed_nbytes(per) + 5 * gs)
        for kind, fn, nbytes in ((f"quantize_grouped x{m} single", qsingles, qb), (f"quantize_grouped_batch {m}", qbatch, qb),
                                 (f"dequantize_grouped x{world} single", dsingles, db), (f"dequantize_grouped_batch {world}", dbatch, db)):
            us, s_ = timed(fn, 1, args.windows, 32, stream)
            rows.append(row(kind, f"f32<->{qname}", G, us, nbytes, s_))
        del xs, qs, sc, zs, ys
        torch.cuda.empty_cache()
    return rows


def ef_rows(ctx, dev, stream, args, G=128, world=8):
    """quantize_grouped_ef against the composition it replaces and against quantize_grouped alone, every pair; the mesh with and without it"""
    import piquant.distributed as D

    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for fname, (fdt, tdt, esize) in FLOAT.items():
        nbuf = max(3, int(args.rotate_gb * 1e9 / (2 * NUMEL * esize)) + 1)
        xs = [torch.empty(NUMEL, dtype=tdt, device=dev).normal_(generator=g) for _ in range(nbuf)]
        rs = [(torch.empty(NUMEL, dtype=torch.float32, device=dev).normal_(generator=g) * 0.01).to(tdt) for _ in range(nbuf)]
        ys = [torch.empty(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
        ds = [torch.empty(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)
        fbytes = NUMEL * esize
        us_add, s_add = timed(lambda i: torch.add(xs[i], rs[i], out=ys[i]), nbuf, args.windows, per_window, stream)
        rows.append(row("torch.add", fname, 0, us_add, 3 * fbytes, s_add))
        us_sub, s_sub = timed(lambda i: torch.sub(ys[i], ds[i], out=rs[i]), nbuf, args.windows, per_window, stream)
        rows.append(row("torch.sub", fname, 0, us_sub, 3 * fbytes, s_sub))
        for qname, (qdt, bits) in QUANT.items():
            pair = f"{fname}->{qname}"
            nq = qdt.packed_nbytes(NUMEL)
            outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]

            def quant(i):
                ctx.quantize_grouped_ptr(xs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                         piquant.RoundMode.NEAREST, _device_ptrs=True)

            def composition(i):
                torch.add(xs[i], rs[i], out=ys[i])
                ctx.quantize_grouped_ptr(ys[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                         piquant.RoundMode.NEAREST, _device_ptrs=True)
                ctx.dequantize_grouped_ptr(outs[i].data_ptr(), qdt, ds[i].data_ptr(), fdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), piquant.ReduceOp.SET,
                                           _device_ptrs=True)
                torch.sub(ys[i], ds[i], out=rs[i])

            def fused(i):
                ctx.quantize_grouped_ef_ptr(xs[i].data_ptr(), fdt, rs[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                            piquant.RoundMode.NEAREST, _device_ptrs=True)

            us_q, s_q = timed(quant, nbuf, args.windows, per_window, stream)
            qr = row("quantize_grouped", pair, G, us_q, fbytes + nq + 5 * ng, s_q)
            us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
            cr = row("ef_composition", pair, G, us_c, 8 * fbytes + 2 * (nq + 5 * ng), s_c)
            us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
            fr = row("quantize_grouped_ef", pair, G, us_f, 3 * fbytes + nq + 5 * ng, s_f)
            fr["over_composition"] = round(us_f / us_c, 3)
            fr["bytes_over_composition"] = round(fr["bytes"] / cr["bytes"], 3)
            fr["over_quantize_grouped"] = round(us_f / us_q, 3)
            fr["bytes_over_quantize_grouped"] = round(fr["bytes"] / qr["bytes"], 3)
            fr["target_0.5x_composition"] = "met" if fr["over_composition"] <= 0.5 else "missed"
            print(f"    fused / composition = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}), fused / quantize_grouped = "
                  f"{fr['over_quantize_grouped']:.3f} (bytes {fr['bytes_over_quantize_grouped']:.3f})", flush=True)
            rows += [qr, cr, fr]
            if pair == "f32->uint8":   # what a batch of one costs against the single kernel (the error-feedback single call is a batch of one)
                us_b, s_b = timed(lambda i: ctx.quantize_grouped_batch_ptr([xs[i].data_ptr()], fdt, [outs[i].data_ptr()], qdt, [NUMEL], G, [sc[i].data_ptr()],
                                                                           [zs[i].data_ptr()], False, piquant.RoundMode.NEAREST, _device_ptrs=True),
                                  nbuf, args.windows, per_window, stream)
                br = row("quantize_grouped_batch 1", pair, G, us_b, fbytes + nq + 5 * ng, s_b)
                br["over_single"] = round(us_b / us_q, 3)
                rows.append(br)
            del outs
        del xs, rs, ys, ds, sc, zs
        torch.cuda.empty_cache()

    # one rank's kernels of an 8-way grouped mesh all-reduce (no wire: stand-in receive buffers), replayed from a graph, with and without the residual
    ops = D._DeviceOps(ctx)
    x = torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g)
    res = torch.zeros(NUMEL, device=dev)
    for qname, bits in (("uint8", 8), ("quint4x2", 4)):
        qdt = getattr(torch, qname)
        chunks = D.ring_chunks(NUMEL, world, bits)
        gbytes = [D.grouped_wire_layout(e - b, G, bits).nbytes for b, e in chunks]
        slot = -(-max(gbytes) // 16) * 16
        bufs = torch.zeros(world * slot, dtype=torch.uint8, device=dev)
        mine = torch.zeros(slot, dtype=torch.uint8, device=dev)
        for j, (b, e) in enumerate(chunks):
            ops.encode_grouped(x[b:e], bufs[j * slot: j * slot + gbytes[j]], qdt, "nearest", G)
        peers = list(range(1, world))

        def mesh(ef):
            vals = [x[chunks[j][0]:chunks[j][1]] for j in peers]
            wire = [bufs[j * slot: j * slot + gbytes[j]] for j in peers]
            if ef:
                ops.encode_batch_grouped_ef(vals, [res[chunks[j][0]:chunks[j][1]] for j in peers], wire, qdt, "nearest", G)
            else:
                ops.encode_batch_grouped(vals, wire, qdt, "nearest", G)
            ops.reduce_encode_grouped([bufs[i * slot: i * slot + gbytes[0]] for i in peers], x[chunks[0][0]:chunks[0][1]], mine[: gbytes[0]], qdt, "nearest", G)
            ops.decode_batch_grouped([bufs[j * slot: j * slot + gbytes[j]] for j in range(world)], [x[chunks[j][0]:chunks[j][1]] for j in range(world)], qdt,
                                     "set", G)

        r = {"kind": "mesh_kernels_per_rank", "pair": f"f32->{qname}", "group_size": G, "world": world, "launches_per_all_reduce": 3}
        for name, ef in (("without_error_feedback_us", False), ("with_error_feedback_us", True)):
            x.uniform_(-1, 1, generator=g)
            for _ in range(3):
                mesh(ef)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                mesh(ef)
                torch.cuda.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    mesh(ef)
                graph.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
            r[name] = round(e0.elapsed_time(e1) * 1e3 / 20, 1)
        r["with_over_without"] = round(r["with_error_feedback_us"] / r["without_error_feedback_us"], 3)
        print(f"mesh f32->{qname}: {r['without_error_feedback_us']} us without, {r['with_error_feedback_us']} us with error feedback", flush=True)
        rows.append(r)
    ctx.set_stream(stream.cuda_stream)
    return rows


def reduce_ef_rows(ctx, dev, stream, args, G=128, world=8):
    """fused reduce + error-feedback quantize against the two-step composition that defines it; the mesh with the flag off and on"""
    import piquant.distributed as D

    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    for fname, qname, k in (("f32", "uint8", 1), ("f32", "uint8", 7), ("f32", "uint4", 1), ("f32", "uint4", 7), ("bf16", "uint4", 1)):
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        nq = qdt.packed_nbytes(NUMEL)
        fbytes = NUMEL * esize
        fused_bytes = 3 * fbytes + (k + 1) * (nq + 5 * ng)                    # acc, residual in and out; k terms in, one record out
        comp_bytes = (2 * k + 3) * fbytes + (k + 1) * (nq + 5 * ng)           # acc in and out per term; then acc, residual in and out
        nbuf = max(3, int(args.rotate_gb * 1e9 / fused_bytes) + 1)
        accs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g).to(tdt) for _ in range(nbuf)]
        ress = [(torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g) * 0.01).to(tdt) for _ in range(nbuf)]
        terms = [[torch.randint(0, 256, (nq,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tsc = [[torch.empty(ng, device=dev).uniform_(1e-3, 2e-3, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tzp = [[torch.randint(0, 1 << bits, (ng,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)

        def fused(i):
            ctx.reduce_quantize_grouped_ef_ptr(accs[i].data_ptr(), fdt, ress[i].data_ptr(), [t.data_ptr() for t in terms[i]], [t.data_ptr() for t in tsc[i]],
                                               [t.data_ptr() for t in tzp[i]], outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                               piquant.RoundMode.NEAREST, _device_ptrs=True)

        def two_step(i):
            for t, s_, z_ in zip(terms[i], tsc[i], tzp[i]):
                ctx.dequantize_grouped_ptr(t.data_ptr(), qdt, accs[i].data_ptr(), fdt, NUMEL, G, s_.data_ptr(), z_.data_ptr(), piquant.ReduceOp.ADD,
                                           _device_ptrs=True)
            ctx.quantize_grouped_ef_ptr(accs[i].data_ptr(), fdt, ress[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                        piquant.RoundMode.NEAREST, _device_ptrs=True)

        pair = f"{fname}+{k}x{qname}"
        us_t, s_t = timed(two_step, nbuf, args.windows, per_window, stream)
        two = row("reduce_ef_two_step", pair, G, us_t, comp_bytes, s_t)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("reduce_quantize_grouped_ef", pair, G, us_f, fused_bytes, s_f)
        fr["over_two_step"] = round(us_f / us_t, 3)
        fr["bytes_over_two_step"] = round(fused_bytes / comp_bytes, 3)
        fr["over_byte_ratio"] = round(fr["over_two_step"] / fr["bytes_over_two_step"], 3)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        print(f"    fused / two-step = {fr['over_two_step']:.3f} (bytes {fr['bytes_over_two_step']:.3f}): {fr['over_byte_ratio']:.3f} x the byte ratio, "
              f"target 1.15 {fr['target_1.15x_byte_ratio']}", flush=True)
        rows += [two, fr]
        del accs, ress, terms, tsc, tzp, outs, sc, zs
        torch.cuda.empty_cache()

    # one rank's three kernels of an 8-way grouped mesh all-reduce with error feedback (no wire: stand-in receive buffers), replayed from a graph
    ops = D._DeviceOps(ctx)
    x = torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g)
    res = torch.zeros(NUMEL, device=dev)
    for qname, bits in (("uint8", 8), ("quint4x2", 4)):
        qdt = getattr(torch, qname)
        chunks = D.ring_chunks(NUMEL, world, bits)
        gbytes = [D.grouped_wire_layout(e - b, G, bits).nbytes for b, e in chunks]
        slot = -(-max(gbytes) // 16) * 16
        bufs = torch.zeros(world * slot, dtype=torch.uint8, device=dev)
        mine = torch.zeros(slot, dtype=torch.uint8, device=dev)
        for j, (b, e) in enumerate(chunks):
            ops.encode_grouped(x[b:e], bufs[j * slot: j * slot + gbytes[j]], qdt, "nearest", G)
        peers = list(range(1, world))

        def mesh(requantize):
            ops.encode_batch_grouped_ef([x[chunks[j][0]:chunks[j][1]] for j in peers], [res[chunks[j][0]:chunks[j][1]] for j in peers],
                                        [bufs[j * slot: j * slot + gbytes[j]] for j in peers], qdt, "nearest", G)
            recv = [bufs[i * slot: i * slot + gbytes[0]] for i in peers]
            own = x[chunks[0][0]:chunks[0][1]]
            if requantize:
                ops.reduce_encode_grouped_ef(recv, own, res[chunks[0][0]:chunks[0][1]], mine[: gbytes[0]], qdt, "nearest", G)
            else:
                ops.reduce_encode_grouped(recv, own, mine[: gbytes[0]], qdt, "nearest", G)
            ops.decode_batch_grouped([bufs[j * slot: j * slot + gbytes[j]] for j in range(world)], [x[chunks[j][0]:chunks[j][1]] for j in range(world)], qdt,
                                     "set", G)

        r = {"kind": "mesh_kernels_per_rank", "pair": f"f32->{qname}", "group_size": G, "world": world, "launches_per_all_reduce": 3}
        for name, requantize in (("requantize_off_us", False), ("requantize_on_us", True)):
            x.uniform_(-1, 1, generator=g)
            res.zero_()
            for _ in range(3):
                mesh(requantize)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                mesh(requantize)
                torch.cuda.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    mesh(requantize)
                graph.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
            r[name] = round(e0.elapsed_time(e1) * 1e3 / 20, 1)
        r["on_over_off"] = round(r["requantize_on_us"] / r["requantize_off_us"], 3)
        print(f"mesh f32->{qname}: {r['requantize_off_us']} us with error_feedback_requantize off, {r['requantize_on_us']} us with it on", flush=True)
        rows.append(r)
    ctx.set_stream(stream.cuda_stream)
    return rows


def ef_f32r_rows(ctx, dev, stream, args, G=128):
    """quantize_grouped_ef of a bf16 tensor with an fp32 residual against widen + the fp32 call, and against the bf16-residual call"""
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    bf16, f32 = piquant.DataType.BF16, piquant.DataType.F32
    nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * 6)) + 1)
    xs = [torch.empty(NUMEL, dtype=torch.bfloat16, device=dev).normal_(generator=g) for _ in range(nbuf)]
    rs = [torch.empty(NUMEL, dtype=torch.float32, device=dev).normal_(generator=g) * 0.01 for _ in range(nbuf)]
    r16 = [r.to(torch.bfloat16) for r in rs]
    wide = [torch.empty(NUMEL, dtype=torch.float32, device=dev) for _ in range(nbuf)]   # where the composition's widened copy goes
    sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
    zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    per_window = max(2 * nbuf, 32)
    for qname, (qdt, bits) in QUANT.items():
        pair = f"bf16->{qname}"
        nq = qdt.packed_nbytes(NUMEL)
        outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]

        def composition(i):
            wide[i].copy_(xs[i])   # x.float() into a buffer that exists: no allocation in the timed window
            ctx.quantize_grouped_ef_ptr(wide[i].data_ptr(), f32, rs[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                        piquant.RoundMode.NEAREST, _device_ptrs=True)

        def fused(i):
            ctx.quantize_grouped_ef_ptr(xs[i].data_ptr(), bf16, rs[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                        piquant.RoundMode.NEAREST, _device_ptrs=True, residual_dtype=f32)

        def same_dtype(i):
            ctx.quantize_grouped_ef_ptr(xs[i].data_ptr(), bf16, r16[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                        piquant.RoundMode.NEAREST, _device_ptrs=True)

        us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
        cr = row("ef_f32r_composition", pair, G, us_c, NUMEL * (2 + 4) + NUMEL * 12 + nq + 5 * ng, s_c)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("quantize_grouped_ef_f32r", pair, G, us_f, NUMEL * (2 + 4 + 4) + nq + 5 * ng, s_f)
        us_b, s_b = timed(same_dtype, nbuf, args.windows, per_window, stream)
        br = row("quantize_grouped_ef", pair, G, us_b, NUMEL * (2 + 2 + 2) + nq + 5 * ng, s_b)
        fr["over_composition"] = round(us_f / us_c, 3)
        fr["bytes_over_composition"] = round(fr["bytes"] / cr["bytes"], 3)
        fr["over_byte_ratio"] = round(fr["over_composition"] / fr["bytes_over_composition"], 3)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        fr["over_bf16_residual"] = round(us_f / us_b, 3)
        fr["bytes_over_bf16_residual"] = round(fr["bytes"] / br["bytes"], 3)
        print(f"    fused / composition = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}): {fr['over_byte_ratio']:.3f} x the byte ratio, "
              f"target 1.15 {fr['target_1.15x_byte_ratio']}; fused / bf16-residual call = {fr['over_bf16_residual']:.3f} (bytes "
              f"{fr['bytes_over_bf16_residual']:.3f})", flush=True)
        rows += [cr, fr, br]
        del outs
    return rows


def reduce_ef_f32r_rows(ctx, dev, stream, args, G=128):
    """fused reduce + error-feedback quantize of a bf16 acc with an fp32 residual against the composition that defines it"""
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    bf16, f32 = piquant.DataType.BF16, piquant.DataType.F32
    for qname, k in (("uint8", 1), ("uint8", 7), ("uint4", 1), ("uint4", 7), ("uint2", 1)):
        qdt, bits = QUANT[qname]
        nq = qdt.packed_nbytes(NUMEL)
        fused_bytes = NUMEL * (2 + 4 + 4) + (k + 1) * (nq + 5 * ng)           # acc in; residual in and out; k terms in, one record out
        comp_bytes = NUMEL * (4 * k + 2 + 4 + 4) + (k + 1) * (nq + 5 * ng)    # acc in and out per term; then acc in, residual in and out
        nbuf = max(3, int(args.rotate_gb * 1e9 / fused_bytes) + 1)
        accs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g).to(torch.bfloat16) for _ in range(nbuf)]
        ress = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g) * 0.01 for _ in range(nbuf)]
        terms = [[torch.randint(0, 256, (nq,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tsc = [[torch.empty(ng, device=dev).uniform_(1e-3, 2e-3, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tzp = [[torch.randint(0, 1 << bits, (ng,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)

        def fused(i):
            ctx.reduce_quantize_grouped_ef_ptr(accs[i].data_ptr(), bf16, ress[i].data_ptr(), [t.data_ptr() for t in terms[i]], [t.data_ptr() for t in tsc[i]],
                                               [t.data_ptr() for t in tzp[i]], outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                               piquant.RoundMode.NEAREST, _device_ptrs=True, residual_dtype=f32)

        def composition(i):   # adds into accs[i] in place, call after call: the sums drift by at most 0.5 a term and call, far from any overflow,
            for t, s_, z_ in zip(terms[i], tsc[i], tzp[i]):   # and neither form's time depends on the values
                ctx.dequantize_grouped_ptr(t.data_ptr(), qdt, accs[i].data_ptr(), bf16, NUMEL, G, s_.data_ptr(), z_.data_ptr(), piquant.ReduceOp.ADD,
                                           _device_ptrs=True)
            ctx.quantize_grouped_ef_ptr(accs[i].data_ptr(), bf16, ress[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                        piquant.RoundMode.NEAREST, _device_ptrs=True, residual_dtype=f32)

        pair = f"bf16+{k}x{qname}"
        us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
        cr = row("reduce_ef_f32r_composition", pair, G, us_c, comp_bytes, s_c)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("reduce_quantize_grouped_ef_f32r", pair, G, us_f, fused_bytes, s_f)
        fr["over_composition"] = round(us_f / us_c, 3)
        fr["bytes_over_composition"] = round(fused_bytes / comp_bytes, 3)
        fr["over_byte_ratio"] = round(fr["over_composition"] / fr["bytes_over_composition"], 3)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        print(f"    fused / composition = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}): {fr['over_byte_ratio']:.3f} x the byte ratio, "
              f"target 1.15 {fr['target_1.15x_byte_ratio']}", flush=True)
        rows += [cr, fr]
        del accs, ress, terms, tsc, tzp, outs, sc, zs
        torch.cuda.empty_cache()
    return rows


def requant_rows(ctx, dev, stream, args, G=128):
    """quantize_dequantize_grouped against quantize_grouped + dequantize_grouped, the two calls that define it"""
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    for fname, qname, op in (("f32", "uint8", "set"), ("f32", "uint4", "set"), ("bf16", "uint8", "set"), ("bf16", "uint4", "set"), ("bf16", "uint2", "set"),
                             ("f32", "uint8", "add")):
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        rop = piquant.ReduceOp.ADD if op == "add" else piquant.ReduceOp.SET
        nq = qdt.packed_nbytes(NUMEL)
        fbytes = NUMEL * esize
        out_bytes = fbytes * (2 if op == "add" else 1)                          # ADD reads the accumulator too
        fused_bytes = fbytes + out_bytes + 5 * ng                               # x in; out; the parameters out
        comp_bytes = fbytes + 2 * nq + out_bytes + 10 * ng                      # the packed tensor out and in again, the parameters too
        nbuf = max(3, int(args.rotate_gb * 1e9 / fused_bytes) + 1)
        xs = [torch.empty(NUMEL, dtype=tdt, device=dev).normal_(generator=g) for _ in range(nbuf)]
        ys = [torch.zeros(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
        tmp = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)

        def fused(i):
            ctx.quantize_dequantize_grouped_ptr(xs[i].data_ptr(), fdt, ys[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                                piquant.RoundMode.NEAREST, rop, _device_ptrs=True)

        def composition(i):
            ctx.quantize_grouped_ptr(xs[i].data_ptr(), fdt, tmp[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                     piquant.RoundMode.NEAREST, _device_ptrs=True)
            ctx.dequantize_grouped_ptr(tmp[i].data_ptr(), qdt, ys[i].data_ptr(), fdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), rop, _device_ptrs=True)

        pair = f"{fname} via {qname} {op.upper()}"
        us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
        cr = row("requant_composition", pair, G, us_c, comp_bytes, s_c)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("quantize_dequantize_grouped", pair, G, us_f, fused_bytes, s_f)
        fr["over_composition"] = round(us_f / us_c, 3)
        fr["bytes_over_composition"] = round(fused_bytes / comp_bytes, 3)
        fr["over_byte_ratio"] = round(fr["over_composition"] / fr["bytes_over_composition"], 3)
        fr["faster_than_composition"] = bool(us_f < us_c)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        print(f"    fused / composition = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}): {fr['over_byte_ratio']:.3f} x the byte ratio, "
              f"target 1.15 {fr['target_1.15x_byte_ratio']}", flush=True)
        rows += [cr, fr]
        del xs, ys, tmp, sc, zs
        torch.cuda.empty_cache()
    return rows


def dequant_sum_rows(ctx, dev, stream, args, G=128):
    """dequantize_sum_grouped against the k grouped dequantize launches that define it; the per-tensor dequantize_sum beside the 7 x uint8 row"""
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(8)
    for fname, qname, k, op in (("f32", "uint8", 1, "add"), ("f32", "uint8", 7, "add"), ("f32", "uint4", 1, "add"), ("f32", "uint4", 7, "add"),
                                ("f32", "uint8", 7, "set"), ("bf16", "uint4", 7, "add")):
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        rop = piquant.ReduceOp.ADD if op == "add" else piquant.ReduceOp.SET
        nq = qdt.packed_nbytes(NUMEL)
        fbytes = NUMEL * esize
        fused_bytes = k * (nq + 5 * ng) + fbytes * (2 if op == "add" else 1)             # k terms in; out (ADD: in and) out
        comp_bytes = k * (nq + 5 * ng) + fbytes * (2 * k if op == "add" else 2 * k - 1)   # out in and out per term (SET: the first only writes)
        nbuf = max(3, int(args.rotate_gb * 1e9 / fused_bytes) + 1)
        outs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g).to(tdt) for _ in range(nbuf)]
        terms = [[torch.randint(0, 256, (nq,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tsc = [[torch.empty(ng, device=dev).uniform_(1e-3, 2e-3, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tzp = [[torch.randint(0, 1 << bits, (ng,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)

        def fused(i):
            ctx.dequantize_sum_grouped_ptr([t.data_ptr() for t in terms[i]], qdt, [t.data_ptr() for t in tsc[i]], [t.data_ptr() for t in tzp[i]],
                                           outs[i].data_ptr(), fdt, NUMEL, G, rop, _device_ptrs=True)

        def composition(i):   # ADD accumulates into outs[i] call after call: at most 0.5 a term and call, far from any overflow
            for j, (t, s_, z_) in enumerate(zip(terms[i], tsc[i], tzp[i])):
                ctx.dequantize_grouped_ptr(t.data_ptr(), qdt, outs[i].data_ptr(), fdt, NUMEL, G, s_.data_ptr(), z_.data_ptr(),
                                           rop if j == 0 else piquant.ReduceOp.ADD, _device_ptrs=True)

        pair = f"{fname}{'+=' if op == 'add' else '='}{k}x{qname}"
        us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
        cr = row("dequant_sum_composition", pair, G, us_c, comp_bytes, s_c)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("dequantize_sum_grouped", pair, G, us_f, fused_bytes, s_f)
        fr["over_composition"] = round(us_f / us_c, 3)
        fr["bytes_over_composition"] = round(fused_bytes / comp_bytes, 3)
        fr["over_byte_ratio"] = round(fr["over_composition"] / fr["bytes_over_composition"], 3)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        print(f"    fused / composition = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}): {fr['over_byte_ratio']:.3f} x the byte ratio, "
              f"target 1.15 {fr['target_1.15x_byte_ratio']}", flush=True)
        rows += [cr, fr]
        if (fname, qname, k, op) == ("f32", "uint8", 7, "add"):   # the second yardstick: the per-tensor call on the same buffers, one record per term
            recs = [[torch.zeros(16, dtype=torch.uint8, device=dev) for _ in range(k)] for _ in range(nbuf)]
            x0 = torch.empty(4096, device=dev).uniform_(-1, 1, generator=g)
            for rr in recs:
                for rec in rr:
                    pt.compute_quant_params_device(x0, dtype=torch.uint8, out=rec)
            us_p, s_p = timed(lambda i: ctx.dequantize_sum_ptr([t.data_ptr() for t in terms[i]], [r_.data_ptr() for r_ in recs[i]], qdt, outs[i].data_ptr(), fdt,
                                                               NUMEL, rop, _device_ptrs=True), nbuf, args.windows, per_window, stream)
            pr = row("dequantize_sum (per tensor)", pair, 0, us_p, k * nq + 2 * fbytes, s_p)
            fr["over_per_tensor_dequantize_sum"] = round(us_f / us_p, 3)
            print(f"    grouped / per-tensor dequantize_sum = {fr['over_per_tensor_dequantize_sum']:.3f}", flush=True)
            rows.append(pr)
            del recs
        del outs, terms, tsc, tzp
        torch.cuda.empty_cache()
    return rows


def rot_rows(ctx, dev, stream, args, G=128, seed=0x9E3779B97F4A7C15):
    """the stand-alone rotation against quantize_dequantize_grouped (the same bytes); the two rotated calls against the compositions they replace"""
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(9)

    def ratio(fr, cr, what="composition"):
        fr["over_composition"] = round(fr["us"] / cr["us"], 3)
        fr["bytes_over_composition"] = round(fr["bytes"] / cr["bytes"], 3)
        fr["over_byte_ratio"] = round(fr["over_composition"] / fr["bytes_over_composition"], 3)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        print(f"    {fr['kind']} / {what} = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}): {fr['over_byte_ratio']:.3f} x the byte "
              f"ratio, target 1.15 {fr['target_1.15x_byte_ratio']}", flush=True)

    for fname, (fdt, tdt, esize) in FLOAT.items():
        fbytes = NUMEL * esize
        nbuf = max(3, int(args.rotate_gb * 1e9 / (2 * fbytes)) + 1)
        xs = [torch.empty(NUMEL, dtype=tdt, device=dev).normal_(generator=g) for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)
        # in place, call after call: the rotation is orthogonal and the fake quantization idempotent, so the values stay where they are
        us_q, s_q = timed(lambda i: ctx.quantize_dequantize_grouped_ptr(xs[i].data_ptr(), fdt, xs[i].data_ptr(), piquant.DataType.UINT8, NUMEL, G, 0, 0, False,
                                                                        piquant.RoundMode.NEAREST, piquant.ReduceOp.SET, _device_ptrs=True),
                          nbuf, args.windows, per_window, stream)
        qr = row("quantize_dequantize_grouped in place", f"{fname} via uint8", G, us_q, 2 * fbytes, s_q)
        us_h, s_h = timed(lambda i: ctx.hadamard_grouped_ptr(xs[i].data_ptr(), fdt, xs[i].data_ptr(), NUMEL, G, seed, False, _device_ptrs=True),
                          nbuf, args.windows, per_window, stream)
        hr = row("hadamard_grouped in place", fname, G, us_h, 2 * fbytes, s_h)
        ratio(hr, qr, "quantize_dequantize_grouped")
        rows += [qr, hr]
        rot = [torch.empty(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        for qname in {"f32": ("uint8", "uint4"), "bf16": ("uint4", "uint2")}[fname]:
            qdt, bits = QUANT[qname]
            nq = qdt.packed_nbytes(NUMEL)
            outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]

            def composition(i):
                ctx.hadamard_grouped_ptr(xs[i].data_ptr(), fdt, rot[i].data_ptr(), NUMEL, G, seed, False, _device_ptrs=True)
                ctx.quantize_grouped_ptr(rot[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                         piquant.RoundMode.NEAREST, _device_ptrs=True)

            def fused(i):
                ctx.quantize_grouped_rotated_ptr(xs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), seed,
                                                 piquant.RoundMode.NEAREST, _device_ptrs=True)

            pair = f"{fname}->{qname}"
            us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
            cr = row("hadamard + quantize_grouped", pair, G, us_c, 3 * fbytes + nq + 5 * ng, s_c)
            us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
            fr = row("quantize_grouped_rotated", pair, G, us_f, fbytes + nq + 5 * ng, s_f)
            ratio(fr, cr)
            rows += [cr, fr]
            if (fname, qname) in (("f32", "uint8"), ("bf16", "uint4")):   # the way back of the same pair, with this call's bytes and parameters
                dpair = f"{qname}->{fname}"

                def dcomposition(i):
                    ctx.dequantize_grouped_ptr(outs[i].data_ptr(), qdt, rot[i].data_ptr(), fdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                               piquant.ReduceOp.SET, _device_ptrs=True)
                    ctx.hadamard_grouped_ptr(rot[i].data_ptr(), fdt, rot[i].data_ptr(), NUMEL, G, seed, True, _device_ptrs=True)

                def dfused(i):
                    ctx.dequantize_grouped_rotated_ptr(outs[i].data_ptr(), qdt, rot[i].data_ptr(), fdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), seed,
                                                       piquant.ReduceOp.SET, _device_ptrs=True)

                us_c, s_c = timed(dcomposition, nbuf, args.windows, per_window, stream)
                cr = row("dequantize_grouped + hadamard", dpair, G, us_c, 3 * fbytes + nq + 5 * ng, s_c)
                us_f, s_f = timed(dfused, nbuf, args.windows, per_window, stream)
                fr = row("dequantize_grouped_rotated", dpair, G, us_f, fbytes + nq + 5 * ng, s_f)
                ratio(fr, cr)
                rows += [cr, fr]
            del outs
        del xs, rot, sc, zs
        torch.cuda.empty_cache()
    return rows


def rot_reduce_rows(ctx, dev, stream, args, G=128, seed=0x9E3779B97F4A7C15):
    """the two steps of a grouped collective in the rotated domain, each next to the composition of public calls that defines it:
    reduce_quantize_grouped_rotated against hadamard_grouped into a float32 scratch (a bfloat16 accumulator is widened into it first), k grouped
    dequantize ADD launches and quantize_grouped; dequantize_sum_grouped_rotated against dequantize_sum_grouped into a float32 scratch,
    hadamard_grouped inverse in place and the add or the convert (float32 SET: the scratch is out itself)"""
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(10)
    f32 = piquant.DataType.F32

    def ratio(fr, cr):
        fr["over_composition"] = round(fr["us"] / cr["us"], 3)
        fr["faster_than_composition"] = bool(fr["us"] < cr["us"])
        fr["bytes_over_composition"] = round(fr["bytes"] / cr["bytes"], 3)
        fr["over_byte_ratio"] = round(fr["over_composition"] / fr["bytes_over_composition"], 3)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        print(f"    fused / composition = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}): {fr['over_byte_ratio']:.3f} x the byte ratio, "
              f"target 1.15 {fr['target_1.15x_byte_ratio']}; faster than its composition: {fr['faster_than_composition']}", flush=True)

    def make_terms(nbuf, k, nq, bits):
        terms = [[torch.randint(0, 256, (nq,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tsc = [[torch.empty(ng, device=dev).uniform_(1e-3, 2e-3, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tzp = [[torch.randint(0, 1 << bits, (ng,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        return terms, tsc, tzp

    for fname, qname, k in (("f32", "uint8", 1), ("f32", "uint8", 7), ("f32", "uint4", 7), ("bf16", "uint4", 1), ("bf16", "uint4", 7)):
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        nq = qdt.packed_nbytes(NUMEL)
        rec = nq + 5 * ng
        fused_bytes = NUMEL * esize + (k + 1) * rec
        comp_bytes = (6 * NUMEL if fname == "bf16" else 0) + 8 * NUMEL + k * (rec + 8 * NUMEL) + 4 * NUMEL + rec
        nbuf = max(3, int(args.rotate_gb * 1e9 / fused_bytes) + 1)
        accs = [torch.empty(NUMEL, device=dev).normal_(generator=g).to(tdt) for _ in range(nbuf)]
        scratch = [torch.empty(NUMEL, device=dev) for _ in range(nbuf)]
        outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        terms, tsc, tzp = make_terms(nbuf, k, nq, bits)
        per_window = max(2 * nbuf, 32)

        def fused(i):
            ctx.reduce_quantize_grouped_rotated_ptr(accs[i].data_ptr(), fdt, [t.data_ptr() for t in terms[i]], [t.data_ptr() for t in tsc[i]],
                                                    [t.data_ptr() for t in tzp[i]], outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), seed,
                                                    piquant.RoundMode.NEAREST, _device_ptrs=True)

        def composition(i):
            src = accs[i]
            if fname == "bf16":
                scratch[i].copy_(accs[i])
                src = scratch[i]
            ctx.hadamard_grouped_ptr(src.data_ptr(), f32, scratch[i].data_ptr(), NUMEL, G, seed, False, _device_ptrs=True)
            for t, s_, z_ in zip(terms[i], tsc[i], tzp[i]):
                ctx.dequantize_grouped_ptr(t.data_ptr(), qdt, scratch[i].data_ptr(), f32, NUMEL, G, s_.data_ptr(), z_.data_ptr(), piquant.ReduceOp.ADD,
                                           _device_ptrs=True)
            ctx.quantize_grouped_ptr(scratch[i].data_ptr(), f32, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                     piquant.RoundMode.NEAREST, _device_ptrs=True)

        pair = f"{fname}+{k}x{qname}->{qname}"
        us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
        cr = row("rot_reduce_composition", pair, G, us_c, comp_bytes, s_c)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("reduce_quantize_grouped_rotated", pair, G, us_f, fused_bytes, s_f)
        ratio(fr, cr)
        rows += [cr, fr]
        del accs, scratch, outs, sc, zs, terms, tsc, tzp
        torch.cuda.empty_cache()

    for fname, qname, k, op in (("f32", "uint8", 1, "set"), ("f32", "uint8", 1, "add"), ("f32", "uint8", 7, "set"), ("f32", "uint8", 7, "add"),
                                ("bf16", "uint4", 7, "add")):
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        rop = piquant.ReduceOp.ADD if op == "add" else piquant.ReduceOp.SET
        nq = qdt.packed_nbytes(NUMEL)
        rec = nq + 5 * ng
        fbytes = NUMEL * esize
        fused_bytes = k * rec + fbytes * (2 if op == "add" else 1)
        direct = fname == "f32" and op == "set"      # the scratch is out itself: two launches
        comp_bytes = k * rec + 4 * NUMEL + 8 * NUMEL + (0 if direct else 4 * NUMEL + 2 * fbytes)
        nbuf = max(3, int(args.rotate_gb * 1e9 / fused_bytes) + 1)
        outs = [torch.empty(NUMEL, device=dev).uniform_(-1, 1, generator=g).to(tdt) for _ in range(nbuf)]
        scratch = outs if direct else [torch.empty(NUMEL, device=dev) for _ in range(nbuf)]
        terms, tsc, tzp = make_terms(nbuf, k, nq, bits)
        per_window = max(2 * nbuf, 32)

        def fused(i):
            ctx.dequantize_sum_grouped_rotated_ptr([t.data_ptr() for t in terms[i]], qdt, [t.data_ptr() for t in tsc[i]], [t.data_ptr() for t in tzp[i]],
                                                   outs[i].data_ptr(), fdt, NUMEL, G, seed, rop, _device_ptrs=True)

        def composition(i):
            ctx.dequantize_sum_grouped_ptr([t.data_ptr() for t in terms[i]], qdt, [t.data_ptr() for t in tsc[i]], [t.data_ptr() for t in tzp[i]],
                                           scratch[i].data_ptr(), f32, NUMEL, G, piquant.ReduceOp.SET, _device_ptrs=True)
            ctx.hadamard_grouped_ptr(scratch[i].data_ptr(), f32, scratch[i].data_ptr(), NUMEL, G, seed, True, _device_ptrs=True)
            if not direct:
                outs[i].add_(scratch[i]) if op == "add" else outs[i].copy_(scratch[i])

        pair = f"{fname}{'+=' if op == 'add' else '='}{k}x{qname}"
        us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
        cr = row("rot_dequant_sum_composition", pair, G, us_c, comp_bytes, s_c)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("dequantize_sum_grouped_rotated", pair, G, us_f, fused_bytes, s_f)
        ratio(fr, cr)
        rows += [cr, fr]
        del outs, scratch, terms, tsc, tzp
        torch.cuda.empty_cache()
    return rows


def rot_ef_rows(ctx, dev, stream, args, G=128, seed=0x9E3779B97F4A7C15):
    """error feedback in the rotated domain, each fused call next to the composition of public calls that defines it: hadamard_grouped into a
    float32 scratch (a bfloat16 tensor is widened into it first), k float32 grouped dequantize ADD launches, quantize_grouped_ef of the scratch
    with the float32 residual.  k = 0: quantize_grouped_rotated_ef."""
    ng = pt.num_groups(NUMEL, G)
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    f32 = piquant.DataType.F32

    def ratio(fr, cr):
        fr["over_composition"] = round(fr["us"] / cr["us"], 3)
        fr["faster_than_composition"] = bool(fr["us"] < cr["us"])
        fr["bytes_over_composition"] = round(fr["bytes"] / cr["bytes"], 3)
        fr["over_byte_ratio"] = round(fr["over_composition"] / fr["bytes_over_composition"], 3)
        fr["target_1.15x_byte_ratio"] = "met" if fr["over_byte_ratio"] <= 1.15 else "missed"
        print(f"    fused / composition = {fr['over_composition']:.3f} (bytes {fr['bytes_over_composition']:.3f}): {fr['over_byte_ratio']:.3f} x the byte ratio, "
              f"target 1.15 {fr['target_1.15x_byte_ratio']}; faster than its composition: {fr['faster_than_composition']}", flush=True)

    for fname, qname, k in (("f32", "uint8", 0), ("f32", "uint4", 0), ("bf16", "uint4", 0), ("bf16", "uint8", 0), ("f32", "uint8", 1), ("f32", "uint4", 7),
                            ("bf16", "uint4", 1)):
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        nq = qdt.packed_nbytes(NUMEL)
        rec = nq + 5 * ng
        fused_bytes = NUMEL * esize + 8 * NUMEL + (k + 1) * rec
        comp_bytes = (6 * NUMEL if fname == "bf16" else 0) + 8 * NUMEL + k * (rec + 8 * NUMEL) + 12 * NUMEL + rec
        nbuf = max(3, int(args.rotate_gb * 1e9 / fused_bytes) + 1)
        accs = [torch.empty(NUMEL, device=dev).normal_(generator=g).to(tdt) for _ in range(nbuf)]
        res = [torch.empty(NUMEL, device=dev).normal_(generator=g).mul_(0.01) for _ in range(nbuf)]
        scratch = [torch.empty(NUMEL, device=dev) for _ in range(nbuf)]
        outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        terms = [[torch.randint(0, 256, (nq,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tsc = [[torch.empty(ng, device=dev).uniform_(1e-3, 2e-3, generator=g) for _ in range(k)] for _ in range(nbuf)]
        tzp = [[torch.randint(0, 1 << bits, (ng,), dtype=torch.uint8, device=dev, generator=g) for _ in range(k)] for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)

        def fused(i):
            if k == 0:
                ctx.quantize_grouped_rotated_ef_ptr(accs[i].data_ptr(), fdt, res[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(),
                                                    zs[i].data_ptr(), seed, piquant.RoundMode.NEAREST, _device_ptrs=True)
            else:
                ctx.reduce_quantize_grouped_rotated_ef_ptr(accs[i].data_ptr(), fdt, res[i].data_ptr(), [t.data_ptr() for t in terms[i]],
                                                           [t.data_ptr() for t in tsc[i]], [t.data_ptr() for t in tzp[i]], outs[i].data_ptr(), qdt, NUMEL, G,
                                                           sc[i].data_ptr(), zs[i].data_ptr(), seed, piquant.RoundMode.NEAREST, _device_ptrs=True)

        def composition(i):
            src = accs[i]
            if fname == "bf16":
                scratch[i].copy_(accs[i])
                src = scratch[i]
            ctx.hadamard_grouped_ptr(src.data_ptr(), f32, scratch[i].data_ptr(), NUMEL, G, seed, False, _device_ptrs=True)
            for t, s_, z_ in zip(terms[i], tsc[i], tzp[i]):
                ctx.dequantize_grouped_ptr(t.data_ptr(), qdt, scratch[i].data_ptr(), f32, NUMEL, G, s_.data_ptr(), z_.data_ptr(), piquant.ReduceOp.ADD,
                                           _device_ptrs=True)
            ctx.quantize_grouped_ef_ptr(scratch[i].data_ptr(), f32, res[i].data_ptr(), outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                        piquant.RoundMode.NEAREST, _device_ptrs=True)

        pair = f"{fname}->{qname}" if k == 0 else f"{fname}+{k}x{qname}->{qname}"
        us_c, s_c = timed(composition, nbuf, args.windows, per_window, stream)
        cr = row("rot_ef_composition" if k == 0 else "rot_reduce_ef_composition", pair, G, us_c, comp_bytes, s_c)
        us_f, s_f = timed(fused, nbuf, args.windows, per_window, stream)
        fr = row("quantize_grouped_rotated_ef" if k == 0 else "reduce_quantize_grouped_rotated_ef", pair, G, us_f, fused_bytes, s_f)
        ratio(fr, cr)
        rows += [cr, fr]
        del accs, res, scratch, outs, sc, zs, terms, tsc, tzp
        torch.cuda.empty_cache()
    return rows


ROT_SEED = 0x9E3779B97F4A7C15
ROT_BATCH_PAIRS = (("f32", "uint8"), ("bf16", "uint4"))
ROT_BATCH_MESH_PAIR = ("f32", "uint4")   # another instance than the rows', so that a kernel trace of the whole run keeps the two apart


def rot_batch_cases(ctx, dev, rotate_gb, G=128, world=8, seed=ROT_SEED):
    """The three batched rotated calls on the chunks of an 8-way mesh (world - 1 members for the two quantizing calls, world for the dequantize, each
    of NUMEL / world elements), next to the loop of single calls -- what the parent of the batched launches made of the same chunks.  Yields
    (kind, pair, members, nbuf, bytes, batch(i), loop(i)) with `nbuf` cold sets of buffers; tools/grouped_rot_batch_workload.py runs the same
    cases under a profiler."""
    per = NUMEL // world
    gs = pt.num_groups(per, G)
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    nearest, op_set = piquant.RoundMode.NEAREST, piquant.ReduceOp.SET
    for fname, qname in ROT_BATCH_PAIRS:
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        nq = qdt.packed_nbytes(per)
        for kind, m in (("quantize_grouped_rotated", world - 1), ("quantize_grouped_rotated_ef", world - 1), ("dequantize_grouped_rotated", world)):
            ef, deq = kind.endswith("_ef"), kind.startswith("dequantize")
            member = per * esize + nq + 5 * gs + (8 * per if ef else 0)
            nbuf = max(3, int(rotate_gb * 1e9 / (m * member)) + 1)
            xs = [[torch.empty(per, device=dev).normal_(generator=g).to(tdt) for _ in range(m)] for _ in range(nbuf)]
            rs = [[torch.empty(per, device=dev).normal_(generator=g).mul_(0.01) for _ in range(m)] for _ in range(nbuf)] if ef else None
            if deq:
                qs = [[torch.randint(0, 256, (nq,), dtype=torch.uint8, device=dev, generator=g) for _ in range(m)] for _ in range(nbuf)]
                sc = [[torch.empty(gs, device=dev).uniform_(1e-3, 2e-3, generator=g) for _ in range(m)] for _ in range(nbuf)]
                zs = [[torch.randint(0, 1 << bits, (gs,), dtype=torch.uint8, device=dev, generator=g) for _ in range(m)] for _ in range(nbuf)]
            else:
                qs = [[torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(m)] for _ in range(nbuf)]
                sc = [[torch.empty(gs, dtype=torch.float32, device=dev) for _ in range(m)] for _ in range(nbuf)]
                zs = [[torch.empty(gs, dtype=torch.uint8, device=dev) for _ in range(m)] for _ in range(nbuf)]
            ptrs = lambda ts: [t.data_ptr() for t in ts]   # noqa: E731

            def batch(i, ef=ef, deq=deq, xs=xs, rs=rs, qs=qs, sc=sc, zs=zs, m=m, fdt=fdt, qdt=qdt):
                if deq:
                    ctx.dequantize_grouped_rotated_batch_ptr(ptrs(qs[i]), qdt, ptrs(xs[i]), fdt, [per] * m, G, ptrs(sc[i]), ptrs(zs[i]), seed, op_set,
                                                             _device_ptrs=True)
                elif ef:
                    ctx.quantize_grouped_rotated_ef_batch_ptr(ptrs(xs[i]), fdt, ptrs(rs[i]), ptrs(qs[i]), qdt, [per] * m, G, ptrs(sc[i]), ptrs(zs[i]), seed,
                                                              nearest, _device_ptrs=True)
                else:
                    ctx.quantize_grouped_rotated_batch_ptr(ptrs(xs[i]), fdt, ptrs(qs[i]), qdt, [per] * m, G, ptrs(sc[i]), ptrs(zs[i]), seed, nearest,
                                                           _device_ptrs=True)

            def loop(i, ef=ef, deq=deq, xs=xs, rs=rs, qs=qs, sc=sc, zs=zs, m=m, fdt=fdt, qdt=qdt):
                for j in range(m):
                    if deq:
                        ctx.dequantize_grouped_rotated_ptr(qs[i][j].data_ptr(), qdt, xs[i][j].data_ptr(), fdt, per, G, sc[i][j].data_ptr(),
                                                           zs[i][j].data_ptr(), seed, op_set, _device_ptrs=True)
                    elif ef:
                        ctx.quantize_grouped_rotated_ef_ptr(xs[i][j].data_ptr(), fdt, rs[i][j].data_ptr(), qs[i][j].data_ptr(), qdt, per, G,
                                                            sc[i][j].data_ptr(), zs[i][j].data_ptr(), seed, nearest, _device_ptrs=True)
                    else:
                        ctx.quantize_grouped_rotated_ptr(xs[i][j].data_ptr(), fdt, qs[i][j].data_ptr(), qdt, per, G, sc[i][j].data_ptr(),
                                                         zs[i][j].data_ptr(), seed, nearest, _device_ptrs=True)

            yield kind, (f"{qname}->{fname}" if deq else f"{fname}->{qname}"), m, nbuf, m * member, batch, loop
            del xs, rs, qs, sc, zs, batch, loop
            torch.cuda.empty_cache()


def rot_batch_mesh(ctx, dev, G=128, world=8, seed=ROT_SEED):
    """One rank's kernels of an 8-way rotated grouped mesh all-reduce (no wire: stand-in receive buffers), built as the replayed-mesh rows of
    --rows ef are: the encode batch of the world - 1 peer chunks, the owner's dequantize_sum_grouped_rotated ADD + quantize_grouped_rotated, the
    decode batch of the world chunks.  -> {"batched": mesh(), "loop": mesh()}: piquant.distributed._DeviceOps as it is, and the same with a local
    copy of the three loops of single launches it had before the batched rotated launches."""
    import piquant.distributed as D

    class LoopOps(D._DeviceOps):
        def encode_batch_grouped_rotated(self, xs, bufs, qdtype, round_mode, group_size, seed):
            for x, b in zip(xs, bufs):
                self.encode_grouped_rotated(x, b, qdtype, round_mode, group_size, seed)

        def decode_batch_grouped_rotated(self, bufs, outs, qdtype, reduce_op, group_size, seed):
            for b, o in zip(bufs, outs):
                self.decode_grouped_rotated(b, o, qdtype, reduce_op, group_size, seed)

        def encode_batch_grouped_rotated_ef(self, xs, residuals, bufs, qdtype, round_mode, group_size, seed):
            for x, r, b in zip(xs, residuals, bufs):
                self.encode_grouped_rotated_ef(x, r, b, qdtype, round_mode, group_size, seed)

    fname, qname = ROT_BATCH_MESH_PAIR
    bits = QUANT[qname][1]
    qdt = {8: torch.uint8, 4: torch.quint4x2, 2: torch.quint2x4}[bits]
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    x = torch.empty(NUMEL, device=dev).normal_(generator=g).to(FLOAT[fname][1])
    chunks = D.ring_chunks(NUMEL, world, bits)
    gbytes = [D.grouped_wire_layout(e - b, G, bits).nbytes for b, e in chunks]
    slot = -(-max(gbytes) // 16) * 16
    bufs = torch.zeros(world * slot, dtype=torch.uint8, device=dev)
    mine = torch.zeros(slot, dtype=torch.uint8, device=dev)
    peers = list(range(1, world))
    D._DeviceOps(ctx).encode_batch_grouped_rotated([x[b:e] for b, e in chunks], [bufs[j * slot: j * slot + gbytes[j]] for j in range(world)], qdt, "nearest",
                                                   G, seed)

    def mesh_of(ops):
        def mesh():
            ops.encode_batch_grouped_rotated([x[chunks[j][0]:chunks[j][1]] for j in peers], [bufs[j * slot: j * slot + gbytes[j]] for j in peers], qdt,
                                             "nearest", G, seed)
            own = x[chunks[0][0]:chunks[0][1]]
            ops.decode_sum_grouped_rotated([bufs[i * slot: i * slot + gbytes[0]] for i in peers], own, qdt, "add", G, seed)
            ops.encode_grouped_rotated(own, mine[: gbytes[0]], qdt, "nearest", G, seed)
            ops.decode_batch_grouped_rotated([bufs[j * slot: j * slot + gbytes[j]] for j in range(world)], [x[chunks[j][0]:chunks[j][1]] for j in range(world)],
                                             qdt, "set", G, seed)
        return mesh

    return {"batched": mesh_of(D._DeviceOps(ctx)), "loop": mesh_of(LoopOps(ctx))}


def rot_batch_kernel_sums(path, world=8):
    """{(kind, pair): (batch kernel us, loop kernel us)} from the kernel statistics (rocprofv3 --kernel-trace --stats, CSV) of a run of
    tools/grouped_rot_batch_workload.py: a batch is ONE dispatch of its batch kernel, the loop `members` dispatches of the single-tensor kernel."""
    import csv
    import re

    avg = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"pq::(\w+)<(\d+), (\d+), \d+, 128>", r["Name"])
            if m:
                avg[(m.group(1), int(m.group(2)), int(m.group(3)))] = float(r["AverageNs"]) / 1000.0
    dt = {"f32": int(piquant.DataType.F32.value), "bf16": int(piquant.DataType.BF16.value)}
    sums = {}
    for fname, qname in ROT_BATCH_PAIRS:
        key = (dt[fname], QUANT[qname][1])
        for kind, m, pair in (("quantize_grouped_rotated", world - 1, f"{fname}->{qname}"), ("quantize_grouped_rotated_ef", world - 1, f"{fname}->{qname}"),
                              ("dequantize_grouped_rotated", world, f"{qname}->{fname}")):
            sums[(kind, pair)] = (avg[(kind + "_batch_kernel",) + key], m * avg[(kind + "_kernel",) + key])
    fname, qname = ROT_BATCH_MESH_PAIR
    key = (dt[fname], QUANT[qname][1])
    owner = avg[("dequantize_sum_grouped_rotated_kernel",) + key] + avg[("quantize_grouped_rotated_kernel",) + key]
    sums[("rotated_mesh_kernels_per_rank", f"{fname}->{qname}")] = (
        avg[("quantize_grouped_rotated_batch_kernel",) + key] + owner + avg[("dequantize_grouped_rotated_batch_kernel",) + key],
        (world - 1) * avg[("quantize_grouped_rotated_kernel",) + key] + owner + world * avg[("dequantize_grouped_rotated_kernel",) + key])
    return sums


def rot_batch_rows(ctx, dev, stream, args, G=128, world=8):
    """the batched rotated launches against the loop of single launches, in the same run: stream time (HIP events around each window of whole
    sequences) and, with --kernel-stats, the sum of the kernel times.  Targets: the batch's stream time <= the loop's + the loop's own spread
    (max - min over its windows); the batch's kernel time <= the loop's kernel-time sum + that same spread."""
    rows = []
    sums = rot_batch_kernel_sums(args.kernel_stats, world) if args.kernel_stats else {}

    def judge(br, lr, key):
        spread = max(lr["windows_us"]) - min(lr["windows_us"])
        br["loop_us"], br["loop_spread_us"], br["over_loop"] = lr["us"], round(spread, 3), round(br["us"] / lr["us"], 3)
        br["stream_time_target"] = "met" if br["us"] <= lr["us"] + spread else "missed"
        line = f"    batch / loop = {br['over_loop']:.3f} (loop spread {spread:.2f} us): stream time {br['stream_time_target']}"
        if key in sums:
            br["kernel_us"], br["loop_kernel_us"] = round(sums[key][0], 3), round(sums[key][1], 3)
            br["kernel_time_target"] = "met" if sums[key][0] <= sums[key][1] + spread else "missed"
            line += f"; kernel time {br['kernel_us']:.2f} against {br['loop_kernel_us']:.2f} us: {br['kernel_time_target']}"
        print(line, flush=True)

    for kind, pair, m, nbuf, nbytes, batch, loop in rot_batch_cases(ctx, dev, args.rotate_gb, G, world):
        per_window = max(2 * nbuf, 32)
        us_l, s_l = timed(loop, nbuf, args.windows, per_window, stream)
        lr = row(f"{kind} x{m} single", pair, G, us_l, nbytes, s_l)
        us_b, s_b = timed(batch, nbuf, args.windows, per_window, stream)
        br = row(f"{kind}_batch {m}", pair, G, us_b, nbytes, s_b)
        judge(br, lr, (kind, pair))
        rows += [lr, br]
    # one rank's replayed mesh: windows of 20 replays of the captured sequence
    meshes = rot_batch_mesh(ctx, dev, G, world)
    res = {}
    for name in ("loop", "batched"):
        mesh = meshes[name]
        for _ in range(3):
            mesh()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            mesh()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                mesh()
            graph.replay()
            torch.cuda.synchronize()
            samples = []
            for _ in range(args.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
                samples.append(e0.elapsed_time(e1) * 1e3 / 20)
        res[name] = samples
    ctx.set_stream(stream.cuda_stream)
    pair = "->".join(ROT_BATCH_MESH_PAIR)
    launches = {"loop": (world - 1) + 2 + world, "batched": 4}
    out = {}
    for name in ("loop", "batched"):
        out[name] = {"kind": f"rotated_mesh_kernels_per_rank ({name})", "pair": pair, "group_size": G, "world": world,
                     "launches_per_all_reduce": launches[name], "us": round(statistics.median(res[name]), 3), "windows_us": [round(s, 3) for s in res[name]]}
        print(f"rotated mesh {pair} ({name}, {launches[name]} launches): {out[name]['us']:.1f} us per replay", flush=True)
    judge(out["batched"], out["loop"], ("rotated_mesh_kernels_per_rank", pair))
    return rows + [out["loop"], out["batched"]]


def clip_rows(ctx, dev, stream, args):
    """quantize_grouped_clipped at 1, 5 and 9 candidates against quantize_grouped: the same bytes, so the difference is arithmetic"""
    rows = []
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    cases = [(f, q, 128, (1, 5, 9)) for f, q in (("f32", "uint8"), ("f32", "uint4"), ("f32", "uint2"), ("bf16", "uint4"), ("bf16", "uint2"))]
    cases += [("f32", "uint4", 32, (9,)), ("f32", "uint4", 1024, (9,))]
    for fname, qname, G, steps_list in cases:
        fdt, tdt, esize = FLOAT[fname]
        qdt, bits = QUANT[qname]
        ng = pt.num_groups(NUMEL, G)
        nq = qdt.packed_nbytes(NUMEL)
        nbytes = NUMEL * esize + nq + 5 * ng                                    # x in; packed bytes and parameters out: the same for both calls
        nbuf = max(3, int(args.rotate_gb * 1e9 / nbytes) + 1)
        xs = [torch.empty(NUMEL, dtype=tdt, device=dev).normal_(generator=g) for _ in range(nbuf)]
        outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
        zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        per_window = max(2 * nbuf, 32)
        pair = f"{fname}->{qname}"

        def plain(i):
            ctx.quantize_grouped_ptr(xs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), False,
                                     piquant.RoundMode.NEAREST, _device_ptrs=True)

        us_p, s_p = timed(plain, nbuf, args.windows, per_window, stream)
        rows.append(row("quantize_grouped", pair, G, us_p, nbytes, s_p))
        for steps in steps_list:
            def clipped(i, steps=steps):
                ctx.quantize_grouped_clipped_ptr(xs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(), 0, steps,
                                                 piquant.RoundMode.NEAREST, _device_ptrs=True)

            us_c, s_c = timed(clipped, nbuf, args.windows, per_window, stream)
            r = row(f"quantize_grouped_clipped steps={steps}", pair, G, us_c, nbytes, s_c)
            r["steps"] = steps
            r["quantize_grouped_us"] = round(us_p, 3)
            r["over_quantize_grouped"] = round(us_c / us_p, 3)
            r["marginal_us_per_candidate"] = round((us_c - us_p) / steps, 3) if steps > 1 else None
            print(f"    clipped / quantize_grouped = {r['over_quantize_grouped']:.3f}, {r['marginal_us_per_candidate']} us per candidate", flush=True)
            rows.append(r)
        del xs, outs, sc, zs
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rotate-gb", type=float, default=3.3)
    ap.add_argument("--rows", choices=("all", "reduce", "ef", "reduce_ef", "ef_f32r", "reduce_ef_f32r", "requant", "dequant_sum", "rot", "rot_reduce", "rot_ef",
                                       "rot_batch", "clip"), default="all")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, help="rot_batch rows: kernel statistics CSV of tools/grouped_rot_batch_workload.py under rocprofv3")
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / {"all": "grouped_bench.json", "reduce": "grouped_reduce_bench.json", "ef": "grouped_ef_bench.json",
                                                   "reduce_ef": "grouped_reduce_ef_bench.json", "ef_f32r": "grouped_ef_f32r_bench.json",
                                                   "reduce_ef_f32r": "grouped_reduce_ef_f32r_bench.json", "requant": "grouped_requant_bench.json",
                                                   "dequant_sum": "grouped_dequant_sum_bench.json", "rot": "grouped_rot_bench.json",
                                                   "rot_reduce": "grouped_rot_reduce_bench.json", "rot_ef": "grouped_rot_ef_bench.json",
                                                   "rot_batch": "grouped_rot_batch_bench.json", "clip": "grouped_clip_bench.json"}[args.rows])
    assert torch.cuda.is_available(), "grouped_bench measures on the GPU; there is nothing to measure without one"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    ctx = piquant.Context.get(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_blocking(False)
    ctx.assume_device_pointers(True)
    rows = []
    if args.rows == "reduce":
        rows = reduce_rows(ctx, dev, stream, args)
    if args.rows == "ef":
        rows = ef_rows(ctx, dev, stream, args)
    if args.rows == "reduce_ef":
        rows = reduce_ef_rows(ctx, dev, stream, args)
    if args.rows == "ef_f32r":
        rows = ef_f32r_rows(ctx, dev, stream, args)
    if args.rows == "reduce_ef_f32r":
        rows = reduce_ef_f32r_rows(ctx, dev, stream, args)
    if args.rows == "requant":
        rows = requant_rows(ctx, dev, stream, args)
    if args.rows == "dequant_sum":
        rows = dequant_sum_rows(ctx, dev, stream, args)
    if args.rows == "rot":
        rows = rot_rows(ctx, dev, stream, args)
    if args.rows == "rot_reduce":
        rows = rot_reduce_rows(ctx, dev, stream, args)
    if args.rows == "rot_ef":
        rows = rot_ef_rows(ctx, dev, stream, args)
    if args.rows == "rot_batch":
        rows = rot_batch_rows(ctx, dev, stream, args)
    if args.rows == "clip":
        rows = clip_rows(ctx, dev, stream, args)
    for fname, (fdt, tdt, esize) in (FLOAT.items() if args.rows == "all" else ()):
        nbuf = max(3, int(args.rotate_gb * 1e9 / (NUMEL * esize)) + 1)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        xs = [torch.empty(NUMEL, dtype=tdt, device=dev).normal_(generator=g) for _ in range(nbuf)]
        per_window = max(2 * nbuf, 64)
        for qname, (qdt, bits) in QUANT.items():
            pair = f"{fname}->{qname}"
            nq = qdt.packed_nbytes(NUMEL)
            outs = [torch.empty(nq, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            rec = [torch.empty(16, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            scale, zp = pt.compute_quant_params(xs[0], dtype={8: torch.uint8, 4: torch.quint4x2, 2: torch.quint2x4}[bits])
            us, s = timed(lambda i: ctx.quantize_ptr(xs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, scale, zp, piquant.RoundMode.NEAREST,
                                                     _device_ptrs=True, uniform=True), nbuf, args.windows, per_window, stream)
            rows.append(row("quantize_uniform", pair, 0, us, NUMEL * esize + nq, s))
            us, s = timed(lambda i: (ctx.compute_quant_params_device_ptr(xs[i].data_ptr(), fdt, NUMEL, qdt, rec[i].data_ptr(), _device_ptrs=True),
                                     ctx.quantize_dp_ptr(xs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, rec[i].data_ptr(), piquant.RoundMode.NEAREST,
                                                         _device_ptrs=True)), nbuf, args.windows, per_window, stream)
            rows.append(row("scan+quantize", pair, 0, us, 2 * NUMEL * esize + nq, s))
            for G in GROUPS:
                ng = pt.num_groups(NUMEL, G)
                sc = [torch.empty(ng, dtype=torch.float32, device=dev) for _ in range(nbuf)]
                zs = [torch.empty(ng, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
                us, s = timed(lambda i: ctx.quantize_grouped_ptr(xs[i].data_ptr(), fdt, outs[i].data_ptr(), qdt, NUMEL, G, sc[i].data_ptr(), zs[i].data_ptr(),
                                                                 False, piquant.RoundMode.NEAREST, _device_ptrs=True), nbuf, args.windows, per_window, stream)
                rows.append(row("quantize_grouped", pair, G, us, NUMEL * esize + nq + 5 * ng, s))
                if G == 128:   # dequantize of the same pair, with this call's parameters
                    dpair = f"{qname}->{fname}"
                    ys = [torch.empty(NUMEL, dtype=tdt, device=dev) for _ in range(nbuf)]
                    us, s = timed(lambda i: ctx.dequantize_ptr(outs[i].data_ptr(), qdt, ys[i].data_ptr(), fdt, NUMEL, scale, zp, piquant.ReduceOp.SET,
                                                               _device_ptrs=True, uniform=True), nbuf, args.windows, per_window, stream)
                    rows.append(row("dequantize_uniform", dpair, 0, us, NUMEL * esize + nq, s))
                    us, s = timed(lambda i: ctx.dequantize_grouped_ptr(outs[i].data_ptr(), qdt, ys[i].data_ptr(), fdt, NUMEL, G, sc[i].data_ptr(),
                                                                       zs[i].data_ptr(), piquant.ReduceOp.SET, _device_ptrs=True),
                                  nbuf, args.windows, per_window, stream)
                    rows.append(row("dequantize_grouped", dpair, G, us, NUMEL * esize + nq + 5 * ng, s))
                    del ys
                del sc, zs
            del outs, rec
        del xs
        torch.cuda.empty_cache()
    if args.rows == "all":
        rows += reduce_ef_f32r_rows(ctx, dev, stream, args)
        rows += requant_rows(ctx, dev, stream, args)
        rows += dequant_sum_rows(ctx, dev, stream, args)
        rows += rot_ef_rows(ctx, dev, stream, args)
        rows += rot_batch_rows(ctx, dev, stream, args)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"numel": NUMEL, "device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS, "rotate_gb": args.rotate_gb,
                               "windows": args.windows, "rows": rows}, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
