#!/usr/bin/env python3
"""Per-rank KERNEL time of a quantized all-reduce (no wire): the sequence of encode / decode / dequantize_sum calls one rank
issues for a `world`-way all-reduce of an fp32 tensor, replayed on one GPU with stand-in receive buffers.  Shows what the
schedules cost in HBM time next to the xGMI transfer time they overlap with (per-link ~153 GB/s, guides/MI355X_MICROARCH.md).
With --group-size G the same rank's schedules on the grouped wire (quantized_all_reduce(group_size=G): quantize_grouped, reduce_quantize_grouped,
dequantize_grouped and their batches) are replayed in the same run, next to the per-chunk-parameter ones.

  python tools/all_reduce_compute_cost.py [--numel 27264000] [--world 8] [--group-size 128] [--out FILE]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pi-quant_amd"))

import torch  # noqa: E402

import piquant  # noqa: E402
import piquant.distributed as D  # noqa: E402

HEADER = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=27_264_000)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--group-size", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, n = args.world, args.numel
    dev = torch.device("cuda")
    ops = D._DeviceOps(piquant.Context())
    x = torch.empty(n, device=dev).uniform_(-1, 1)
    out = {"numel": n, "world": W}
    for qname, bits in (("uint8", 8), ("quint4x2", 4)):
        qdt = getattr(torch, qname)
        chunks = D.ring_chunks(n, W, bits)
        nbytes = [HEADER + piquant.DataType.UINT8.packed_nbytes(e - b) if bits == 8 else HEADER + piquant.DataType.UINT4.packed_nbytes(e - b) for b, e in chunks]
        slot = -(-max(nbytes) // 16) * 16
        bufs = torch.zeros(W * slot, dtype=torch.uint8, device=dev)
        mine = torch.zeros(slot, dtype=torch.uint8, device=dev)
        for j, (b, e) in enumerate(chunks):          # valid wire content in every slot
            ops.encode(x[b:e], bufs[j * slot: j * slot + nbytes[j]], qdt, "nearest")

        def ring():
            ops.encode(x[chunks[0][0]:chunks[0][1]], bufs[0: nbytes[0]], qdt, "nearest")
            for step in range(W - 1):                # reduce-scatter hops: add what arrives, forward the re-quantized sum (one launch)
                r = (0 - step - 1) % W
                ops.reduce_encode([bufs[r * slot: r * slot + nbytes[r]]], x[chunks[r][0]:chunks[r][1]], mine[: nbytes[r]], qdt, "nearest")
            for j in range(W):                       # all-gather: every chunk decoded once
                ops.decode(bufs[j * slot: j * slot + nbytes[j]], x[chunks[j][0]:chunks[j][1]], qdt, "set")

        def direct():
            peers = list(range(1, W))                # one launch quantizes the chunk of every peer
            ops.encode_batch([x[chunks[j][0]:chunks[j][1]] for j in peers], [bufs[j * slot: j * slot + nbytes[j]] for j in peers], qdt, "nearest")
            ops.reduce_encode([bufs[i * slot: i * slot + nbytes[0]] for i in range(1, W)], x[chunks[0][0]:chunks[0][1]], mine[: nbytes[0]], qdt, "nearest")
            ops.decode_batch([bufs[j * slot: j * slot + nbytes[j]] for j in range(W)], [x[chunks[j][0]:chunks[j][1]] for j in range(W)], qdt, "set")

        schedules = [("", ring, direct, max(nbytes))]
        G = args.group_size
        if G is not None:
            gbytes = [D.grouped_wire_layout(e - b, G, bits).nbytes for b, e in chunks]
            gslot = -(-max(gbytes) // 16) * 16
            gbufs = torch.zeros(W * gslot, dtype=torch.uint8, device=dev)
            gmine = torch.zeros(gslot, dtype=torch.uint8, device=dev)
            for j, (b, e) in enumerate(chunks):
                ops.encode_grouped(x[b:e], gbufs[j * gslot: j * gslot + gbytes[j]], qdt, "nearest", G)

            def ring_grouped():
                ops.encode_grouped(x[chunks[0][0]:chunks[0][1]], gbufs[0: gbytes[0]], qdt, "nearest", G)
                for step in range(W - 1):
                    r = (0 - step - 1) % W
                    ops.reduce_encode_grouped([gbufs[r * gslot: r * gslot + gbytes[r]]], x[chunks[r][0]:chunks[r][1]], gmine[: gbytes[r]], qdt, "nearest", G)
                for j in range(W):
                    ops.decode_grouped(gbufs[j * gslot: j * gslot + gbytes[j]], x[chunks[j][0]:chunks[j][1]], qdt, "set", G)

            def direct_grouped():
                peers = list(range(1, W))
                ops.encode_batch_grouped([x[chunks[j][0]:chunks[j][1]] for j in peers], [gbufs[j * gslot: j * gslot + gbytes[j]] for j in peers], qdt,
                                         "nearest", G)
                ops.reduce_encode_grouped([gbufs[i * gslot: i * gslot + gbytes[0]] for i in range(1, W)], x[chunks[0][0]:chunks[0][1]], gmine[: gbytes[0]],
                                          qdt, "nearest", G)
                ops.decode_batch_grouped([gbufs[j * gslot: j * gslot + gbytes[j]] for j in range(W)], [x[chunks[j][0]:chunks[j][1]] for j in range(W)],
                                         qdt, "set", G)

            schedules.append((f"grouped{G}_", ring_grouped, direct_grouped, max(gbytes)))

        row = {}
        for prefix, ring_fn, direct_fn, chunk_wire in schedules:
            for name, fn in (("ring", ring_fn), ("direct", direct_fn)):
                x.uniform_(-1, 1)
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    fn()
                    torch.cuda.synchronize()
                    with torch.cuda.graph(g, stream=s):
                        fn()
                    g.replay()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                row[prefix + name + "_kernel_us_per_all_reduce"] = round(e0.elapsed_time(e1) * 1e3 / 20, 1)
                x.uniform_(-1, 1)                        # values drift under repeated accumulation; irrelevant for timing
            row[prefix + "wire_bytes_per_rank"] = 2 * (W - 1) * chunk_wire
            row[prefix + "xgmi_us_ring_one_link_153GBps"] = round(2 * (W - 1) * chunk_wire / 153e9 * 1e6, 1)
            row[prefix + "xgmi_us_mesh_all_links"] = round(2 * chunk_wire / 153e9 * 1e6, 1)
        if G is not None:
            row["grouped_direct_over_per_chunk"] = round(row[f"grouped{G}_direct_kernel_us_per_all_reduce"] / row["direct_kernel_us_per_all_reduce"], 3)
            row["grouped_wire_over_per_chunk"] = round(row[f"grouped{G}_wire_bytes_per_rank"] / row["wire_bytes_per_rank"], 4)
        out[qname] = row
    print(json.dumps(out, indent=1))
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
