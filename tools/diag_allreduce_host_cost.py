#!/usr/bin/env python3
"""HOST time of the three calls of the mesh all-reduce schedule (encode_batch for 7 peers, reduce_encode with 7 terms, decode_batch of 8 chunks) as
piquant.distributed issues them, on chunks so small that the GPU never is the bottleneck: what the schedule costs the launching thread.  Round 5: 220 us
through the tensor-level wrappers of piquant.torch (two slices and a dozen attribute checks per buffer), 67 us through the context's raw-pointer entry
points -- the kernels of an 8-way all-reduce of 109 MB take 72 us.
--wire grouped / mx: the same three calls on the grouped wire (uint8, groups of 128) and on the MX wire (FP8 E4M3), whose host side is
csrc/capi_grouped.cpp / capi_mx.cpp.  PIQUANT_HIP_LIBRARY names the build to measure (A/B of two builds: one process each, alternating)."""
import argparse, sys, time
sys.path.insert(0, "pi-quant_amd")
import torch, piquant, piquant.distributed as D
ap = argparse.ArgumentParser()
ap.add_argument("--wire", choices=("chunk", "grouped", "mx"), default="chunk")
ap.add_argument("--iters", type=int, default=500)
args = ap.parse_args()
ops = D._DeviceOps(piquant.Context())
n, W, G, FMT = 40000, 8, 128, "fp8_e4m3"
x = torch.empty(n * W, device="cuda").uniform_(-1, 1)
slot = 2 * n if args.wire != "chunk" else 16 + n   # a grouped record is n + 5 n / G bytes (+ padding), an MX one n + n / 32: both well under 2 n
bufs = torch.zeros(W * slot + 64, dtype=torch.uint8, device="cuda")
mine = torch.zeros(slot, dtype=torch.uint8, device="cuda")
chunks = [(i * n, (i + 1) * n) for i in range(W)]
rec = lambda j: bufs[j * slot: (j + 1) * slot]
xs = lambda js: [x[chunks[j][0]:chunks[j][1]] for j in js]
peers, everyone = list(range(1, W)), list(range(W))
if args.wire == "chunk":
    for j, (b, e) in enumerate(chunks):
        ops.encode(x[b:e], rec(j), torch.uint8, "nearest")
    def direct():
        ops.encode_batch(xs(peers), [rec(j) for j in peers], torch.uint8, "nearest")
        ops.reduce_encode([rec(i) for i in peers], xs([0])[0], mine, torch.uint8, "nearest")
        ops.decode_batch([rec(j) for j in everyone], xs(everyone), torch.uint8, "set")
elif args.wire == "grouped":
    def direct():
        ops.encode_batch_grouped(xs(peers), [rec(j) for j in peers], torch.uint8, "nearest", G)
        ops.reduce_encode_grouped([rec(i) for i in peers], xs([0])[0], mine, torch.uint8, "nearest", G)
        ops.decode_batch_grouped([rec(j) for j in everyone], xs(everyone), torch.uint8, "set", G)
    ops.encode_batch_grouped(xs([0]), [rec(0)], torch.uint8, "nearest", G)   # record 0 is only decoded: make it a record
else:
    def direct():
        ops.encode_batch_mx(xs(peers), [rec(j) for j in peers], FMT)
        ops.reduce_encode_mx([rec(i) for i in peers], xs([0])[0], mine, FMT)
        ops.decode_batch_mx([rec(j) for j in everyone], xs(everyone), "set", FMT)
    ops.encode_batch_mx(xs([0]), [rec(0)], FMT)
for _ in range(50): direct()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.iters): direct()
t1 = time.perf_counter()
torch.cuda.synchronize()
t2 = time.perf_counter()
print(f"host us per direct schedule ({args.wire} wire, 3 calls, 8 ranks, tiny chunks): {(t1 - t0) / args.iters * 1e6:.1f}; incl. drain {(t2 - t0) / args.iters * 1e6:.1f}")
