"""GPU: bench.py's plain run (the headline alone, K timed steps) and what --dump-outputs writes."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_plain_bench_is_the_headline_alone_and_dumps_the_last_step(oracle_mod, tmp_path):
    """`bench.py --steps 20 --warmup 5 --dump-outputs DIR`: one JSON line with the headline fields and nothing measured beside it, exactly 20 timed
    steps, and DIR holds the output of the last timed step (buffer set 19 of the rotation) -- a seeded sample, its indices, the histogram of the
    whole output, (scale, zero_point) -- in float32 / float64 within 64 MB, byte for byte what the checker makes of the same input."""
    O = oracle_mod
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["steps"] == 20 and d["warmup"] == 5 and d["timed_windows"]["count"] == 1 and d["timed_windows"]["steps_each"] == 20
    assert abs(d["value"] - 27_264_000 * 4 / 2**30 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    assert not {"extras", "cpu_baseline", "shard_bit_exact", "self_check"} & set(d), sorted(d)

    files = {p.name: np.load(p) for p in out.glob("*.npy")}
    assert set(files) == {"quantized.npy", "quantized_index.npy", "quantized_histogram.npy", "quant_params.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(p.stat().st_size for p in out.glob("*.npy")) <= 64 << 20
    n = d["config"]["numel_total"]
    idx = files["quantized_index.npy"].astype(np.int64)
    assert idx.size == files["quantized.npy"].size and np.all(np.diff(idx) > 0) and idx[0] == 0 and idx[-1] == n - 1
    assert files["quantized_histogram.npy"].shape == (256,) and files["quantized_histogram.npy"].sum() == n

    def bench_input(s):      # bench.py's buffer set s on rank 0
        g = torch.Generator(device="cuda")
        g.manual_seed(s)
        return torch.empty(n, dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=g).cpu().numpy()

    scale, zp = O.compute_quant_params(bench_input(0), O.F32, O.UINT8)      # the parameters of tensor 0 serve every set
    assert files["quant_params.npy"].tolist() == [scale, zp] == [d["config"]["scale"], d["config"]["zero_point"]]
    want = O.quantize(bench_input(19), O.F32, O.UINT8, scale, zp)
    assert np.array_equal(files["quantized.npy"], want[idx].astype(np.float32))
    assert np.array_equal(files["quantized_histogram.npy"], np.bincount(want, minlength=256).astype(np.float64))
