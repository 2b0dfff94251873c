"""CPU: the grouped dequantize-sum -- the symbol is declared and exported, the Python surface exists and refuses bad arguments with ValueError
before a native call could abort (tests/test_gpu_grouped_dequant_sum.py runs the kernel)."""
import re
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
SYMBOL = "piquant_hip_dequantize_sum_grouped"


def test_symbol_is_declared_and_exported():
    header = (ROOT / "include" / "piquant_hip.h").read_text()
    assert re.search(r"PIQUANT_EXPORT\s+void\s+" + SYMBOL + r"\s*\(", header), f"{SYMBOL} is not declared in piquant_hip.h"
    import piquant
    import piquant.distributed as D
    import piquant.torch as pt
    from piquant._bootstrap import C_LIB, library_path

    assert len(getattr(C_LIB, SYMBOL).argtypes) == 11
    nm = subprocess.run(["nm", "-D", "--defined-only", str(library_path())], capture_output=True, text=True, check=True).stdout
    assert SYMBOL in {line.split()[-1] for line in nm.splitlines() if line.strip()}, f"libpiquant.so does not export {SYMBOL}"
    assert callable(piquant.Context.dequantize_sum_grouped_ptr) and callable(pt.dequantize_sum_grouped)
    assert callable(D.quantized_reduce_scatter) and callable(D.quantized_all_gather) and callable(D._DeviceOps.decode_sum_grouped)


def test_torch_wrapper_refuses_bad_arguments():
    """Host tensors throughout: nothing here touches a device."""
    import piquant.torch as pt

    q = torch.zeros(1000, dtype=torch.uint8)
    s, z = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    kw = dict(dtype=torch.float32, group_size=128)
    with pytest.raises(ValueError, match="at least one"):
        pt.dequantize_sum_grouped([], [], [], **kw)
    with pytest.raises(ValueError, match="same length"):
        pt.dequantize_sum_grouped([q, q], [s], [z, z], **kw)
    with pytest.raises(ValueError, match="same length"):
        pt.dequantize_sum_grouped([q], [s, s], [z], **kw)
    for bad in (100, 16, 8192, None, 128.0, True):
        with pytest.raises(ValueError, match="group_size"):
            pt.dequantize_sum_grouped([q], [s], [z], dtype=torch.float32, group_size=bad)
    with pytest.raises(ValueError, match="accumulates into out"):
        pt.dequantize_sum_grouped([q], [s], [z], reduce_op="add", **kw)
    with pytest.raises(ValueError, match="reduce_op"):
        pt.dequantize_sum_grouped([q], [s], [z], reduce_op="mul", **kw)
    with pytest.raises(ValueError, match="float dtype"):
        pt.dequantize_sum_grouped([q], [s], [z], dtype=torch.uint8, group_size=128)
    with pytest.raises(ValueError, match="float dtype"):
        pt.dequantize_sum_grouped([q], [s], [z], dtype=torch.float16, group_size=128)
    with pytest.raises(ValueError, match="quantized tensor"):
        pt.dequantize_sum_grouped([torch.zeros(1000)], [s], [z], **kw)
    with pytest.raises(ValueError, match="ROCm"):
        pt.dequantize_sum_grouped([q], [s], [z], **kw)   # everything matches, but host tensors
