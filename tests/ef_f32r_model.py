"""CPU model of error-feedback group-wise quantization of a bfloat16 tensor with a FLOAT32 residual (piquant_hip_quantize_grouped_ef_mixed).

The definition is a composition: the float32 error-feedback step (tests/ef_model.py) on the widened tensor.  x is bf16 bit patterns (uint16),
r a float32 array:
  1. y = rn_f32(widen(x) + r)
  2. (q, scales, zero points) = quantize_grouped(y) in the float32 pipeline, computed parameters
  3. d = dequantize_grouped(q, scales, zero points) in float32 (SET)
  4. r <- rn_f32(y - d)
No arithmetic of its own."""
import oracle as O
from ef_model import ef_step, widen


def ef_f32r_step(x_bf16, r_f32, qd, G, round_mode=O.NEAREST, threshold=0.0, quantize=None):
    """-> (packed bytes, scales, zero points, new float32 residual, y, d), y and d float32; x_bf16 and r_f32 are not modified.  quantize: as in
    tests/ef_model.py's ef_step."""
    return ef_step(widen(x_bf16, O.BF16), r_f32, O.F32, qd, G, round_mode, threshold, quantize)
