"""Inputs for the grouped kernels' rounding-step tests (tests/test_grouped_step_edges_cpu.py, tests/test_gpu_grouped_step_edges.py); numpy only.

grouped_quantize_chunk (csrc/grouped_kernels.hpp) picks one of two rounding steps per wave: the short one for a full chunk whose groups are all
"bounded" -- fl(max(|min|, |max|) * fl(1 / scale)) < 1e9 in float32 -- and the long one otherwise; misaligned buffers take a third, scalar one.
edge_tensor() lays whole groups out so that the same bits meet all of them:

  S  STEP_CHUNKS full chunks (chunk = NG * G elements of the pair's tile, chunk_elems) in which every group is bounded: the short step
  L  the same groups bit for bit, but in every chunk one group is replaced by an unbounded one: the long step for the whole chunk.  Where a
     tile has NG = 1 the chunk is that group.  Every third chunk of a tile with NG > 1 also gets a +-0 group
  T  a tail shorter than one chunk: S's groups 1 .. k again and the front of S's group 0; it ends inside a group with n % 4 in {1, 3}, so the
     last packed byte of a 4-bit or 2-bit output is partial.  A partial chunk takes the long step

Classes of S (all bounded):
  ties_rand, ties_fixed   scale s from TIE_SCALES, zero point z0 random / from {0, qmax // 2, qmax}; element 0 is -z0 s, element 1 (qmax - z0) s, the
                          others (k + f) s with k an integer and f from TIE_FRACTIONS, inside the group's range
  far_pos, far_neg        one-sided [c, c + w] and its mirror image, w a power of two, values c + j w / 4: the zero point clamps to 0 / qmax and every
                          code saturates.  c / w is the largest ratio at which the input type still represents c and c + w / 4, 0.84 2^22 for float32 (a product
                          of 0.9e9 for uint8) and 0.84 2^6 for bfloat16; 0.9e9 / qmax itself is out of reach: w would be below an ulp of c
  line_below              float32 -> uint8 only (no other pair has two distinct values whose product reaches 1e9): one-sided, the product is the
                          float just below 1e9.  The other pairs get one more ties_fixed group
  nan_among               a ties group with quiet and signaling NaNs of both signs among the numbers
  denormal_among          a ties group with denormals of both signs among the numbers
  zeros, const_near       +-0 only; the constant 3.25: both get the degenerate (1.0, qmax >> 1) and are bounded, so they sit here and take the short step
  ordinary                Gaussian, magnitude 10^uniform(-3, 3)
Replacements of L (all unbounded):
  pos_inf, neg_inf        an ordinary group holding one infinity
  all_nan                 nothing but NaNs, quiet and signaling
  const_far               the constant +-3e9: scale 1, product 3e9
  all_denormal            nothing but denormals below 2^-130: the scale is below 2^-128 and its reciprocal overflows
  unbounded_pos / _neg    float32 -> uint8 only: one-sided with c / w = 0.9 2^23, the product is 1.9e9 (4e9 would need w below one ulp of c)
  line_above              float32 -> uint8 only: the product is exactly 1e9 or the float just above it

Measured on the final generator (tests/test_grouped_step_edges_cpu.py prints them), seed 0, the range over G in {32, 128, 4096}: the share of S's
elements on a decision edge -- the model's nearest code changes when the element moves by one ulp of the input type --
  float32 -> uint8 14-18 %, uint4 18-21 %, uint2 17-18 %; bfloat16 -> uint8 41-49 %, uint4 22-26 %, uint2 15-24 %.
For float32 input 15-24 % of S's products x * fl(1 / scale) have a fractional part of exactly 0.5, 12-16 % of exactly 0.25 and 0.8-5 % of exactly 0.375
(bfloat16: 11-26 %, 8-20 % and 0.3-3 %).
"""
import numpy as np

F32, BF16 = 0, 1                      # the dtype codes of include/piquant_hip.h (and of oracle.py)
UINT2, UINT4, UINT8 = 2, 3, 4
BITS = {UINT2: 2, UINT4: 4, UINT8: 8}
QMAX = {UINT2: 3, UINT4: 15, UINT8: 255}
EPV = {F32: 4, BF16: 8}               # elements per 16-byte input vector

TIE_SCALES = (0.5, 1.0, 3.0, 2.0 ** -7, 1.5e-3, 96.0)
TIE_FRACTIONS = (0.5, -0.5, 0.25, 0.375, 0.75, 0.49999997, 0.50000006, 0.0)
STEP_CHUNKS = 10                      # chunks of S (and of L): one per class where a chunk is one group
TAIL_GROUPS = 5                       # at most this many whole groups in T

QNAN, SNAN, NEG_SNAN, NEG_QNAN = 0x7FC00000, 0x7F800001, 0xFF812345, 0xFFC10000


def chunk_elems(dt_in, qd, G):
    """NG * G of GroupedQuantTile<dt_in, bits, G> (csrc/grouped_kernels.hpp): what one wave quantizes"""
    epv = EPV[dt_in]
    ob = epv * BITS[qd] // 8
    v = G // epv
    rpg = 1 if v < 64 else v // 64
    nv_want = max(16 // ob, 4)
    return max(rpg, min(v, nv_want)) * 64 * epv


def narrow_bits(u32):
    """float32 bit patterns -> bfloat16 bit patterns: numbers round to nearest even; a NaN is cut and stays a NaN of its kind (signaling or quiet)"""
    u = np.asarray(u32, dtype=np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    t = u >> 16
    t = np.where((t & 0x7F) == 0, t | 1, t)
    return np.where(nan, t, r).astype(np.uint16)


def widen_bits(u16):
    return np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16


def values(bits):
    """the input's bits (uint32: float32, uint16: bfloat16) as float32 values"""
    return (bits if bits.dtype == np.uint32 else widen_bits(bits)).view(np.float32)


def unpack(q, qd, n):
    """packed bytes -> one code per element"""
    bits, per = BITS[qd], 8 // BITS[qd]
    codes = (np.asarray(q, dtype=np.uint8)[:, None] >> (np.arange(per, dtype=np.uint8) * bits)[None, :]) & ((1 << bits) - 1)
    return codes.reshape(-1)[:n]


def _f32bits(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32).copy()


def _ties(rng, G, qd, dt_in, z0=None):
    qmax = QMAX[qd]
    s = float(np.float32(rng.choice(TIE_SCALES)))
    z0 = int(rng.integers(0, qmax + 1)) if z0 is None else z0
    lo, hi = 0.0 - z0 * s, (qmax - z0) * s
    f = rng.choice(TIE_FRACTIONS, G)
    k = rng.integers(-z0, qmax - z0, G) + (f < 0)          # k + f stays inside the range: few elements are clipped onto a code's centre
    x = np.clip((k + f) * s, lo, hi)
    x[0], x[1] = lo, hi
    return _f32bits(x)


def _ties_rand(rng, G, qd, dt_in):
    return _ties(rng, G, qd, dt_in)


def _ties_fixed(rng, G, qd, dt_in):
    return _ties(rng, G, qd, dt_in, z0=int(rng.choice([0, QMAX[qd] // 2, QMAX[qd]])))


def _one_sided(rng, G, ratio4, sign, steps=(0, 1, 2, 3, 4)):
    """values (ratio4 + j) w / 4, j from steps (0 and 4 in front): c = ratio4 w / 4 and c + w are the extremes"""
    w = 2.0 ** int(rng.integers(-10, 11))
    x = (ratio4 + rng.choice(steps, G)) * (w / 4)
    x[0], x[1] = ratio4 * (w / 4), (ratio4 + 4) * (w / 4)
    return _f32bits(sign * x)


def _far_ratio4(qd, dt_in):
    cap = 2.0 ** 22 if dt_in == F32 else 2.0 ** 6          # c < cap w keeps w / 4 a whole number of ulps of c
    return int(round(min(0.9e9 / QMAX[qd], 0.84 * cap) * 4))


def _far_pos(rng, G, qd, dt_in):
    return _one_sided(rng, G, _far_ratio4(qd, dt_in), 1.0)


def _far_neg(rng, G, qd, dt_in):
    return _one_sided(rng, G, _far_ratio4(qd, dt_in), -1.0)


def _unbounded_pos(rng, G, qd, dt_in):
    return _one_sided(rng, G, int(0.9 * 2 ** 23) * 4, 1.0, steps=(0, 2, 4))


def _unbounded_neg(rng, G, qd, dt_in):
    return _one_sided(rng, G, int(0.9 * 2 ** 23) * 4, -1.0, steps=(0, 2, 4))


def line_product(ratio4, qmax=255):
    """fl(max|x| * fl(1 / scale)) of the one-sided group with c = ratio4 w / 4 (any power of two w): the epilogue's scale is float32(w / qmax)"""
    hi = np.float32(ratio4 + 4) * np.float32(0.25)
    inv = np.float32(1.0) / np.float32(1.0 / qmax)
    return np.float32(hi * inv)


def _line(rng, G, qd, below):
    assert qd == UINT8
    line = np.float32(1.0e9)
    want = (np.nextafter(line, np.float32(0)),) if below else (line, np.nextafter(line, np.float32(np.inf)))
    j0 = int(round(1.0e9 / 255 * 4))
    hits = [j for j in range(j0 - 64, j0 + 64) if line_product(j) in want]
    assert hits, "no one-sided float32 group lands on the 1e9 line"
    return _one_sided(rng, G, int(rng.choice(hits)), float(rng.choice([-1.0, 1.0])))


def _line_below(rng, G, qd, dt_in):
    return _line(rng, G, qd, True)


def _line_above(rng, G, qd, dt_in):
    return _line(rng, G, qd, False)


def _nan_among(rng, G, qd, dt_in):
    x = _ties(rng, G, qd, dt_in)
    x[2::7] = QNAN
    x[3::11] = SNAN
    x[5] = NEG_SNAN
    x[6::13] = NEG_QNAN
    return x


def _denormal_among(rng, G, qd, dt_in):
    x = _ties(rng, G, qd, dt_in)
    x[2::7] = 0x00010000
    x[3::11] = 0x80070000
    x[5] = 0x00000001
    x[6::13] = 0x807F0000
    x[9] = 0x007FFFFF
    return x


def _zeros(rng, G, qd, dt_in):
    return np.where(rng.integers(0, 2, G) == 0, 0x00000000, 0x80000000).astype(np.uint32)


def _const_near(rng, G, qd, dt_in):
    return np.full(G, np.float32(3.25).view(np.uint32), dtype=np.uint32)


def _ordinary(rng, G, qd, dt_in):
    return _f32bits(rng.standard_normal(G) * 10.0 ** rng.uniform(-3, 3))


def _with_inf(rng, G, qd, dt_in, bits):
    x = _ordinary(rng, G, qd, dt_in)
    x[int(rng.integers(0, G))] = bits
    return x


def _pos_inf(rng, G, qd, dt_in):
    return _with_inf(rng, G, qd, dt_in, 0x7F800000)


def _neg_inf(rng, G, qd, dt_in):
    return _with_inf(rng, G, qd, dt_in, 0xFF800000)


def _all_nan(rng, G, qd, dt_in):
    return rng.choice(np.array([QNAN, SNAN, NEG_SNAN, NEG_QNAN], dtype=np.uint32), G)


def _const_far(rng, G, qd, dt_in):
    return np.full(G, np.float32(rng.choice([-3.0e9, 3.0e9])).view(np.uint32), dtype=np.uint32)


def _all_denormal(rng, G, qd, dt_in):
    mag = rng.integers(1, 8, G).astype(np.uint32) << 16 if dt_in == BF16 else rng.integers(1, 2 ** 19, G).astype(np.uint32)
    return mag | (rng.integers(0, 2, G).astype(np.uint32) << 31)


_BUILD = {f.__name__[1:]: f for f in (_ties_rand, _ties_fixed, _far_pos, _far_neg, _line_below, _nan_among, _denormal_among, _zeros, _const_near, _ordinary,
                                      _pos_inf, _neg_inf, _all_nan, _const_far, _all_denormal, _unbounded_pos, _unbounded_neg, _line_above)}
TIE_CLASSES = ("ties_rand", "ties_fixed", "nan_among", "denormal_among")


def bounded_classes(dt_in, qd):
    line = "line_below" if (dt_in, qd) == (F32, UINT8) else "ties_fixed"
    return ["ties_rand", "ties_fixed", "far_pos", "nan_among", line, "denormal_among", "far_neg", "zeros", "ordinary", "const_near"]


def unbounded_classes(dt_in, qd):
    more = ["unbounded_pos", "line_above", "unbounded_neg"] if (dt_in, qd) == (F32, UINT8) else []
    return ["pos_inf", "all_nan", "const_far", "neg_inf", "all_denormal"] + more


class Layout:
    """n, G, chunk, NG; sections: name -> (first element, end); per group g: cls[g], section[g], origin[g] (the group of S whose bits it repeats, g
    itself in S, -1 for a replaced group)"""

    def __init__(self, n, G, chunk):
        self.n, self.G, self.chunk, self.NG = n, G, chunk, chunk // G
        self.sections, self.cls, self.section, self.origin = {}, [], [], []

    def bounds(self, g):
        return g * self.G, min((g + 1) * self.G, self.n)

    def groups_of(self, name):
        b, e = self.sections[name]
        return range(b // self.G, (e + self.G - 1) // self.G)

    def chunks_of(self, name):
        """the whole chunks of a section as ranges of groups"""
        b, e = self.sections[name]
        return [range(c // self.G, (c + self.chunk) // self.G) for c in range(b, e - self.chunk + 1, self.chunk)]

    def describe(self, g):
        return f"section {self.section[g]}, group {g} ({self.cls[g]})"

    def describe_element(self, i):
        return f"element {i} = " + self.describe(i // self.G) + f" + {i % self.G}"


def edge_tensor(dt_in, qd, G, seed):
    """-> (the input as bits: uint32 for float32, uint16 for bfloat16; its Layout)"""
    rng = np.random.default_rng([seed, dt_in, qd, G])
    chunk = chunk_elems(dt_in, qd, G)
    NG = chunk // G
    bounded, unbounded = bounded_classes(dt_in, qd), unbounded_classes(dt_in, qd)
    ns = STEP_CHUNKS * NG
    s_cls = bounded + [str(c) for c in rng.choice(bounded + list(TIE_CLASSES), ns - len(bounded))]
    s_groups = [_BUILD[c](rng, G, qd, dt_in) for c in s_cls]
    l_cls, l_groups, l_origin = list(s_cls), list(s_groups), list(range(ns))
    for c in range(STEP_CHUNKS):
        slots = rng.permutation(NG)
        for slot, name in zip(slots, [unbounded[(c + seed) % len(unbounded)]] + (["zeros"] if NG > 1 and c % 3 == 0 else [])):
            g = c * NG + int(slot)
            l_cls[g], l_groups[g], l_origin[g] = name, _BUILD[name](rng, G, qd, dt_in), -1
    k = min(NG - 1, TAIL_GROUPS)
    part = G // 2 + (1 if seed % 2 == 0 else 3)
    t_origin = list(range(1, k + 1)) + [0]
    t_groups = [s_groups[g] for g in t_origin]
    t_groups[-1] = t_groups[-1][:part]
    bits = np.concatenate(s_groups + l_groups + t_groups).astype(np.uint32)
    lay = Layout(bits.size, G, chunk)
    lay.sections = {"S": (0, ns * G), "L": (ns * G, 2 * ns * G), "T": (2 * ns * G, bits.size)}
    lay.cls = s_cls + l_cls + [s_cls[g] for g in t_origin]
    lay.section = ["S"] * ns + ["L"] * ns + ["T"] * (k + 1)
    lay.origin = list(range(ns)) + l_origin + t_origin
    assert bits.size % 4 in (1, 3) and bits.size - lay.sections["T"][0] < chunk
    return (narrow_bits(bits) if dt_in == BF16 else bits), lay


def bounded_by_product_rule(lo, hi, scales):
    """the kernels' per-group test for the short step, in float32: fl(max(|min|, |max|) * fl(1 / scale)) < 1e9"""
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / np.asarray(scales, dtype=np.float32)
        prod = np.maximum(np.abs(np.asarray(lo, dtype=np.float32)), np.abs(np.asarray(hi, dtype=np.float32))) * inv
        return prod.astype(np.float32) < np.float32(1.0e9)
