"""The committed cases of the per-group clip search (tests/clip_model.py has the definition): the data the CPU tests prove their wrong variants on
and the edge groups the GPU tests run.  Everything is generated from fixed seeds or written out, so a case is the same array everywhere.

A case is (name, float32 values); `as_input` turns the values into the tensor of a pair's input type.  `EDGE_GROUPS` are single groups of 32
elements each, laid end to end by `edge_tensor` (G = 32: one group each; a larger G sees other groups, which is fine -- the model decides).
"""
import numpy as np

import oracle as O

PAIRS = [(O.F32, O.UINT8), (O.F32, O.UINT4), (O.F32, O.UINT2), (O.BF16, O.UINT8), (O.BF16, O.UINT4), (O.BF16, O.UINT2)]
GROUP_SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096]
ESIZE = {O.F32: 4, O.BF16: 2}
BITS = {O.UINT8: 8, O.UINT4: 4, O.UINT2: 2}
QMAX = {O.UINT8: 255, O.UINT4: 15, O.UINT2: 3}


def as_input(values: np.ndarray, dt_in: int) -> np.ndarray:
    v = np.ascontiguousarray(values, dtype=np.float32)
    return O.f32_to_bf16(v) if dt_in == O.BF16 else v


def chunk_elems(dt_in: int, qd: int, G: int) -> int:
    """Elements of one wave's chunk of the streaming tile (GroupedQuantTile, csrc/grouped_kernels.hpp), restated."""
    epv = 16 // ESIZE[dt_in]
    ob = epv * BITS[qd] // 8
    v = G // epv
    rpg = 1 if v < 64 else v // 64
    want = max(16 // ob, 4)
    nv = max(rpg, min(v, want))
    return nv * 64 * epv


def spiky_gaussian(n: int, seed: int, G: int) -> np.ndarray:
    """Seeded N(0, 1), every group scaled by its own power of two, with one large element (1 to 6) in two groups of three: the best range
    differs from group to group, so the choices spread over several k."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    for g in range(n // G):
        x[g * G:(g + 1) * G] *= np.float32(2.0 ** -int(rng.integers(0, 5)))
        if g % 3 == 2:
            continue
        i = g * G + int(rng.integers(0, G))
        x[i] = np.float32((1.0 if rng.integers(0, 2) else -1.0) * rng.uniform(1.0, 6.0))
    return x


# An exact tie between two candidates at the minimum, uint2 from float32 or bfloat16, G = 32: lo = -24, hi = 24, so candidate k has
# scale (48 - 3 k) / 3 = 16 - k and zero point 2 exactly, every dequantized value and every error is a small integer, and every sum is exact.
# tests/clip_model.py asserts E[TIE_KS[0]] == E[TIE_KS[1]] == min E on it, so that the case cannot silently stop being a tie.
TIE_GROUP = np.array([-24, 24, 8, 12, 21, 14, 23, -24, -20, -17, -18, -20, -19, -7, 3, -7, -22, 12, 2, 11, 18, 19, -2, 9, -13, 5, 11, 24, -8, 7, -14, -5],
                     dtype=np.float32)
TIE_KS = (1, 4)   # E_1 == E_4 == 891 is the minimum of the nine candidates: strict `<` keeps 1


def near_tie_group(G: int, m: int, permute_second_half: bool = False) -> np.ndarray:
    """TIE_GROUP tiled to G elements and scaled by 1 + m / 1024: nothing is exact any more, E_1 and E_4 differ by an ulp or two, and which of them
    is smaller depends on the order of the sum.  permute_second_half: the same multiset in another order there, so that rows differ."""
    v = np.tile(TIE_GROUP, G // 32)
    if permute_second_half:
        v[G // 2:] = v[G // 2:][np.random.default_rng(3).permutation(G // 2)]
    return (v * np.float32(1.0 + m / 1024.0)).astype(np.float32)


def grid_group(G: int, qd: int, k: int, seed: int) -> np.ndarray:
    """A group built so that candidate k can win on ANY wire, uint8 included.  lo = -8 qmax, hi = 8 qmax: candidate j has scale 16 - j and zero
    point (qmax + 1) / 2 exactly, every error is a small integer and every sum exact.  The bulk lies on candidate k's grid -- multiples of 16 - k,
    those farthest from the grids of the candidates before k (for k = 1 the half-steps of candidate 0's grid: error 8 each) -- so candidate k pays
    only for clipping the two extremes, about 2 (qmax k / 2)^2, and gains up to 64 an element.  The price grows with qmax^2: on uint8 candidate 1
    needs G >= 512 and candidate 2 G >= 2048 (grid_min_choices)."""
    Q = QMAX[qd]
    rng = np.random.default_rng(seed)
    v = np.arange(-(Q + 1) // 2, (Q - 1) // 2 + 1) * (16 - k)
    if k:
        score = np.min([np.abs(v - (16 - j) * np.round(v / (16.0 - j))) for j in range(k)], axis=0)
        v = v[score == score.max()]
    x = rng.choice(v, G).astype(np.float32)
    x[0], x[1] = -8 * Q, 8 * Q
    return x


GRID_TARGETS = (0, 1, 2, 3, 4, 1, 2)


def grid_tensor(G: int, qd: int, tail: int = 3) -> np.ndarray:
    """grid_group for the targets 0, 1, 2, 3, 4, 1, 2 end to end, then a ragged group"""
    return np.concatenate([grid_group(G, qd, k, 10 * G + k) for k in GRID_TARGETS] + [np.full(tail, 5.0, dtype=np.float32)])


def grid_min_choices(qd: int, G: int) -> int:
    """Distinct k the model must choose on grid_tensor (the tests assert it).  Three on every wire and group size but uint8 below G = 2048: there a
    bulk element gains at most (s / 2)^2 = 64 against candidate 0 (s = 16 its step), and clipping the extremes +-2040 costs candidate 1
    120^2 + 135^2 - 128 = 32 497 and candidate 2 248^2 + 262^2 - 128 = 130 020 more than candidate 0: no k > 0 below G = 510, no k > 1 below 2034."""
    if qd != O.UINT8 or G >= 2048:
        return 3
    return 2 if G >= 512 else 1


def _edge_groups():
    rng = np.random.default_rng(20240607)
    g = lambda: rng.standard_normal(32).astype(np.float32)   # noqa: E731
    groups = []
    groups.append(("all_nan", np.full(32, np.nan, dtype=np.float32)))
    x = g(); x[5] = np.nan
    groups.append(("one_nan", x))
    x = g(); x[0] = np.nan; x[31] = np.nan; x[7] = 6.0
    groups.append(("nan_at_both_ends_and_a_spike", x))
    x = g(); x[9] = np.inf
    groups.append(("plus_inf", x))
    x = g(); x[30] = -np.inf
    groups.append(("minus_inf", x))
    groups.append(("constant", np.full(32, 1.25, dtype=np.float32)))
    x = np.zeros(32, dtype=np.float32); x[1::2] = -0.0
    groups.append(("signed_zeros", x))
    groups.append(("denormal_range", (rng.integers(-40, 41, 32) * np.float32(1.4e-45)).astype(np.float32)))
    groups.append(("tiny_normal_range", (rng.standard_normal(32) * 3e-38).astype(np.float32)))
    groups.append(("all_positive", (np.abs(g()) + np.float32(0.5)).astype(np.float32)))
    x = (np.abs(g()) + np.float32(0.5)).astype(np.float32); x[3] = 9.0
    groups.append(("all_positive_spike", x))
    groups.append(("all_negative", (-np.abs(g()) - np.float32(0.25)).astype(np.float32)))
    x = (-np.abs(g()) - np.float32(0.25)).astype(np.float32); x[17] = -7.5
    groups.append(("all_negative_spike", x))
    groups.append(("tie", TIE_GROUP.copy()))
    # The short step's bound max(|lo|, |hi|) / scale_k < 10^9 holds for candidate 0 and fails for the later ones ON A uint8 WIRE: lo = 2^23,
    # hi = lo + 3 gives 2^23 * 255 / (3 r_k) = 7.1e8 at k = 0 and above 10^9 from k = 5 on (clip_model.assert_crosses_short_step_line).  No group
    # crosses on a narrower wire: hi - lo is at least one ulp of the larger extreme, so the ratio stays below qmax * 2^24 / r_11 = 8.1e8 (uint4),
    # and bfloat16's ulp is 2^-8 of the value (qmax * 2^8 / r_11 = 2.1e5 for uint8): float32 -> uint8 is the only pair that has such a group.
    x = np.full(32, 8388608.0, dtype=np.float32); x[4::3] = 8388609.0; x[11] = 8388610.0; x[20] = 8388611.0
    groups.append(("short_long_line_uint8", x))
    groups.append(("huge_range", (g() * np.float32(1e37)).astype(np.float32)))
    x = g(); x[13] = 40.0
    groups.append(("big_spike", x))
    groups.append(("plain", g()))
    return groups


EDGE_GROUPS = _edge_groups()


def edge_tensor(tail: int = 5) -> np.ndarray:
    """Every edge group end to end, then a ragged group of `tail` elements with a spike (it must not be searched)."""
    rng = np.random.default_rng(7)
    t = rng.standard_normal(tail).astype(np.float32)
    if tail:
        t[0] = 11.0
    return np.concatenate([v for _, v in EDGE_GROUPS] + [t])


# The cases the CPU test proves its wrong variants on: (name, dt_in, qd, G, steps, values)
def variant_cases():
    cases = [
        ("gauss_f32_u2_G128", O.F32, O.UINT2, 128, 9, spiky_gaussian(16 * 128 + 37, 11, 128)),
        ("gauss_f32_u4_G32", O.F32, O.UINT4, 32, 9, spiky_gaussian(64 * 32 + 3, 12, 32)),
        ("gauss_bf16_u4_G128", O.BF16, O.UINT4, 128, 9, spiky_gaussian(16 * 128, 13, 128)),
        ("gauss_bf16_u2_G64", O.BF16, O.UINT2, 64, 12, spiky_gaussian(32 * 64 + 9, 14, 64)),
        ("rows_f32_u4_G1024", O.F32, O.UINT4, 1024, 9, spiky_gaussian(6 * 1024, 15, 1024)),
        ("rows_bf16_u2_G2048", O.BF16, O.UINT2, 2048, 9, spiky_gaussian(4 * 2048, 16, 2048)),
        ("ragged_f32_u2_G128", O.F32, O.UINT2, 128, 9, np.concatenate([spiky_gaussian(2 * 128, 17, 128), spiky_gaussian(128, 18, 128)[:100]])),
        ("edges_f32_u2_G32", O.F32, O.UINT2, 32, 9, edge_tensor()),
        ("edges_bf16_u2_G32", O.BF16, O.UINT2, 32, 9, edge_tensor()),
        ("edges_f32_u8_G32", O.F32, O.UINT8, 32, 12, edge_tensor()),
        ("grid_f32_u8_G2048", O.F32, O.UINT8, 2048, 9, grid_tensor(2048, O.UINT8)),
        ("grid_bf16_u8_G4096", O.BF16, O.UINT8, 4096, 9, grid_tensor(4096, O.UINT8)),
        ("grid_f32_u8_G512", O.F32, O.UINT8, 512, 9, grid_tensor(512, O.UINT8)),
        ("grid_f32_u4_G32", O.F32, O.UINT4, 32, 9, grid_tensor(32, O.UINT4)),
        ("grid_bf16_u4_G64", O.BF16, O.UINT4, 64, 9, grid_tensor(64, O.UINT4)),
        ("near_tie_f32_u2_G512", O.F32, O.UINT2, 512, 9, np.concatenate([near_tie_group(512, m) for m in (349, 373, 341)])),
        ("near_tie_rows_f32_u2_G512", O.F32, O.UINT2, 512, 9, np.concatenate([near_tie_group(512, m, True) for m in (2, 41, 53)])),
    ]
    return cases
