"""CPU: the position lists of tests/extremum_positions.py do what they claim, and the host scans find an extremum wherever it is.

1. The launch constants that extremum_positions mirrors equal the C++ headers' (a retune must look at the sweeps).
2. For every kernel family a numpy restatement of its index mapping folds every element exactly when nothing is removed, and for every
   single-fault model -- a lane, a slot k, a round class, a resident round, a row, an element of a vector, the head, the tail, a block, the
   clamped last vector, a wave-skipped slot -- at least one listed position is among the elements the faulty mapping no longer folds: with
   the extremum planted there the faulty kernel's result differs.
3. The sweep itself on the host companion (libpiquant_cpu.so: AVX-512 and scalar scans behind the thread pool's partitions) and on the
   checker (oracle.minmax against numpy.min / numpy.max): every position of a tensor of a few thousand elements.
"""
from pathlib import Path

import numpy as np
import pytest

import extremum_positions as X

CSRC = Path(__file__).resolve().parent.parent / "pi-quant_amd" / "csrc"
CUS = 256   # the geometry checks run for an MI355X's 256 CUs and for a small device


def test_mirrored_constants_equal_the_headers():
    found = X.constants_in(CSRC / "tuning.hpp", CSRC / "grouped_kernels.hpp")
    for name, value in X.MIRRORED.items():
        assert name in found, f"{name} is no longer a `constexpr int` of csrc/tuning.hpp or csrc/grouped_kernels.hpp"
        assert found[name] == value, f"{name} is {found[name]} in the headers and {value} in tests/extremum_positions.py: check the sweeps, then update MIRRORED"
    minmax = (CSRC / "minmax_kernels.hpp").read_text()
    fused = (CSRC / "fused_kernels.hpp").read_text()
    kernels = (CSRC / "kernels.hip").read_text()
    hint = "tests/extremum_positions.py mirrors `{}` of csrc/{}, which is no longer there as written: look at what changed, check the sweeps' geometry, then update {} and this text"
    for text, name, line, mirrored in (
            (minmax, "minmax_kernels.hpp", f"constexpr int kMinmaxGatherMax = {X.GATHER_MAX};", "GATHER_MAX"),
            (minmax, "minmax_kernels.hpp", "constexpr int LPL = 8;", "GATHER_ONE_WAVE"),
            (minmax, "minmax_kernels.hpp", "G - 1 <= 64u * LPL", "GATHER_ONE_WAVE"),
            (fused, "fused_kernels.hpp", f"constexpr int kFusedMaxBlocks = {X.F_MAX_BLOCKS};", "F_MAX_BLOCKS"),
            (fused, "fused_kernels.hpp", f"int STREAM_BATCH = {X.F_STREAM_BATCH},", "F_STREAM_BATCH"),
            (kernels, "kernels.hip", f"capped_grid((numel + kMinmaxBlock - 1) / kMinmaxBlock, {X.SCALAR_BLOCKS_PER_CU}, num_cu)", "SCALAR_BLOCKS_PER_CU")):
        assert line in text, hint.format(line, name, mirrored)
    assert X.GATHER_ONE_WAVE == 64 * 8


def test_pairs_visit_every_position_in_both_roles_and_never_share_one():
    for n in (4, 5, 64, 1001):
        p = np.arange(n) * 3
        pairs = X.pair_up(p)
        assert sorted(pairs[:, 0]) == sorted(p) and sorted(pairs[:, 1]) == sorted(p)
        assert (pairs[:, 0] != pairs[:, 1]).all()
        nxt = np.roll(pairs, -1, axis=0)   # what the next launch plants never lands on what this launch's restore writes
        assert all(len({a, b, c, d}) == 4 for (a, b), (c, d) in zip(pairs, nxt))
    bg = X.background(10_000, 1)
    assert np.abs(bg).max() < 1 and not (bg.view(np.uint32) & 0xFFFF).any()


def _missed(folded, positions, what):
    """at least one listed position is among the elements the faulty mapping does not fold"""
    assert not folded[positions].all(), f"no listed position notices: {what}"


# ---- the per-tensor scan

SCAN_SHAPES = [   # (n, element size, head elements, CUs)
    (1 + 4 * 2047 + 3, 4, 1, CUS), (1 + 8 * 2047 + 5, 2, 1, CUS),                 # just under one block's 2048 vectors, a head and a tail
    (1 + 4 * 4095 + 3, 4, 1, CUS), (1 + 8 * 4095 + 5, 2, 1, CUS),                 # two blocks
    (3 + 4 * (2 * 4 * 8 * 512 + 5000) + 2, 4, 3, 8), (7 + 8 * (3 * 4 * 8 * 512 + 9001) + 7, 2, 7, 8),   # every round class, on an 8-CU device
]


@pytest.mark.parametrize("n,esize,head,cus", SCAN_SHAPES)
def test_scan_mapping_and_exhaustive_list(n, esize, head, cus):
    g = X.ScanGeometry(n, esize, head, cus)
    assert g.folded().all(), "the restated scan must fold every element"
    every = g.every_position()
    # the coordinates are the simulation's: dropping exactly what coords() names un-folds exactly that element's vector / head / tail element
    rng = np.random.default_rng(n)
    for i in rng.choice(n, 40, replace=False):
        c = g.coords(int(i))
        if c["part"] == "head":
            assert not g.folded(X.ScanFault(head=True))[i]
        elif c["part"] == "tail":
            assert not g.folded(X.ScanFault(tail=True))[i]
        else:
            assert g.element(c["cls"], c["k"], c["block"], c["wave"], c["lane"], c["elem"], rnd=c["round"]) == i
            assert not g.folded(X.ScanFault(slot=(c["cls"], c["k"])))[i], g.describe(i)
            assert not g.folded(X.ScanFault(lane=c["lane"], wave=c["wave"]))[i], g.describe(i)
            assert not g.folded(X.ScanFault(block=c["block"]))[i], g.describe(i)
    for fault in _scan_faults(g, fine=True):
        _missed(g.folded(fault), every, f"{fault} in {n} x {esize} bytes")


def _scan_faults(g, fine):
    faults = [X.ScanFault(lane=lane) for lane in range(64)]
    if fine:
        faults += [X.ScanFault(lane=lane, wave=w) for lane in (0, 31, 63) for w in range(X.BLOCK // 64)]
    classes = [c for c, there in (("first", g.whole >= 1), ("refill", g.whole >= 2), ("ragged", g.start <= g.last)) if there]
    faults += [X.ScanFault(cls=c) for c in classes]
    for c in classes:
        for k in range(X.U):
            if c != "ragged" or g.start + k * g.nthreads <= g.last:
                faults.append(X.ScanFault(slot=(c, k)))
    faults += [X.ScanFault(elem=e) for e in range(g.epv)]
    faults += [X.ScanFault(block=b) for b in sorted({0, g.grid // 2, g.grid - 1})]
    faults += [X.ScanFault(clamp=True)]
    if g.last % 64 != 63:
        faults.append(X.ScanFault(wave_skip=True))
    if g.head:
        faults.append(X.ScanFault(head=True))
    if g.tail:
        faults.append(X.ScanFault(tail=True))
    return faults


@pytest.mark.parametrize("esize", [4, 2])
@pytest.mark.parametrize("cus", [8, 256, 304])
def test_scan_class_list_notices_every_fault(esize, cus):
    """the thinned list of the multi-round sweep, at a size with a whole first round, a refilled round and a ragged round"""
    n = X.scan_size_with_every_round_class(esize, cus, head=16 // esize - 1, tail=X.EPV[esize] - 1)
    g = X.ScanGeometry(n, esize, 16 // esize - 1, cus)
    assert g.whole == 2 and g.start <= g.last and g.last % 64 != 63 and g.head and g.tail
    positions = g.class_positions()
    assert positions.size < 1200 and np.unique(positions).size == positions.size
    # the whole fault set is simulated on the 8-CU geometry (a simulation is one pass over every thread of the grid per fault); on the large grids -- 256
    # CUs is the MI355X the GPU sweep runs on -- the faults whose place depends on the grid: slots, classes, blocks, the clamp, the wave skip, head, tail
    assert g.folded().all()
    for fault in _scan_faults(g, fine=False):
        if cus == 8 or (fault.lane is None and fault.elem is None):
            _missed(g.folded(fault), positions, f"{fault} at {cus} CUs")
    seen = [g.coords(int(i)) for i in positions]
    body = [c for c in seen if c["part"] == "body"]
    assert {(c["cls"], c["k"]) for c in body} >= {(c, k) for c in ("first", "refill") for k in range(X.U)} | {("ragged", k) for k in range(3)}
    assert {c["lane"] for c in body} >= {0, 1, 31, 32, 62, 63} and {c["wave"] for c in body} >= {0, X.BLOCK // 64 - 1}
    assert {c["block"] for c in body} >= {0, 1, g.grid // 2, g.grid - 2, g.grid - 1} and {c["elem"] for c in body} == set(range(g.epv))
    assert sum(c["part"] == "head" for c in seen) == g.head and sum(c["part"] == "tail" for c in seen) == g.tail
    blocks = g.block_positions()
    assert [g.coords(int(i))["block"] for i in blocks] == list(range(g.grid))
    assert len({(g.coords(int(i))["cls"], g.coords(int(i))["k"]) for i in blocks}) >= 6 and np.unique(blocks).size == g.grid


def test_scalar_scan_lists_reach_every_block_and_both_ends_of_the_gather():
    big = X.ScalarScanGeometry(X.scalar_scan_size(8 * CUS, CUS, beyond=4 * CUS * X.BLOCK + 77), CUS)
    assert big.grid == 2048 == X.GATHER_MAX and big.grid - 1 > X.GATHER_ONE_WAVE and big.n > big.nthreads
    small = X.ScalarScanGeometry(X.scalar_scan_size(300, CUS), CUS)
    assert 2 <= small.grid == 300 <= X.GATHER_ONE_WAVE + 1
    for g in (big, small):
        p = g.block_positions()
        assert [g.coords(int(i))["block"] for i in p] == list(range(g.grid)) and p.max() < g.n and np.unique(p).size == g.grid
        for b in (0, 1, 511, 512, 513, g.grid - 2, g.grid - 1):
            if b < g.grid:
                _missed(g.folded(block=b), p, f"block {b} of the scalar scan dropped")
        for lane in range(64):
            _missed(g.folded(lane=lane), p, f"lane {lane} of the scalar scan dropped")
    _missed(big.folded(last_pass=True), big.block_positions(), "the last grid-stride pass dropped")
    assert {big.coords(int(i))["pass"] for i in big.block_positions()} == {0, 1}


# ---- the fused kernel

def _fused_faults(g):
    rounds = max(g.rounds_of(b) for b in range(g.G))
    faults = [X.FusedFault(round=k) for k in range(rounds)]
    faults += [X.FusedFault(wave=w) for w in range(X.FBLOCK // 64)]
    faults += [X.FusedFault(lane=lane, wave=w) for lane in (0, 29, 63) for w in (0, 7, 15)]
    faults += [X.FusedFault(elem=e) for e in range(g.epv)]
    faults += [X.FusedFault(block=b) for b in sorted({0, g.G // 2, g.G - 1})]
    faults += [X.FusedFault(clamp=True)]
    if g.tail:
        faults.append(X.FusedFault(tail=True))
    return faults


@pytest.mark.parametrize("esize", [4, 2])
def test_fused_lists_notice_every_fault(esize):
    # the batch member: a sub-grid of 16 blocks with 29 or 30 rounds each -- every register round, every LDS round, a ragged streamed batch
    n, G = X.fused_batch_big_numel(esize, CUS)
    assert G == 16 == X.fused_blocks_per_group(n, esize, 16, CUS)
    g = X.FusedGeometry(n, esize, G)
    assert sorted({g.rounds_of(b) for b in range(G)}) == [X.F_REG + X.F_LDS + 2, X.F_REG + X.F_LDS + 3] and g.tail == 3
    assert g.folded().all()
    full = g.class_positions()
    kinds = {(c["kind"], c["round"]) for c in (g.coords(int(i)) for i in full) if c["part"] == "body"}
    assert len(kinds) == X.F_REG + X.F_LDS + 3 and {k for k, _ in kinds} == {"register", "LDS", "streamed"}
    thin = g.class_positions(waves=[5], lanes=[29])
    assert full.size < 4500 and thin.size < 100
    for fault in _fused_faults(g):
        _missed(g.folded(fault), full, f"{fault}")
        if fault.wave is None and fault.lane is None and fault.elem is None:
            _missed(g.folded(fault), thin, f"{fault} (thinned list)")
    for i in np.random.default_rng(esize).choice(n - 3, 30, replace=False):
        c = g.coords(int(i))
        assert g.element(c["block"], c["round"], c["wave"], c["lane"], c["elem"]) == i
    # (a share's first rounds are also folded by the block in front of it: its last streamed batch reads past its share's end.  Block 0's are not.)
    for i in np.random.default_rng(esize).choice(g.rounds_of(0) * X.FBLOCK * g.epv, 10, replace=False):
        c = g.coords(int(i))
        assert c["block"] == 0 and not g.folded(X.FusedFault(block=0))[i]
        assert not g.folded(X.FusedFault(round=c["round"]))[i] and not g.folded(X.FusedFault(lane=c["lane"], wave=c["wave"]))[i]


@pytest.mark.parametrize("reg,rounds,tail", [(X.F_REG, X.F_REG + X.F_LDS, 4), (X.F_RED_REG, 19, 0)])
def test_fused_full_chip_and_reduce_lists(reg, rounds, tail):
    """the single call at the full-chip size and the reduce variant at 19 rounds per block (its LDS rounds 10 to 18), on a 16-CU stand-in"""
    cus = 16
    n = rounds * X.FBLOCK * cus * 4 + tail
    G = X.fused_blocks_per_group(n, 4, 1, cus)
    g = X.FusedGeometry(n, 4, G, reg)
    assert G == cus and {g.rounds_of(b) for b in range(G)} <= {rounds, rounds + 1}
    positions = g.class_positions(waves=[9], lanes=[40])
    got = {(c["block"], c["round"]) for c in (g.coords(int(i)) for i in positions) if c["part"] == "body"}
    assert got >= {(b, k) for b in (0, G // 2, G - 1) for k in range(rounds)}
    assert {g.kind(k) for k in range(rounds)} == {"register", "LDS"} and g.kind(reg) == "LDS" and g.kind(reg - 1) == "register"
    for k in range(rounds):
        _missed(g.folded(X.FusedFault(round=k)), positions, f"round {k} dropped")
    for b in (0, G // 2, G - 1):
        _missed(g.folded(X.FusedFault(block=b)), positions, f"block {b} dropped")


# ---- the grouped tile

@pytest.mark.parametrize("G", [32, 64, 128, 256, 512, 1024, 2048, 4096])
def test_grouped_sweep_notices_every_fault(G):
    n, lo, hi = X.grouped_sweep(G)
    assert n % G and lo.size == hi.size == 2 * G + 1 and (lo != hi).all() and (lo // G == hi // G).all() and (lo // G == np.arange(2 * G + 1)).all()
    assert sorted(lo[:-1] % G) == sorted(hi[:-1] % G) == sorted(list(range(G)) * 2)
    assert lo[-1] == 2 * G * G and hi[-1] == n - 1
    for esize in (4, 2):
        for bits in (8, 4, 2):
            t = X.GroupedTile(G, esize, bits)
            assert t.folded(np.arange(min(n, 3 * t.chunk + 5))).all()
            faults = [X.GroupedFault(seglane=s) for s in range(t.LPG)] + [X.GroupedFault(row=r) for r in range(t.NV)]
            faults += [X.GroupedFault(set=s) for s in range(t.SETS)] + [X.GroupedFault(elem=e) for e in range(t.epv)]
            faults += [X.GroupedFault(xor_step=1 << s) for s in range(6) if (1 << s) < t.LPG]
            for role, p in (("minimum", lo), ("maximum", hi)):   # lo and hi are separate chains: each role on its own must notice
                for fault in faults:
                    assert not t.folded(p, fault).all(), f"no listed position notices: {fault} in the {role}s of G={G}, {esize}-byte elements, {bits} bits"
            c = t.coords(int(lo[G + 1]))
            assert c["group"] == G + 1 and c["position in group"] == 1 and c["row"] // t.RPG == c["set"]


def test_grouped_tiles_equal_the_header():
    """GroupedTile restates GroupedQuantTile; its formulas are in the header as written here"""
    text = (CSRC / "grouped_kernels.hpp").read_text()
    for line in ("static constexpr int LPG = V < 64 ? V : 64;", "static constexpr int RPG = V < 64 ? 1 : V / 64;",
                 "static constexpr int NV_WANT = (16 / OB) > 4 ? 16 / OB : 4;",
                 "static constexpr int NV = RPG > (V < NV_WANT ? V : NV_WANT) ? RPG : (V < NV_WANT ? V : NV_WANT);",
                 "static constexpr int SETS = NV / RPG;", "static constexpr int GPR = 64 / LPG;"):
        assert line in text, (f"GroupedTile of tests/extremum_positions.py restates `{line}` of csrc/grouped_kernels.hpp, which is no longer there as written: "
                              "compare GroupedQuantTile with GroupedTile, then update both GroupedTile and this text")


# ---- the sweep on the host: the companion library and the checker

@pytest.fixture(scope="module")
def O(oracle_mod):
    return oracle_mod


def _host_tensor(n, off, dt, O):
    """background of n elements `off` elements behind a 64-byte boundary -> (keep-alive, view); bfloat16 as bit patterns"""
    esize = 4 if dt == O.F32 else 2
    bg = X.background(n, n + off)
    vals = bg if dt == O.F32 else O.f32_to_bf16(bg)
    raw = np.zeros((n + off) * esize + 64, dtype=np.uint8)
    base = (-raw.ctypes.data) % 64
    view = raw[base + off * esize: base + (off + n) * esize].view(vals.dtype)
    view[:] = vals
    assert view.ctypes.data % 64 == off * esize
    return raw, view


def _planted(dt, O):
    lo, hi = (X.LO, X.HI) if dt == O.F32 else O.f32_to_bf16(np.array([X.LO, X.HI], dtype=np.float32))
    return lo, hi


def test_oracle_minmax_finds_the_extremes_everywhere(O):
    """the checker checked: oracle.minmax against numpy on every position"""
    for dt in (O.F32, O.BF16):
        for n in (1037, 4099):
            _, x = _host_tensor(n, 0, dt, O)
            x = x.copy()
            lo, hi = _planted(dt, O)
            for a, b in X.pair_up(np.arange(n)):
                keep = x[[a, b]].copy()
                x[a], x[b] = lo, hi
                xf = x if dt == O.F32 else O.bf16_to_f32(x)
                assert O.minmax(x, dt) == (float(xf.min()), float(xf.max())) == (-3.0, 5.0), (dt, n, a, b)
                x[[a, b]] = keep
    assert O.compute_quant_params(np.array([-3, 5], dtype=np.float32), O.F32, O.UINT8) == O.quant_params_from_minmax(-3.0, 5.0, O.UINT8)


@pytest.mark.parametrize("vector", [True, False], ids=["avx512", "scalar"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_companion_scans_find_the_extremes_everywhere(O, vector, dtype):
    from piquant import cpu

    before = cpu.has_avx512()   # the scan form in effect when the test began: restored at the end
    if vector and not cpu.use_avx512(True):
        cpu.use_avx512(before)
        pytest.skip("host without AVX-512")
    dt = O.F32 if dtype == "f32" else O.BF16
    lo, hi = _planted(dt, O)
    want_params = {t: O.compute_quant_params(np.array([X.LO, X.HI], dtype=np.float32), O.F32, t) for t in (O.UINT8, O.UINT4, O.UINT2)}
    cpu.use_avx512(vector)
    try:
        for threads in (1, 3, 0):   # 0: the default pool; partition heads and tails move with the thread count
            ctx = cpu.CpuContext(threads)
            try:
                for off in range(4):
                    n = 3001 + 16 * off
                    keep_alive, x = _host_tensor(n, off, dt, O)
                    bad = []
                    for k, (a, b) in enumerate(X.pair_up(np.arange(n))):
                        keep = x[[a, b]].copy()
                        x[a], x[b] = lo, hi
                        if ctx.minmax_ptr(x.ctypes.data, dt, n) != (-3.0, 5.0):
                            bad.append((int(a), int(b), ctx.minmax_ptr(x.ctypes.data, dt, n)))
                        if k % 97 == 0:
                            for t, want in want_params.items():
                                assert ctx.compute_quant_params_ptr(x.ctypes.data, dt, n, t) == want, (threads, off, a, b, t)
                        x[[a, b]] = keep
                    assert not bad, (f"{dtype}, {ctx.num_threads} threads, {off} elements off a 64-byte boundary, n={n}: {len(bad)} launches missed an extremum; "
                                     f"first: minimum at element {bad[0][0]}, maximum at element {bad[0][1]}, got {bad[0][2]}")
                    del keep_alive
            finally:
                ctx.close()
    finally:
        cpu.use_avx512(before)
