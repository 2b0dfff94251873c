"""Where to put the one minimum and the one maximum of a tensor so that every term of a min/max reduction is visited.  Pure numpy.

Every quantization parameter of the library comes out of a min/max reduction, and a reduction that drops one position -- a lane, a slot of the
ragged round, one resident round, one row, the head, the tail -- still returns a plausible (scale, zero point): on random data almost always the
right one, because the extremum is somewhere else.  A sweep (tests/test_extremum_positions_cpu.py runs it on the host scans) plants
LO = -3 and HI = +5 over a background inside (-1, 1) at chosen places, so the expected result is the same for every place.

This module mirrors the index arithmetic of the three kernel families -- it says for every element WHICH block, round, slot, wave, lane and
element of a vector folds it -- and simulates each mapping in numpy with one term removed (the fault models), so that the position lists can be
proven to visit every term (tests/test_extremum_positions_cpu.py).  MIRRORED holds the launch constants the arithmetic depends on; the CPU test
compares them with the C++ headers, so a retune forces a look at the sweeps.
"""
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

LO, HI = np.float32(-3.0), np.float32(5.0)

# csrc/tuning.hpp and csrc/grouped_kernels.hpp (kGroupedBlock)
MIRRORED = {
    "kMinmaxBlock": 512,
    "kMinmaxU": 4,
    "kMinmaxBlocksPerCU": 1,
    "kFusedBlock": 1024,
    "kFusedRegRounds": 18,
    "kFusedLdsRounds": 9,
    "kFusedReduceRegRounds": 10,
    "kFusedMinRounds": 2,
    "kGroupedBlock": 256,
}
BLOCK, U, BLOCKS_PER_CU = MIRRORED["kMinmaxBlock"], MIRRORED["kMinmaxU"], MIRRORED["kMinmaxBlocksPerCU"]
FBLOCK, F_REG, F_LDS, F_RED_REG, F_MIN_ROUNDS = (MIRRORED[k] for k in ("kFusedBlock", "kFusedRegRounds", "kFusedLdsRounds", "kFusedReduceRegRounds", "kFusedMinRounds"))
F_STREAM_BATCH = 4        # fused_params_quantize_kernel's STREAM_BATCH default
F_MAX_BLOCKS = 256        # kFusedMaxBlocks
SCALAR_BLOCKS_PER_CU = 8  # minmax_t: capped_grid(.., 8, num_cu) for the scan of a buffer that is not element-aligned
GATHER_ONE_WAVE = 512     # minmax_block_end_gather: grids of up to 64 * LPL + 1 blocks are swept by every wave, larger ones in shares
GATHER_MAX = 2048         # kMinmaxGatherMax
EPV = {4: 4, 2: 8}        # elements per 16-byte vector by element size


def constants_in(*headers):
    """{name: value} of every `constexpr int NAME = VALUE;` in the given C++ headers"""
    found = {}
    for h in headers:
        for name, value in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", Path(h).read_text()):
            found[name] = int(value)
    return found


def background(n, seed, dtype=np.float32):
    """n values inside (-1, 1), every one representable in bfloat16 (the low 16 bits of the float32 pattern are zero)"""
    x = np.random.default_rng(seed).uniform(-0.96875, 0.96875, n).astype(np.float32)
    x = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    assert float(np.abs(x).max()) < 1.0
    return x.astype(dtype)


def pair_up(positions):
    """[(index of LO, index of HI)] -- one launch each: LO walks the list, HI walks it half a list ahead, so both roles visit every position and
    never share one (lo and hi are separate chains of the reduction)"""
    p = np.asarray(positions, dtype=np.int64)
    assert p.size >= 4 and np.unique(p).size == p.size, "positions must be distinct (and at least four, so that consecutive launches do not collide)"
    return np.stack([p, np.roll(p, -(p.size // 2))], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the per-tensor scan: minmax_kernel / minmax_scan_share (csrc/minmax_kernels.hpp), launched by minmax_t (csrc/kernels.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScanFault:
    """One term of the scan removed.  None / False: nothing removed."""
    lane: int = None          # this lane of every wave folds nothing
    wave: int = None          # with `lane`: only in this wave
    slot: tuple = None        # (round class, k): the loads of slot k in rounds of that class are never folded
    cls: str = None           # every load of this round class
    elem: int = None          # this element of every vector
    head: bool = False        # block 0's head elements
    tail: bool = False        # the scalar tail
    block: int = None         # everything this block folds
    clamp: bool = False       # loads whose address was clamped to the last vector -- the lane that owns it included (`i < last ? i : last`)
    wave_skip: bool = False   # a ragged slot is skipped for a wave whose LAST lane is past the end, not only for one whose first lane is


class ScanGeometry:
    """The vector scan of `n` elements of `esize` bytes at a pointer `head` elements in front of a 16-byte boundary, on `num_cu` CUs."""

    def __init__(self, n, esize, head, num_cu):
        self.n, self.esize, self.epv = n, esize, EPV[esize]
        self.head = min(head, n)
        body = n - self.head
        self.n_vec, self.tail = body // self.epv, body % self.epv
        per_block = BLOCK * U * self.epv
        self.grid = max(1, min((body + per_block - 1) // per_block, BLOCKS_PER_CU * num_cu))
        self.nthreads = self.grid * BLOCK
        self.round = U * self.nthreads
        self.whole = self.n_vec // self.round          # whole rounds
        self.start = self.whole * self.round           # first vector of the ragged round
        self.last = self.n_vec - 1

    # -- coordinates ----------------------------------------------------------------------------------------------------------------------
    def coords(self, i):
        """element index -> dict of the kernel's own terms"""
        if i < self.head:
            return {"part": "head", "i": i, "block": 0, "wave": 0, "lane": i}
        v, e = divmod(i - self.head, self.epv)
        if v >= self.n_vec:
            return {"part": "tail", "j": e, "block": 0, "wave": 0, "lane": e}
        if v < self.start:
            r, off = divmod(v, self.round)
            cls = "first" if r == 0 else "refill"
        else:
            r, off, cls = self.whole, v - self.start, "ragged"
        k, tid = divmod(off, self.nthreads)
        return {"part": "body", "cls": cls, "round": r, "k": k, "block": tid // BLOCK, "wave": tid % BLOCK // 64, "lane": tid % 64, "elem": e, "vector": v}

    def element(self, cls, k, block, wave, lane, elem, rnd=None):
        """the element that (round class, slot, block, wave, lane, element) folds, or None when that vector is past the end"""
        r = {"first": 0, "refill": 1 if rnd is None else rnd, "ragged": self.whole}[cls]
        if (cls == "first" and self.whole < 1) or (cls == "refill" and not 1 <= r < self.whole):
            return None
        v = r * self.round + k * self.nthreads + block * BLOCK + wave * 64 + lane
        return self.head + v * self.epv + elem if v <= self.last else None

    def describe(self, i):
        return f"element {i} of {self.n} (grid {self.grid}, {self.whole} whole rounds): {self.coords(i)}"

    # -- simulation ------------------------------------------------------------------------------------------------------------------------
    def folded(self, fault=ScanFault()):
        """bool[n]: the elements that some thread folds -- minmax_scan_share's loops restated thread by thread, with `fault` removed"""
        done = np.zeros(self.n, dtype=bool)
        tid = np.arange(self.nthreads, dtype=np.int64)
        lane, wave, block = tid % 64, tid % BLOCK // 64, tid // BLOCK
        dead = np.zeros(self.nthreads, dtype=bool)
        if fault.lane is not None:
            dead |= (lane == fault.lane) & (True if fault.wave is None else wave == fault.wave)
        if fault.block is not None:
            dead |= block == fault.block

        def fold(vec, cls, k, active=None, clamped=None):
            keep = ~dead if active is None else active & ~dead
            if fault.cls == cls or fault.slot == (cls, k):
                return
            if fault.clamp and clamped is not None:
                keep = keep & ~clamped
            for e in range(self.epv):
                if e != fault.elem:
                    done[self.head + vec[keep] * self.epv + e] = True

        if self.n_vec > 0:
            start, held, raw, cls_of = 0, False, [None] * U, ["first"] * U
            if self.round <= self.n_vec:
                raw = [tid + k * self.nthreads for k in range(U)]
                held, start = True, self.round
                while start + self.round <= self.n_vec:
                    for k in range(U):
                        fold(raw[k], cls_of[k], k)
                        raw[k], cls_of[k] = start + tid + k * self.nthreads, "refill"
                    start += self.round
            assert start == self.start
            wave_first = tid - lane
            live, ragged = [], []
            for k in range(U):
                if held:
                    fold(raw[k], cls_of[k], k)
                edge = wave_first + (63 if fault.wave_skip else 0)
                live.append(edge + start + k * self.nthreads <= self.last)
                ragged.append(start + tid + k * self.nthreads)
            for k in range(U):
                fold(np.minimum(ragged[k], self.last), "ragged", k, active=live[k], clamped=ragged[k] >= self.last)
        if not fault.tail:
            for j in range(self.tail):        # i = n_vec * EPV + tid < numel: thread j of block 0 (the grid has more threads than a vector has elements)
                if not dead[j] and j != fault.elem:
                    done[self.head + self.n_vec * self.epv + j] = True
        if not fault.head:
            for i in range(self.head):        # block 0, thread i
                if not dead[i]:
                    done[i] = True
        return done

    # -- position lists --------------------------------------------------------------------------------------------------------------------
    def every_position(self):
        return np.arange(self.n, dtype=np.int64)

    def class_positions(self):
        """The multi-round classes: round class x slot k x blocks {0, 1, middle, grid - 2, grid - 1} x waves {0, last} x lanes {0, 1, 31, 32, 62, 63}
        with the element cycling; the tensor's last vector and the one before it; the first vector of the wave that the tensor ends in; every
        tail element and every head element."""
        g = self.grid
        blocks = sorted({0, min(1, g - 1), g // 2, max(g - 2, 0), g - 1})
        out, e = [], 0
        for cls in ("first", "refill", "ragged"):
            for k in range(U):
                for b in blocks:
                    for w in (0, BLOCK // 64 - 1):
                        for lane in (0, 1, 31, 32, 62, 63):
                            i = self.element(cls, k, b, w, lane, e % self.epv)
                            if i is not None:
                                out.append(i)
                                e += 1
        for lane in range(64):   # every lane of a wave once (the DPP reduction treats each differently), wave, block, slot and class varying
            for cls in (("first", "refill", "ragged")[lane % 3], "first", "ragged"):
                i = self.element(cls, lane % U, blocks[lane % len(blocks)], lane % (BLOCK // 64), lane, e % self.epv)
                if i is not None:
                    out.append(i)
                    e += 1
                    break
        if self.whole > 2:   # the last refilled round as well as the first
            for k in range(U):
                i = self.element("refill", k, g // 2, 3, 17, e % self.epv, rnd=self.whole - 1)
                out.append(i)
                e += 1
        for v in (self.last, self.last - 1, self.last // 64 * 64):
            for el in (0, self.epv - 1):
                out.append(self.head + v * self.epv + el)
        c = self.coords(self.head + self.last * self.epv)
        if c["cls"] == "ragged":   # the first vector of the wave whose later lanes are past the end
            out.append(self.element("ragged", c["k"], c["block"], c["wave"], 0, 1))
        out += list(range(self.head)) + list(range(self.head + self.n_vec * self.epv, self.n))
        return np.array(sorted(set(out)), dtype=np.int64)

    def block_positions(self):
        """one position in every block, the thread and the slot varying with the block"""
        out = []
        for b in range(self.grid):
            t = (b * 37) % BLOCK
            i = None
            for cls in (("first", "ragged", "refill")[b % 3], "first", "ragged"):
                i = self.element(cls, b % U, b, t // 64, t % 64, b % self.epv)
                if i is not None:
                    break
            if i is None:   # a short tensor: the block's first vector
                i = self.element("ragged", 0, b, 0, 0, 0)
            out.append(i)
        return np.array(out, dtype=np.int64)


def scan_size_with_every_round_class(esize, num_cu, head=1, tail=3):
    """n such that the scan has a whole first round, one refilled whole round and a ragged round that ends inside a wave:
    n_vec ~ 2.6 x U x grid x BLOCK"""
    grid = BLOCKS_PER_CU * num_cu
    n_vec = 2 * U * grid * BLOCK + (U * grid * BLOCK * 3) // 5 + 37
    return head + n_vec * EPV[esize] + tail


class ScalarScanGeometry:
    """minmax_scalar_kernel (a buffer that is not element-aligned): element i is folded by thread i % nthreads in pass i // nthreads"""

    def __init__(self, n, num_cu):
        self.n = n
        self.grid = max(1, min((n + BLOCK - 1) // BLOCK, SCALAR_BLOCKS_PER_CU * num_cu))
        self.nthreads = self.grid * BLOCK

    def coords(self, i):
        p, tid = divmod(i, self.nthreads)
        return {"pass": p, "block": tid // BLOCK, "wave": tid % BLOCK // 64, "lane": tid % 64}

    def describe(self, i):
        end = "slot" if self.grid > GATHER_MAX else ("large-grid gather" if self.grid - 1 > GATHER_ONE_WAVE else "one-wave gather")
        return f"element {i} of {self.n} (grid {self.grid}, {end} end): {self.coords(i)}"

    def folded(self, lane=None, block=None, last_pass=False):
        i = np.arange(self.n, dtype=np.int64)
        tid = i % self.nthreads
        done = np.ones(self.n, dtype=bool)
        if lane is not None:
            done &= tid % 64 != lane
        if block is not None:
            done &= tid // BLOCK != block
        if last_pass:
            done &= i // self.nthreads != (self.n - 1) // self.nthreads
        return done

    def block_positions(self):
        """one position per block, the thread varying with the block; odd blocks in the last (partial) grid-stride pass where it reaches them"""
        out = []
        for b in range(self.grid):
            i = b * BLOCK + (b * 37 + 5) % BLOCK
            if b % 2 and i + self.nthreads < self.n:
                i += self.nthreads
            out.append(min(i, self.n - 1) if b == self.grid - 1 else i)
        return np.array(out, dtype=np.int64)


def scalar_scan_size(grid, num_cu, beyond=0):
    """n for which minmax_scalar_kernel's grid is `grid` blocks (at most 8 per CU), plus `beyond` elements of a further grid-stride pass"""
    assert 1 <= grid <= SCALAR_BLOCKS_PER_CU * num_cu and (beyond == 0 or grid == SCALAR_BLOCKS_PER_CU * num_cu)
    return grid * BLOCK - 3 + (beyond + 3 if beyond else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the one-launch quantize_dynamic: fused_params_quantize_kernel (csrc/fused_kernels.hpp), sized by fused_blocks_per_group (csrc/kernels.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fused_blocks_per_group(max_numel, esize, count, num_cu):
    n_vec = max_numel // EPV[esize]
    cap = min(num_cu // count, F_MAX_BLOCKS)
    per = FBLOCK * F_MIN_ROUNDS
    return min(cap, max((n_vec + per - 1) // per, 1))


@dataclass(frozen=True)
class FusedFault:
    lane: int = None
    wave: int = None          # every lane of this wave (with `lane`: that lane of this wave only)
    round: int = None         # round k of every block's share (register, LDS or streamed)
    elem: int = None
    tail: bool = False
    block: int = None
    clamp: bool = False       # loads whose address was clamped to the last vector, its owner included


class FusedGeometry:
    """One tensor of a fused launch: `n` elements in a sub-grid of G blocks with `reg` register-resident and F_LDS LDS-resident rounds."""

    def __init__(self, n, esize, G, reg=F_REG):
        self.n, self.esize, self.epv, self.G, self.reg = n, esize, EPV[esize], G, reg
        self.n_vec, self.tail = n // self.epv, n % self.epv
        self.all_rounds = (self.n_vec + FBLOCK - 1) // FBLOCK
        self.first_round = [b * self.all_rounds // G for b in range(G + 1)]

    def rounds_of(self, b):
        return self.first_round[b + 1] - self.first_round[b]

    def kind(self, k):
        return "register" if k < self.reg else ("LDS" if k < self.reg + F_LDS else "streamed")

    def coords(self, i):
        v, e = divmod(i, self.epv)
        if v >= self.n_vec:
            return {"part": "tail", "j": e, "block (min/max)": 0, "block (bytes)": self.G - 1, "lane": e}
        rg, tid = divmod(v, FBLOCK)
        b = int(np.searchsorted(self.first_round, rg, side="right")) - 1
        k = rg - self.first_round[b]
        return {"part": "body", "block": b, "round": k, "kind": self.kind(k), "wave": tid // 64, "lane": tid % 64, "elem": e, "vector": v}

    def element(self, block, k, wave, lane, elem):
        if k >= self.rounds_of(block):
            return None
        v = (self.first_round[block] + k) * FBLOCK + wave * 64 + lane
        return v * self.epv + elem if v < self.n_vec else None

    def describe(self, i):
        return f"element {i} of {self.n} (sub-grid {self.G}, {self.all_rounds} rounds, {self.reg} + {F_LDS} resident): {self.coords(i)}"

    def folded(self, fault=FusedFault()):
        """bool[n]: the elements that phase 1 folds into some block's min/max, with `fault` removed"""
        done = np.zeros(self.n, dtype=bool)
        tid = np.arange(FBLOCK, dtype=np.int64)
        dead = np.zeros(FBLOCK, dtype=bool)
        if fault.lane is not None:
            dead |= (tid % 64 == fault.lane) & (True if fault.wave is None else tid // 64 == fault.wave)
        elif fault.wave is not None:
            dead |= tid // 64 == fault.wave
        v_last = max(self.n_vec - 1, 0)
        for b in range(self.G):
            if b == fault.block or self.n_vec == 0:
                continue
            total = self.rounds_of(b)
            resident = min(total, self.reg + F_LDS)
            ks = list(range(resident))
            k0 = self.reg + F_LDS
            while k0 < total:   # streamed batches: whole batches, slots past the share's end hold other real data of the tensor
                ks += list(range(k0, k0 + F_STREAM_BATCH))
                k0 += F_STREAM_BATCH
            for k in ks:
                if k == fault.round:
                    continue
                v = (self.first_round[b] + k) * FBLOCK + tid
                keep = ~dead & ~(v >= v_last) if fault.clamp else ~dead
                v = np.minimum(v, v_last)[keep]
                for e in range(self.epv):
                    if e != fault.elem:
                        done[v * self.epv + e] = True
        if not fault.tail and fault.block != 0:
            for j in range(self.tail):   # block 0, thread j
                if not dead[j]:
                    done[self.n_vec * self.epv + j] = True
        return done

    def class_positions(self, waves=None, lanes=(0, 29, 63), blocks=None):
        """blocks {first, middle, last} x every round x every wave x lanes {0, interior, 63}, the element cycling; the tensor's last vector; every
        tail element"""
        blocks = sorted({0, self.G // 2, self.G - 1}) if blocks is None else blocks
        waves = range(FBLOCK // 64) if waves is None else waves
        out, e = [], 0
        for b in blocks:
            for k in range(self.rounds_of(b)):
                for w in waves:
                    for lane in lanes:
                        i = self.element(b, k, w, lane, e % self.epv)
                        if i is not None:
                            out.append(i)
                            e += 1
        out += [(self.n_vec - 1) * self.epv, self.n_vec * self.epv - 1]
        out += list(range(self.n_vec * self.epv, self.n))
        return np.array(sorted(set(out)), dtype=np.int64)


def fused_batch_big_numel(esize, num_cu, count=16, tail=3):
    """The tensor of a batch of `count` whose sub-grid reaches every resident round plus a ragged streamed batch: the sub-grid's blocks get
    F_REG + F_LDS + 2 or + 3 rounds, the last block's share ends a few hundred vectors short, and `tail` elements follow the last vector"""
    G = min(num_cu // count, F_MAX_BLOCKS)
    rounds = G * (F_REG + F_LDS + 2) + G // 2      # half the blocks get one round more
    return (rounds * FBLOCK - 300) * EPV[esize] + tail, G


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the grouped tile: GroupedQuantTile / grouped_quantize_chunk (csrc/grouped_kernels.hpp)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GroupedFault:
    seglane: int = None       # this lane of every segment folds nothing
    xor_step: int = None      # this step of segment_minmax is a no-op: lanes with that bit set never reach the segment's lane 0
    row: int = None           # this row of the lane's NV rows
    set: int = None           # this group of the lane's SETS groups (all its rows)
    elem: int = None


class GroupedTile:
    """The tile of group size G for tile elements of `esize` bytes (the residual's type for the mixed error-feedback call) and `bits`-wide output."""

    def __init__(self, G, esize, bits):
        self.G, self.epv = G, EPV[esize]
        ob = self.epv * bits // 8
        self.V = G // self.epv
        self.LPG = min(self.V, 64)
        self.RPG = 1 if self.V < 64 else self.V // 64
        want = max(16 // ob, 4)
        self.NV = max(self.RPG, min(self.V, want))
        self.SETS = self.NV // self.RPG
        self.GPR = 64 // self.LPG
        self.NG = self.SETS * self.GPR
        self.chunk = self.NV * 64 * self.epv
        assert 1 <= self.NG <= 64 and self.NG * G == self.chunk

    def coords(self, i):
        c, e = divmod(i % self.chunk, self.epv)
        row, lane = divmod(c, 64)
        return {"chunk": i // self.chunk, "group": i // self.G, "set": row // self.RPG, "row": row, "row in group": row % self.RPG, "lane": lane,
                "lane in segment": lane % self.LPG, "elem": e, "position in group": i % self.G}

    def describe(self, i):
        return f"element {i} (G={self.G}: NV={self.NV} SETS={self.SETS} LPG={self.LPG} RPG={self.RPG}): {self.coords(i)}"

    def folded(self, i, fault=GroupedFault()):
        """bool per element index of `i`: does the element reach its group's result"""
        i = np.asarray(i, dtype=np.int64)
        c, e = np.divmod(i % self.chunk, self.epv)
        row, lane = np.divmod(c, 64)
        seg = lane % self.LPG
        done = np.ones(i.size, dtype=bool)
        if fault.seglane is not None:
            done &= seg != fault.seglane
        if fault.xor_step is not None and fault.xor_step < self.LPG:
            done &= seg & fault.xor_step == 0
        if fault.row is not None:
            done &= row != fault.row
        if fault.set is not None:
            done &= row // self.RPG != fault.set
        if fault.elem is not None:
            done &= e != fault.elem
        return done


def grouped_sweep(G, ragged=None):
    """The layout of one grouped sweep call: 2 G whole groups and a ragged last one.  Group g has its minimum at g mod G and its maximum at
    (g + G / 2) mod G; the ragged group at its first and last element.  -> (n, indices of LO, indices of HI)"""
    ragged = G // 2 + 3 if ragged is None else ragged
    assert 2 <= ragged < G
    g = np.arange(2 * G, dtype=np.int64)
    lo = np.append(g * G + g % G, 2 * G * G)
    hi = np.append(g * G + (g + G // 2) % G, 2 * G * G + ragged - 1)
    return 2 * G * G + ragged, lo, hi
