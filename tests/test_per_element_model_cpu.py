"""CPU: the inputs of tests/per_element_cases.py have teeth.  For every input of the quantize step that tests/test_gpu_grouped_per_element.py
puts through a kernel, with every index base and seed it uses, each fault model of tests/per_element_model.py that applies to the case (its
index differs from the right one for at least one element) gives packed bytes that differ from the right model's.  A kernel or host path that
computes the element index in one of those wrong ways therefore fails the device test; this is a property of the model and the inputs alone.
The windows of tests/test_gpu_grouped_large.py are checked the same way on a small stand-in for the faults that only a large tensor shows."""
import numpy as np
import pytest

import oracle as O
import per_element_cases as C
import per_element_model as M
from extremum_positions import EPV


def right_model(y, dt, qd, G, seed, base, params, dt_tile, start=0):
    return M.quantize(y, dt, qd, G, seed, base, params, dt_tile=dt_tile, start=start)[0]


def check_stage(what, y, dt, dt_tile, qd, G, params, chunk_begin, named_bases, right=right_model):
    """-> {(base name, fault)} that applied; asserts that each changed the bytes"""
    t = M.tile(dt_tile, qd, G)
    applied = set()
    for name, base, seed in named_bases:
        want = right(y, dt, qd, G, seed, base, params, dt_tile)
        for f in M.FAULTS:
            if not M.applies(y.size, base, t, f, chunk_begin=chunk_begin):
                continue
            got = M.quantize(y, dt, qd, G, seed, base, params, f, dt_tile, chunk_begin=chunk_begin)[0]
            assert got.size == want.size
            assert not np.array_equal(got, want), f"{what}, base {name!r}: fault model ({f}) gives the right model's bytes -- the inputs cannot tell them apart"
            applied.add((name, f))
    return applied


@pytest.mark.parametrize("dt_tile,qd", C.PAIRS)
@pytest.mark.parametrize("G", C.GROUP_SIZES)
def test_bases_are_where_they_say(oracle_mod, dt_tile, qd, G):
    t = M.tile(dt_tile, qd, G)
    assert t.epv == EPV[M.ESIZE[dt_tile]] and t.chunk == t.NV * 64 * t.epv == t.NG * G
    found = C.check_bases(t)
    assert found["row 0"]["row"] == 0 and found["last row"]["row"] == t.NV - 1 and t.NV >= 2


def test_fault_path_with_the_right_index_is_the_definition(oracle_mod):
    """the run-by-run path the fault models take, fed the right index (fault i from a base one lower), gives the group-by-group definition's bytes"""
    for dt, qd, G in ((O.F32, O.UINT8, 32), (O.BF16, O.UINT4, 128), (O.BF16, O.UINT2, 4096)):
        x = C.single(dt, qd, G)[0]
        for _, base, seed in C.bases(M.tile(dt, qd, G)):
            assert np.array_equal(M.quantize(x, dt, qd, G, seed, base)[0], M.quantize(x, dt, qd, G, seed, base - 1, fault="i")[0])


def expect_applied(applied, names, stage_faults):
    for name in names:
        crossing = name != "above"
        for f in stage_faults:
            hits = (name, f) in applied
            if f in "abcijk":
                assert hits, (name, f)
            elif f == "e":
                assert not hits, (name, f)          # no element index of a small tensor reaches 2^32
            elif f == "f":
                assert hits, (name, f)              # every base puts the sum past 2^32
            elif f == "h" and name == "ragged chunk":
                pass                                # applies only where the ragged chunk has a second row
            elif f in "gh":
                assert hits == (crossing and name != "chunk boundary"), (name, f)   # a crossing on a chunk boundary switches no key inside a lane


@pytest.mark.parametrize("dt,qd", C.PAIRS)
def test_single_calls_separate_every_fault(oracle_mod, dt, qd):
    seen = 0
    for what, y, dty, dt_tile, q, G, params, cb in C.quantize_stages(pairs=[(dt, qd)], mixed_qds=[]):
        if "batch" in what:
            continue
        t = M.tile(dt_tile, q, G)
        assert y.size == C.size_of(t)
        applied = check_stage(what, y, dty, dt_tile, q, G, params, cb, C.bases(t))
        expect_applied(applied, [n for n, _, _ in C.bases(t)], "abcefghijk")
        assert not any(f == "d" for _, f in applied)
        seen += 1
    assert seen == 8 * 3 + 3 * (len(C.REDUCE_TERMS) + len(C.REDUCE_EF_TERMS))


@pytest.mark.parametrize("qd", C.QDS)
def test_float32_residual_calls_separate_every_fault(oracle_mod, qd):
    seen = 0
    for what, y, dty, dt_tile, q, G, params, cb in C.quantize_stages(pairs=[], mixed_qds=[qd]):
        if "batch" in what:
            continue
        t = M.tile(dt_tile, q, G)
        assert y.size == C.size_of(t) and t.epv == 4
        applied = check_stage(what, y, dty, dt_tile, q, G, params, cb, C.bases(t))
        expect_applied(applied, [n for n, _, _ in C.bases(t)], "abcefghijk")
        seen += 1
    assert seen == 8 + 3 * len(C.REDUCE_EF_TERMS)


@pytest.mark.parametrize("dt,qd", C.PAIRS + [("mixed", q) for q in C.QDS])
def test_batches_separate_every_fault(oracle_mod, dt, qd):
    """Every member is indexed from index_base + 0, and a fault of a batch kernel is a fault in every member it applies to: the bytes of the batch
    (its members' laid end to end) must differ.  Fault d -- the index continued from the members before it -- applies to every member behind the
    first of its launch."""
    stages = C.quantize_stages(pairs=[], mixed_qds=[qd]) if dt == "mixed" else C.quantize_stages(pairs=[(dt, qd)], mixed_qds=[])
    batches = {}
    for what, y, dty, dt_tile, q, G, params, cb in stages:
        if "batch" in what:
            batches.setdefault(what.rsplit(" member", 1)[0], []).append((y, dty, dt_tile, q, G, cb))
    assert len(batches) == 3 * (1 if dt == "mixed" else 2)
    for what, members in batches.items():
        _, dty, dt_tile, q, G, _ = members[0]
        t = M.tile(dt_tile, q, G)
        assert len(members) == C.BATCH and [m[5] for m in members] == C.batch_chunk_begins(t) and sum(1 for m in members if m[5] > 0) >= 14
        for name, base, seed in C.bases(t):
            want = np.concatenate([M.quantize(y, dty, q, G, seed, base, dt_tile=dt_tile)[0] for y, *_ in members])
            for f in M.FAULTS:
                hit = [M.applies(y.size, base, t, f, chunk_begin=cb) for y, _, _, _, _, cb in members]
                assert any(hit) == (f != "e" and not (f in "gh" and name in ("above", "chunk boundary"))), (what, name, f)
                if any(hit):
                    got = np.concatenate([M.quantize(y, dty, q, G, seed, base, None, f, dt_tile, chunk_begin=cb)[0] for y, _, _, _, _, cb in members])
                    assert not np.array_equal(got, want), f"{what}, base {name!r}: fault model ({f}) gives the right model's bytes"


def test_graph_capture_replay_separates_every_fault(oracle_mod):
    """the fresh input that the captured calls replay on, with the base and seed they were captured with"""
    dt, qd, G = C.CAPTURE
    t = M.tile(dt, qd, G)
    stages = list(C.capture_stages())
    assert len(stages) == 2
    for what, y, dty, dt_tile, q, G, params, cb in stages:
        assert y.size == C.size_of(t)
        expect_applied(check_stage(what, y, dty, dt_tile, q, G, params, cb, C.bases(t)[:1]), ["row 0"], "abcefghijk")


def test_batch_layout(oracle_mod):
    for dt, qd in C.PAIRS:
        for G in C.SOME_G:
            t = M.tile(dt, qd, G)
            ns = C.batch_numels(t)
            assert ns[4] == 0 and ns[9] == 1 and ns[2] == 5 * t.chunk + 3 and len(ns) == 19
            assert sum(1 for i, n in enumerate(ns) if n and i != C.MISALIGNED_MEMBER) > 16, "more than one launch"
            begins = C.batch_chunk_begins(t)
            assert begins[0] == 0 and begins[-1] == 0 and begins[1] == -(-ns[0] // t.chunk)   # the 17th streamed member opens the second launch


# ---- the windows of the large tensors: a fault that needs an element index past 2^32 (e) and the others, on a window that starts there

@pytest.mark.parametrize("dt,qd,G", [(O.BF16, O.UINT4, 128), (O.F32, O.UINT8, 128), (O.BF16, O.UINT4, 32), (O.BF16, O.UINT4, 4096), (O.BF16, O.UINT2, 128)])
def test_windows_past_2_pow_32_separate_every_fault(oracle_mod, dt, qd, G):
    """index_base 0 and a seed with a non-zero upper half, as tests/test_gpu_grouped_large.py runs: a window of eight chunks around element 2^32"""
    t = M.tile(dt, qd, G)
    start, n = 2 ** 32 - 4 * t.chunk, 8 * t.chunk
    y = C.make_input(n, dt, [G, qd, dt, 5], nans=True)[0]
    want = M.quantize(y, dt, qd, G, C.SEED_FULL, 0, start=start)[0]
    for f in M.FAULTS:
        hits = M.applies(n, 0, t, f, start=start)
        assert hits == (f not in "adgh"), f   # base 0: ignoring it changes nothing, and 2^32 is a chunk boundary, where no lane switches its key
        if hits:
            assert not np.array_equal(M.quantize(y, dt, qd, G, C.SEED_FULL, 0, fault=f, start=start)[0], want), f
