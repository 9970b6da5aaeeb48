"""Spell statistics without a GPU: the entry point is declared and exported, the Python wrappers lay out planes and offsets (the
library call stubbed), the NumPy model the GPU tests compare with is pinned against a per-cell loop and against the oracle, the
inputs of the GPU tests are shown to tell a carried run from a restarted one, and tests/sim/spell_check.cpp runs the fold, the hit
test and the planner on the CPU under AddressSanitizer and UBSan."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import spell_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_symbol_declared_and_exported():
    from dcdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    m = re.search(r"int dcdf_raster_spells_batch\(([^;]*)\);", hdr)
    assert m, "dcdf_raster_spells_batch is not declared"
    args = re.sub(r"\s+", " ", m.group(1))
    assert args == ("const dcdf_raster* r, const dcdf_cube* cubes, const double* lower, const double* upper, size_t nq, "
                    "uint32_t ops, uint32_t* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms")
    assert re.search(r"enum \{ DCDF_SPELL_COUNT = 1, DCDF_SPELL_LONGEST = 2, DCDF_SPELL_LONGEST_START = 4, DCDF_SPELL_FIRST = 8, "
                     r"DCDF_SPELL_LAST = 16 \};", hdr)
    assert re.search(r"#define DCDF_SPELL_NONE 0xffffffffu", hdr)
    assert "dcdf_raster_spells_batch" in _lib.SYMBOLS
    assert _lib.SPELL_OPS == M.BIT and tuple(_lib.SPELL_OPS) == M.NAMES and _lib.SPELL_NONE == M.NONE == 0xffffffff
    so = _lib.LIB_PATH
    assert os.path.exists(so), "library not built"
    lib = C.CDLL(so)  # (loading needs no GPU)
    assert lib.dcdf_raster_spells_batch
    assert lib.dcdf_abi_version() == 3  # an added entry point: the ABI version stays


class _Stub:
    """Stands in for the loaded library: records what the entry point is called with."""

    def __init__(self):
        self.calls = []

    def dcdf_raster_spells_batch(self, h, cubes, lower, upper, nq, ops, out, mem, off, stats, ms):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        lo = np.ctypeslib.as_array(C.cast(lower, C.POINTER(C.c_double)), shape=(max(nq, 1),))[:nq].copy()
        hi = np.ctypeslib.as_array(C.cast(upper, C.POINTER(C.c_double)), shape=(max(nq, 1),))[:nq].copy()
        self.calls.append((q, o, ops.value, mem, out.value, lo, hi))
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0


def test_wrappers_lay_out_planes(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    R._native = C.c_void_p(1)  # (never dereferenced: the library is stubbed)
    try:
        #        5 x 7            reversed: 7 x 20      no instants      reversed rows: 50 x 60  no rows
        cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 5], [0, 10, 50, 0, 0, 60], [1, 2, 3, 3, 4, 9]]
        lower, upper = [0.5, -np.inf, 3.0, 9.0, 1.0], [2.5, 7.0, 1.0, np.inf, 1.0]
        for ops, mask in ((31, 31), (("longest_start",), 4), ("count", 1), (["last", "count", "longest"], 19), (np.uint32(24), 24)):
            stub.calls.clear()
            n = bin(mask).count("1")
            flat, off, ms, stats = R.spells_flat(cubes, lower, upper, ops)
            q, o, got_mask, mem, _, lo, hi = stub.calls[0]
            assert got_mask == mask and mem == _lib.MEM_HOST
            np.testing.assert_array_equal(q, cubes)  # (the library normalises reversed bounds itself)
            np.testing.assert_array_equal(off, [0, 35 * n, 175 * n, 175 * n, 3175 * n])
            np.testing.assert_array_equal(o, off)
            np.testing.assert_array_equal(lo, lower)  # (and reversed value bounds)
            np.testing.assert_array_equal(hi, upper)
            assert flat.dtype == np.uint32 and flat.size == 3175 * n and stats.tolist() == [5, 6, 7]
        stub.calls.clear()
        R.spells_flat(cubes, 1.5, np.inf, "count")  # scalar bounds: shared by all cubes
        assert stub.calls[0][5].tolist() == [1.5] * 5 and stub.calls[0][6].tolist() == [np.inf] * 5
        assert EncodedRaster.spell_ops(["last", "count", "longest_start"]) == (21, ["count", "longest_start", "last"])  # plane order = bit order
        assert EncodedRaster.spell_ops(31)[1] == list(M.NAMES)
        for bad in (0, 32, [], ["median"], "longest_end"):
            with pytest.raises(ValueError):
                EncodedRaster.spell_ops(bad)
        # device form: the caller's offsets go through untouched
        stub.calls.clear()
        ms, stats = R.spells_flat(cubes, lower, upper, ("longest", "first"), out_device_ptr=4096, out_offset=[9, 200, 700, 701, 40000])
        q, o, got_mask, mem, ptr, _, _ = stub.calls[0]
        assert (got_mask, mem, ptr) == (10, _lib.MEM_DEVICE, 4096) and o.tolist() == [9, 200, 700, 701, 40000]
        # spells(): one cube, a dict of planes in bit order
        stub.calls.clear()
        d = R.spells(0.0, 1.0, ("last", "count"), 2, 7)
        assert list(d) == ["count", "last"] and all(v.shape == (50, 60) and v.dtype == np.uint32 for v in d.values())
        assert stub.calls[0][0].tolist() == [[2, 7, 0, 50, 0, 60]] and stub.calls[0][2] == 17
        d = R.spells(-np.inf, 4.0, window=(3, 10, 20, 60))
        assert list(d) == ["count", "longest"] and d["count"].shape == (7, 40) and stub.calls[1][0].tolist() == [[0, 10, 3, 10, 20, 60]]
        d = R.spells(0.0, 1.0, 31, 3, 3)  # no instants: nothing to read, no call
        assert len(stub.calls) == 2 and list(d) == list(M.NAMES) and all(v.dtype == np.uint32 and v.shape == (50, 60) for v in d.values())
        assert (d["count"] == 0).all() and (d["longest"] == 0).all()
        assert all((d[n] == _lib.SPELL_NONE).all() for n in ("longest_start", "first", "last"))
        for bad in (dict(start=5, stop=4), dict(stop=11), dict(start=-1, stop=3), dict(window=(0, 51, 0, 60)), dict(window=(4, 3, 0, 60)), dict(ops=0),
                    dict(ops=("count", "mean"))):
            with pytest.raises(ValueError):
                R.spells(0.0, 1.0, **bad)
        for lo, hi in ((np.nan, 1.0), (0.0, np.nan)):  # a NaN bound
            with pytest.raises(ValueError):
                R.spells(lo, hi)
            with pytest.raises(ValueError):
                R.spells(lo, hi, start=3, stop=3)
            with pytest.raises(ValueError):
                R.spells_flat(cubes, [0, 0, lo, 0, 0], [1, 1, hi, 1, 1], 1)
        assert len(stub.calls) == 2
    finally:
        R._native = None


def brute(series):
    """The five numbers of one cell's hit series, run by run."""
    count = longest = 0
    lstart = first = last = M.NONE
    i = 0
    for hit, grp in itertools.groupby(series):
        n = len(list(grp))
        if hit:
            count += n
            if n > longest:
                longest, lstart = n, i
            if first == M.NONE:
                first = i
            last = i + n - 1
        i += n
    return count, longest, lstart, first, last


def test_model_against_a_per_cell_loop():
    rng = np.random.default_rng(4)
    for T, p in ((1, 0.5), (2, 0.5), (13, 0.5), (40, 0.2), (40, 0.8), (31, 0.5)):
        h = rng.random((T, 9, 11)) < p
        h[:, 0, 0] = True    # all hit
        h[:, 0, 1] = False   # no hit
        if T >= 13:
            h[:, 0, 2] = [(i % 4) != 3 for i in range(T)]      # tied longest runs of 3: the first one wins
            h[:, 0, 3] = [i in (2, 3, 8, 9, 11) for i in range(T)]
        got = M.spells(h)
        assert all(got[n].dtype == np.uint32 and got[n].shape == (9, 11) for n in M.NAMES) and list(got) == list(M.NAMES)
        for r in range(9):
            for c in range(11):
                assert tuple(int(got[n][r, c]) for n in M.NAMES) == brute(h[:, r, c].tolist()), (T, r, c)
        assert tuple(int(got[n][0, 0]) for n in M.NAMES) == (T, T, 0, 0, T - 1)
        assert tuple(int(got[n][0, 1]) for n in M.NAMES) == (0, 0, M.NONE, M.NONE, M.NONE)
        if T >= 13:
            assert int(got["longest"][0, 2]) == 3 and int(got["longest_start"][0, 2]) == 0
            assert tuple(int(got[n][0, 3]) for n in M.NAMES) == (5, 2, 2, 2, 11)
    empty = M.spells(np.zeros((0, 2, 3), dtype=bool))
    assert (empty["count"] == 0).all() and (empty["first"] == M.NONE).all()


def test_hit_rule_of_the_model():
    i = np.array([-3, -1, 0, 1, 2, 7], dtype=np.int32)
    assert M.hits(i, -0.5, 1.5).tolist() == [False, False, True, True, False, False]
    assert M.hits(i, 1.5, -0.5).tolist() == M.hits(i, -0.5, 1.5).tolist()  # reversed bounds
    assert not M.hits(i, 0.5, 0.5).any() and M.hits(i, -np.inf, np.inf).all() and not M.hits(i, 2.0 ** 40, np.inf).any()
    assert M.hits(i, -np.inf, -1.0).tolist() == [True, True, False, False, False, False]
    big = np.array([2 ** 53 + 1, 2 ** 53], dtype=np.int64)  # integers never round to double
    assert M.hits(big, 2.0 ** 53 + 2, np.inf).tolist() == [False, False] and M.hits(big, 2.0 ** 53, 2.0 ** 53).tolist() == [False, True]
    f = np.array([0.1, np.nan, 0.25, -0.0], dtype=np.float32)
    assert M.hits(f, 0.1, 1.0).tolist() == [True, False, True, False]  # float32(0.1) > 0.1: widened first, it is a hit
    assert M.hits(f, float(np.float32(0.1)), 1.0).tolist() == [True, False, True, False]
    assert M.hits(f, -np.inf, np.inf).tolist() == [True, False, True, True]


def test_model_against_the_oracle():
    """The model applied to the oracle's Chunk::fill_window of a forced-block chunk equals the loop on the source array."""
    import oracle_lib as O
    from bulk_model import leaf_kinds_array
    a = np.ascontiguousarray(leaf_kinds_array(np.random.default_rng(33))[:, :200, :131])
    oc = O.Chunk(O.chunk_build_forced(a, 2, 8))
    w = oc.fill_window(0, 40, 0, 200, 0, 131, dtype=np.int64)
    np.testing.assert_array_equal(w, a)
    med = float(np.median(a))
    got = M.spells(M.hits(w, med, np.inf))
    h = a >= math.ceil(med)
    assert 0 < h.mean() < 1
    np.testing.assert_array_equal(got["count"], h.sum(0).astype(np.uint32))
    rng = np.random.default_rng(1)
    for r, c in zip(rng.integers(0, 200, 300), rng.integers(0, 131, 300)):
        assert tuple(int(got[n][r, c]) for n in M.NAMES) == brute(h[:, r, c].tolist())
    part = M.spells(M.hits(oc.fill_window(5, 17, 3, 90, 7, 100, dtype=np.int32), med, np.inf))
    np.testing.assert_array_equal(part["count"], h[5:17, 3:90, 7:100].sum(0).astype(np.uint32))
    np.testing.assert_array_equal(part["first"], np.where(h[5:17, 3:90, 7:100].any(0), h[5:17, 3:90, 7:100].argmax(0), M.NONE).astype(np.uint32))


def test_the_inputs_prove_something():
    """The raster of the GPU tests, cut where its three segments (8, 8, 4 instants) are cut: a longest run that is carried across a
    segment boundary differs from the longest run inside any one segment -- in the bulk chunks, in the 8 x 8 corner chunk and in
    both edge strips --, some cell has two longest runs of equal length, some cell never hits and some always does."""
    import test_gpu_bulk_decode as BD
    a = BD.source("i32", (20, 264, 264))
    lower = float(np.median(a)) + 0.5
    h = M.hits(a, lower, np.inf)
    assert 0.3 < h.mean() < 0.7
    whole = M.spells(h)
    no_carry = np.maximum(np.maximum(M.spells(h[0:8])["longest"], M.spells(h[8:16])["longest"]), M.spells(h[16:20])["longest"])
    differ = whole["longest"] != no_carry
    print("median", np.median(a), "hit fraction", h.mean(), "differ: bulk", differ[:256, :256].sum(), "corner", differ[256:, 256:].sum(), "strips",
          differ[256:, :256].sum(), differ[:256, 256:].sum())
    assert differ[:256, :256].any() and differ[256:, 256:].any() and differ[256:, :256].any() and differ[:256, 256:].any()
    tied = 0
    for r in range(64):
        for c in range(64):
            runs = [len(list(g)) for hit, g in itertools.groupby(h[:, r, c].tolist()) if hit]
            tied += bool(runs) and runs.count(max(runs)) > 1
    never, always = (whole["count"] == 0).sum(), (whole["count"] == 20).sum()
    print("tied", tied, "never", never, "always", always)
    assert tied > 0 and never > 0 and always > 0


def test_fold_hit_test_and_planner_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/sim/spell_check.cpp over k2r_spell.h and plan_spells, host code only, with AddressSanitizer and UBSan."""
    exe = str(tmp_path / "spell_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", exe, os.path.join(HERE, "sim", "spell_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    got = dict(line.split()[1:3] for line in out.stdout.splitlines() if line.startswith("ok "))
    assert set(got) == {"cuts", "hits", "plan"} and all(int(v) > 1000 for v in got.values()), out.stdout
