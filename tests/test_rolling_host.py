"""The rolling windows over time without a GPU: tests/sim/rolling_check.cpp runs plan_rolling_time and the cell body of
k_rolling_stream (rolling_cell, k2r_rolling.h) on the CPU under AddressSanitizer and UBSan, exactly as the kernel indexes them;
tests/sim/rolling_cell_check.cpp runs the cell body over every short series against a naive sum; rolling_model.py is checked
against hand-made cases; the two entry points are declared, exported and listed; and the Python layer --
EncodedRaster.rolling_time*, Variable's methods of the same names -- is run against a stubbed library: the argument order of
both entries, plane counts and offsets, every ValueError, and the fills where nothing is read."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rolling_model as WM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = "max, argmax, min, argmin, count"
FLAGS = ["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
         "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter"]


def _run(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(FLAGS + ["-o", exe, os.path.join(HERE, "sim", name + ".cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return out.stdout.split()


def test_plan_and_cell_body_in_a_sanitized_stand_alone_program(tmp_path):
    """Every slab read inside the band's used elements, every output element written exactly once and nothing else, the bits of a
    loop with its own integers that only ever sums a window again: 160 cases over four geometries, three slab caps, five label
    sets and seven (window, min_count, kind) triples."""
    words = _run(tmp_path, "rolling_check")
    assert words[:2] == ["ok", "rolling"] and int(words[2]) == 160 and int(words[3]) > 1_000_000 and int(words[4]) > int(words[3]), words


def test_cell_body_over_every_short_series(tmp_path):
    """Every series of up to 8 instants over {3, -2.5, 2^53, NaN} in three segments of different encodings, every window 1 .. 9,
    every min_count, SUM and MEAN, sliding (one group) and rebuilding (i % 2); every label series over {0, 1, none} with 32 series
    each.  The product of every series with every label series (2e10 cell bodies) is not enumerated."""
    words = _run(tmp_path, "rolling_cell_check")
    n_a = sum(4 ** n * 2 for n in range(9)) * 54  # 45 (window, min_count) pairs, 9 of them also as MEAN
    n_b = sum(3 ** n * min(4 ** n, 32) for n in range(9)) * 54
    assert words == ["ok", "cells", str(n_a), str(n_b)], words


def test_model_on_cases_made_by_hand():
    nan = np.nan
    x = np.array([1.0, 4.0, nan, 2.0, 4.0, 1.0, 3.0]).reshape(7, 1, 1)
    d = WM.rolling_time(x, 2, min_count=1)  # sums 5 4 2 6 5 4 ending at 1 .. 6
    assert [d[n][0, 0] for n in WM.NAMES] == [6.0, 4.0, 2.0, 3.0, 6.0]
    d = WM.rolling_time(x, 2)  # whole windows only: 5 . . 6 5 4
    assert [d[n][0, 0] for n in WM.NAMES] == [6.0, 4.0, 4.0, 6.0, 4.0]
    d = WM.rolling_time(x, 2, mean=True)
    assert [d[n][0, 0] for n in WM.NAMES] == [3.0, 4.0, 2.0, 6.0, 4.0]
    d = WM.rolling_time(x, 8, min_count=1)  # wider than the series
    assert all(np.isnan(d[n][0, 0]) for n in WM.NAMES[:4]) and d["count"][0, 0] == 0 and not np.signbit(d["count"][0, 0])
    lab = np.array([0, 1, 1, 0, WM.NONE, 1, 0])
    d = WM.rolling_time_groups(x, 2, lab, 3, min_count=1)  # a window is its last instant's: group 0 has 2 and 4, group 1 has 5 4 5
    assert [d[n][0, 0, 0] for n in WM.NAMES] == [4.0, 6.0, 2.0, 3.0, 2.0]
    assert [d[n][1, 0, 0] for n in WM.NAMES] == [5.0, 1.0, 4.0, 2.0, 3.0]  # equal sums: the earliest
    assert np.isnan(d["max"][2, 0, 0]) and d["count"][2, 0, 0] == 0
    # rounding is not the order: 2^54 and 2^54 + 2 round to one double
    big = np.array([2.0 ** 53, 2.0 ** 53, 2.0 ** 53 + 2, 0.0]).reshape(4, 1, 1)
    d = WM.rolling_time(big, 2)
    assert d["argmax"][0, 0] == 2 and d["max"][0, 0] == 2.0 ** 54 and d["argmin"][0, 0] == 3
    # a constant cell: the earliest window both ways; a sum of zero is +0.0
    d = WM.rolling_time(np.full((9, 1, 1), -0.0), 4)
    assert d["argmax"][0, 0] == 3 and d["argmin"][0, 0] == 3 and d["max"][0, 0] == 0 and not np.signbit(d["max"][0, 0])
    # one rounding: 2^53 + 1 + 1 is 2^53 + 2 exactly, not (2^53 + 1 -> 2^53) + 1 -> 2^53
    d = WM.rolling_time(np.array([2.0 ** 53, 1.0, 1.0]).reshape(3, 1, 1), 3)
    assert d["max"][0, 0] == 2.0 ** 53 + 2


def test_symbols_declared_exported_and_listed():
    from dcdf_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read())
    assert ("int dcdf_raster_rolling_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t window, "
            "uint32_t min_count, int32_t kind, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);") in hdr
    assert ("int dcdf_raster_rolling_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t window, "
            "uint32_t min_count, int32_t kind, const uint16_t* labels, const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem, "
            "const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);") in hdr
    assert ("enum { DCDF_ROLLING_MAX = 1, DCDF_ROLLING_ARGMAX = 2, DCDF_ROLLING_MIN = 4, DCDF_ROLLING_ARGMIN = 8, DCDF_ROLLING_COUNT = 16 };") in hdr
    assert "enum { DCDF_ROLLING_SUM = 0, DCDF_ROLLING_MEAN = 1 };" in hdr
    assert "dcdf_raster_rolling_time_batch" in _lib.SYMBOLS and "dcdf_raster_rolling_time_groups_batch" in _lib.SYMBOLS
    assert os.path.exists(_lib.LIB_PATH), "library not built"
    lib = _lib.lib()  # (loading needs no GPU)
    assert lib.dcdf_raster_rolling_time_batch and lib.dcdf_raster_rolling_time_groups_batch
    assert len(lib.dcdf_raster_rolling_time_batch.argtypes) == 12 and len(lib.dcdf_raster_rolling_time_groups_batch.argtypes) == 15
    assert lib.dcdf_abi_version() == 3  # added entry points: the ABI version stays
    assert _lib.ROLLING_OPS == WM.BITS and list(_lib.ROLLING_OPS) == list(WM.NAMES)
    assert (_lib.ROLLING_SUM, _lib.ROLLING_MEAN, _lib.ROLLING_MAX_WINDOW) == (0, 1, 65535)
    mk = open(os.path.join(ROOT, "dcdf_amd", "csrc", "Makefile")).read()
    assert "$(OUT)/k2r_rolling.o" in mk


# ---- the Python layer against a stubbed library -------------------------------------------------------------------------------------
def _u64(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(max(n, 1),))[:n].copy()


class _Stub:
    """Stands in for the loaded library: records what the two entry points are called with, in the C order of their arguments."""

    def __init__(self):
        self.calls = []

    def _record(self, name, cubes, nq, ops, window, min_count, kind, lab, loff, n_groups, out, mem, off, stats):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        nt = np.abs(q[:, 1].astype(np.int64) - q[:, 0])
        labels = None
        if lab is not None:
            lo = _u64(loff, nq)
            flat = np.ctypeslib.as_array(C.cast(lab, C.POINTER(C.c_uint16)), shape=(int(lo[-1] + nt[-1]) + 1,))
            labels = [flat[int(lo[i]):int(lo[i]) + int(nt[i])].copy() for i in range(nq)]
        assert isinstance(kind, C.c_int32) and isinstance(window, C.c_uint32) and isinstance(min_count, C.c_uint32)
        self.calls.append(dict(name=name, q=q, ops=ops.value, w=window.value, mc=min_count.value, kind=kind.value, labels=labels, n_groups=n_groups,
                               mem=mem, out=out.value, off=_u64(off, nq)))
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0

    def dcdf_raster_rolling_time_batch(self, h, cubes, nq, ops, window, min_count, kind, out, mem, off, stats, ms):
        return self._record("plain", cubes, nq, ops, window, min_count, kind, None, None, None, out, mem, off, stats)

    def dcdf_raster_rolling_time_groups_batch(self, h, cubes, nq, ops, window, min_count, kind, lab, loff, n_groups, out, mem, off, stats, ms):
        return self._record("groups", cubes, nq, ops, window, min_count, kind, lab, loff, n_groups.value, out, mem, off, stats)


@pytest.fixture()
def stubbed(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    R._native = C.c_void_p(1)  # (never dereferenced: the library is stubbed)
    yield R, stub
    R._native = None


def raises(msg, f, *a, **k):
    with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
        f(*a, **k)


#        5 x 7            reversed: 7 x 20      no instants      reversed rows: 50 x 60  no rows
CUBES = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 5], [0, 10, 50, 0, 0, 60], [1, 2, 3, 3, 4, 9]]
NT = [3, 3, 0, 10, 1]


def test_flat_forms(stubbed):
    R, stub = stubbed
    labels = [(np.arange(n) % 2).astype(np.uint16) for n in NT]
    for ops, n in ((31, 5), ("max", 1), (("count", "argmin", "max"), 3), (6, 2)):
        stub.calls.clear()
        flat, off, ms, stats = R.rolling_time_flat(CUBES, ops, 5, 2)
        c = stub.calls[0]
        assert c["name"] == "plain" and c["ops"] == R.rolling_ops(ops)[0] and c["mem"] == 0 and c["labels"] is None
        assert (c["w"], c["mc"], c["kind"]) == (5, 2, 0)
        np.testing.assert_array_equal(c["q"], CUBES)  # (the library normalises reversed bounds itself)
        np.testing.assert_array_equal(off, [0, 35 * n, 175 * n, 175 * n, 3175 * n])
        np.testing.assert_array_equal(c["off"], off)
        assert flat.dtype == np.float64 and flat.size == 3175 * n and stats.tolist() == [5, 6, 7]
        flat, off, ms, stats = R.rolling_time_groups_flat(CUBES, ops, labels, 3, 4, mean=True)
        c = stub.calls[1]
        assert c["name"] == "groups" and c["ops"] == R.rolling_ops(ops)[0] and c["n_groups"] == 3 and (c["w"], c["mc"], c["kind"]) == (4, 4, 1)
        np.testing.assert_array_equal(off, [0, 105 * n, 525 * n, 525 * n, 9525 * n])
        assert flat.size == 9525 * n
        for got, want in zip(c["labels"], labels):
            np.testing.assert_array_equal(got, want)
    assert R.rolling_ops(("min", "max")) == (5, ["max", "min"]) and R.rolling_ops(31)[1] == list(WM.NAMES)
    stub.calls.clear()
    R.rolling_time_flat(CUBES, "max", np.int64(65535))  # min_count None is the window; numpy integers are integers
    R.rolling_time_flat(CUBES, "max", 7, min_count=7, mean=True)
    assert [(c["w"], c["mc"], c["kind"]) for c in stub.calls] == [(65535, 65535, 0), (7, 7, 1)]
    # device form: the caller's offsets go through untouched
    stub.calls.clear()
    ms, stats = R.rolling_time_groups_flat(CUBES, "argmax", labels, 2, 3, 1, out_device_ptr=4096, out_offset=[9, 200, 700, 701, 40000])
    c = stub.calls[0]
    assert (c["mem"], c["out"]) == (1, 4096) and c["off"].tolist() == [9, 200, 700, 701, 40000] and stats.tolist() == [5, 6, 7]


def test_whole_raster_forms(stubbed):
    R, stub = stubbed
    d = R.rolling_time(31, 5)
    c = stub.calls[0]
    assert c["name"] == "plain" and c["q"].tolist() == [[0, 10, 0, 50, 0, 60]] and (c["ops"], c["w"], c["mc"], c["kind"]) == (31, 5, 5, 0)
    assert list(d) == list(WM.NAMES) and all(v.shape == (50, 60) and v.dtype == np.float64 for v in d.values())
    d = R.rolling_time(("argmax", "max"), window=3, min_count=2, start=2, stop=7, region=(3, 10, 20, 60))
    c = stub.calls[1]
    assert c["q"].tolist() == [[2, 7, 3, 10, 20, 60]] and (c["ops"], c["w"], c["mc"]) == (3, 3, 2) and list(d) == ["max", "argmax"]
    assert d["max"].shape == (7, 40)
    d = R.rolling_time("min", 7, mean=True)
    assert (stub.calls[2]["mc"], stub.calls[2]["kind"]) == (7, 1)
    R.rolling_time("max", 11)  # wider than the instants: the library's to answer
    assert stub.calls[3]["w"] == 11
    lab = np.array([0, 2, 2, 0xffff, 0, 2, 0, 0, 2, 5], dtype=np.uint16)
    d = R.rolling_time_groups(("min", "max"), lab, 5, 1)
    c = stub.calls[4]
    assert c["name"] == "groups" and c["n_groups"] == 6 and c["ops"] == 5 and c["labels"][0].tolist() == lab.tolist() and (c["w"], c["mc"]) == (5, 1)
    assert list(d) == ["max", "min"] and all(v.shape == (6, 50, 60) for v in d.values())
    d = R.rolling_time_groups("count", lab[1:4], 2, start=1, stop=4, n_groups=2)
    c = stub.calls[5]
    assert c["n_groups"] == 2 and c["q"].tolist() == [[1, 4, 0, 50, 0, 60]] and d["count"].shape == (2, 50, 60)
    assert len(stub.calls) == 6


def test_every_refusal(stubbed):
    R, stub = stubbed
    f, g = R.rolling_time, R.rolling_time_groups
    lab = np.zeros(10, dtype=np.uint16)
    raises("rolling_time: unknown statistic 'mean' (one of %s)" % NAMES, f, "mean", 3)
    raises("rolling_time: unknown statistic 'sum' (one of %s)" % NAMES, f, ("max", "sum"), 3)
    raises("rolling_time: ops 32 is not a set of %s" % NAMES, f, 32, 3)
    raises("rolling_time: ops 0 is not a set of %s" % NAMES, f, 0, 3)
    raises("rolling_time: ops () is not a set of %s" % NAMES, f, (), 3)
    for w in (0, -1, 65536, 2.0, True, None, "5"):
        raises("rolling_time: window %r outside 1 .. 65535" % (w,), f, "max", w)
        raises("rolling_time: window %r outside 1 .. 65535" % (w,), g, "max", lab, w)
    for mc in (0, 6, -1, 2.0, False):
        raises("rolling_time: min_count %r outside 1 .. window 5" % (mc,), f, "max", 5, mc)
        raises("rolling_time: min_count %r outside 1 .. window 5" % (mc,), g, "max", lab, 5, mc)
    raises("rolling_time: the mean takes whole windows, min_count 4 is not window 5", f, "max", 5, 4, True)
    raises("rolling_time: the mean takes whole windows, min_count 1 is not window 2", g, "max", lab, 2, 1, mean=True)
    raises("instants [5, 4) outside [0, 10)", f, "max", 3, start=5, stop=4)
    raises("window (0:51, 0:60) outside the raster's 50 x 60 cells", f, "max", 3, region=(0, 51, 0, 60))
    # grouped: the statistics first, then the window, then the labels and n_groups
    raises("rolling_time: unknown statistic 'median' (one of %s)" % NAMES, g, "median", np.zeros(2), 0, n_groups=0)
    raises("rolling_time: window 0 outside 1 .. 65535", g, "max", np.zeros(2), 0, n_groups=0)
    raises("rolling_time_groups: the labels are float64 (2,), the instants uint16 (10,)", g, "max", np.zeros(2), 3, n_groups=0)
    raises("rolling_time_groups: n_groups 0 outside 1 .. 65535", g, "max", lab, 3, n_groups=0)
    raises("rolling_time_groups: n_groups 65536 outside 1 .. 65535", g, "max", lab, 3, n_groups=65536)
    # the flat forms
    a = np.zeros(3, dtype=np.uint16)
    labels = [a, a, a[:0], lab, a[:1]]
    ff, gg = R.rolling_time_flat, R.rolling_time_groups_flat
    raises("rolling_time: ops 32 is not a set of %s" % NAMES, ff, CUBES, 32, 3)
    raises("rolling_time: window 65536 outside 1 .. 65535", ff, CUBES, 31, 65536)
    raises("rolling_time: min_count 4 outside 1 .. window 3", ff, CUBES, 31, 3, 4)
    raises("rolling_time: the mean takes whole windows, min_count 2 is not window 3", ff, CUBES, 31, 3, 2, True)
    raises("rolling_time: ops 0 is not a set of %s" % NAMES, gg, CUBES, 0, [], 0, 0)
    raises("rolling_time: window 0 outside 1 .. 65535", gg, CUBES, 31, [], 0, 0)
    raises("rolling_time_groups: n_groups 0 outside 1 .. 65535", gg, CUBES, 31, [], 0, 3)
    raises("rolling_time_groups: 0 label arrays for 5 cubes", gg, CUBES, 31, [], 3, 3)
    raises("rolling_time_groups: labels 1 are int64, not uint16", gg, CUBES, 31, [a, np.zeros(3, dtype=np.int64)] + labels[2:], 3, 3)
    raises("rolling_time_groups: labels 4 have shape (2,), their cube 1 instants", gg, CUBES, 31, labels[:4] + [a[:2]], 3, 3)
    assert stub.calls == []  # nothing reached the library


def _filled(d, names, shape):
    assert list(d) == names
    for n, v in d.items():
        assert v.shape == shape and v.dtype == np.float64, (n, v.shape, v.dtype)
        if n == "count":
            assert (v == 0).all() and not np.signbit(v).any()
        else:
            assert np.isnan(v).all(), n


def test_nothing_to_read(stubbed):
    R, stub = stubbed
    lab10 = np.zeros(10, dtype=np.uint16)
    for kw in (dict(start=3, stop=3), dict(start=10), dict(region=(5, 5, 0, 60)), dict(region=(0, 50, 60, 60))):
        rows, cols = (kw["region"][1] - kw["region"][0], kw["region"][3] - kw["region"][2]) if "region" in kw else (50, 60)
        lab = lab10 if "region" in kw else lab10[:0]
        _filled(R.rolling_time(31, 3, **kw), list(WM.NAMES), (rows, cols))
        _filled(R.rolling_time("argmin", 3, 1, **kw), ["argmin"], (rows, cols))
        _filled(R.rolling_time_groups(31, lab, 4, mean=True, n_groups=3, **kw), list(WM.NAMES), (3, rows, cols))
        _filled(R.rolling_time_groups(("count", "max"), lab, 2, **kw), ["max", "count"], (1, rows, cols))
        raises("rolling_time: window 0 outside 1 .. 65535", R.rolling_time, 31, 0, **kw)  # the checks come first
    assert stub.calls == []


# ---- Variable ----------------------------------------------------------------------------------------------------------------------
def test_variable_forms(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd import dataset as D
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    made = []

    class FakeVar:
        """Variable's two methods over a shape alone; its raster's library is the stub."""
        rolling_time = D.Variable.rolling_time
        rolling_time_groups = D.Variable.rolling_time_groups
        _region = D.Variable._region
        _check = D.Variable._check

        def __init__(self, shape):
            self.shape = shape

        def raster(self):
            R = EncodedRaster(self.shape, [None], tile=1 << 20, chunk_size=32)
            R._native = C.c_void_p(1)
            made.append(R)
            return R

    try:
        v = FakeVar((10, 50, 60))
        d = v.rolling_time(5, 31)
        c = stub.calls[0]
        assert c["name"] == "plain" and c["q"].tolist() == [[0, 10, 0, 50, 0, 60]] and list(d) == list(WM.NAMES) and (c["w"], c["mc"], c["kind"]) == (5, 5, 0)
        d = v.rolling_time(window=3, min_count=1, start=2, stop=8, top=4, left=50)  # the default: the greatest sum
        c = stub.calls[1]
        assert c["ops"] == 1 and c["q"].tolist() == [[2, 8, 4, 50, 50, 60]] and d["max"].shape == (46, 10) and (c["w"], c["mc"]) == (3, 1)
        ids_in = np.array([12, -1, 3, 12, 700000, 3, -5, 12, 3, 3])
        ids, d = v.rolling_time_groups(ids_in, 2, ("min", "argmax"), mean=True)
        c = stub.calls[2]
        assert ids.tolist() == [3, 12, 700000] and c["name"] == "groups" and c["n_groups"] == 3 and c["ops"] == 6 and (c["w"], c["mc"], c["kind"]) == (2, 2, 1)
        assert c["labels"][0].tolist() == [1, 0xffff, 0, 1, 2, 0, 0xffff, 1, 0, 0]
        assert list(d) == ["argmax", "min"] and all(x.shape == (3, 50, 60) for x in d.values())
        ids, d = v.rolling_time_groups(ids_in[4:6], 1, start=4, stop=6)
        assert ids.tolist() == [3, 700000] and stub.calls[3]["labels"][0].tolist() == [1, 0] and list(d) == ["max"]
        assert len(stub.calls) == 4
        # nothing to read: the fills, after the checks
        _filled(v.rolling_time(3, 31, start=4, stop=4), list(WM.NAMES), (50, 60))
        _filled(v.rolling_time(3, "argmin", top=7, bottom=7), ["argmin"], (0, 60))
        ids, d = v.rolling_time_groups(np.full(10, -1), 3, 31)
        assert ids.size == 0
        _filled(d, list(WM.NAMES), (0, 50, 60))
        ids, d = v.rolling_time_groups(ids_in[:0], 3, "count", start=10)
        assert ids.size == 0 and d["count"].shape == (0, 50, 60)
        ids, d = v.rolling_time_groups(ids_in, 3, 31, left=60)
        assert ids.tolist() == [3, 12, 700000]
        _filled(d, list(WM.NAMES), (3, 50, 0))
        assert len(stub.calls) == 4
        raises("rolling_time: unknown statistic 'mean' (one of %s)" % NAMES, v.rolling_time, 3, "mean")
        raises("rolling_time: window 0 outside 1 .. 65535", v.rolling_time, 0)
        raises("rolling_time: window 0 outside 1 .. 65535", v.rolling_time, 0, start=3, stop=3)
        raises("rolling_time: min_count 4 outside 1 .. window 3", v.rolling_time_groups, ids_in, 3, "max", 4)
        raises("rolling_time: the mean takes whole windows, min_count 1 is not window 3", v.rolling_time, 3, "max", 1, True)
        raises("rolling_time_groups: the labels are float64 (2,), the instants integers (10,)", v.rolling_time_groups, np.zeros(2), 3)
        with pytest.raises(IndexError):
            v.rolling_time(3, stop=11)
        assert len(stub.calls) == 4
    finally:
        for R in made:
            R._native = None
