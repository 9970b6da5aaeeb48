"""The raster calls of the regression over time without a GPU: tests/sim/regress_stream_check.cpp runs plan_regress_time and the cell
body of k_regress_stream (regress_cell, k2r_regress.h) on the CPU under AddressSanitizer and UBSan, exactly as the kernel indexes
them; the two entry points are declared, exported and listed; and the Python layer -- EncodedRaster.regress_time*, Variable's methods
of the same names -- is run against a stubbed library: the argument order of both entries, plane counts and offsets, the shifted
regressor of the whole-raster forms against the as-given one of the flat forms, every ValueError, and the fills where nothing is
read."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import regress_model as RM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = "count, slope, intercept, corr"


def test_plan_and_cell_body_in_a_sanitized_stand_alone_program(tmp_path):
    """Every slab read inside the band's used elements, every output element written exactly once and nothing else, the bits of a
    loop written apart from the header: 160 cases over four geometries, three slab caps, five label sets."""
    exe = str(tmp_path / "regress_stream_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", exe,
                           os.path.join(HERE, "sim", "regress_stream_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    words = out.stdout.split()
    assert words[:2] == ["ok", "stream"] and int(words[2]) == 160 and int(words[3]) > 1_000_000 and int(words[4]) > int(words[3]), out.stdout


def test_symbols_declared_exported_and_listed():
    from dcdf_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read())
    assert ("int dcdf_raster_regress_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const double* regressor, "
            "const uint64_t* regressor_offset, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);") in hdr
    assert ("int dcdf_raster_regress_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, "
            "const double* regressor, const uint64_t* regressor_offset, const uint16_t* labels, const uint64_t* label_offset, "
            "uint32_t n_groups, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);") in hdr
    assert "not part of this library yet" not in hdr
    assert "No kernel runs them yet" not in open(os.path.join(ROOT, "dcdf_amd", "csrc", "k2r_regress.h")).read()
    assert "dcdf_raster_regress_time_batch" in _lib.SYMBOLS and "dcdf_raster_regress_time_groups_batch" in _lib.SYMBOLS
    assert os.path.exists(_lib.LIB_PATH), "library not built"
    lib = _lib.lib()  # (loading needs no GPU)
    assert lib.dcdf_raster_regress_time_batch and lib.dcdf_raster_regress_time_groups_batch
    assert len(lib.dcdf_raster_regress_time_batch.argtypes) == 11 and len(lib.dcdf_raster_regress_time_groups_batch.argtypes) == 14
    assert lib.dcdf_abi_version() == 3  # added entry points: the ABI version stays
    assert _lib.REGRESS_OPS == RM.BITS and list(_lib.REGRESS_OPS) == list(RM.NAMES)


# ---- the Python layer against a stubbed library -------------------------------------------------------------------------------------
def _u64(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(max(n, 1),))[:n].copy()


class _Stub:
    """Stands in for the loaded library: records what the two entry points are called with, in the C order of their arguments."""

    def __init__(self):
        self.calls = []

    def _record(self, name, cubes, nq, ops, reg, roff, lab, loff, n_groups, out, mem, off, stats):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        nt = np.abs(q[:, 1].astype(np.int64) - q[:, 0])
        regs = labels = None
        if reg is not None or roff is not None:
            ro = _u64(roff, nq)
            flat = np.ctypeslib.as_array(C.cast(reg, C.POINTER(C.c_double)), shape=(int(ro[-1] + nt[-1]) + 1,))
            regs = [flat[int(ro[i]):int(ro[i]) + int(nt[i])].copy() for i in range(nq)]
        if lab is not None:
            lo = _u64(loff, nq)
            flat = np.ctypeslib.as_array(C.cast(lab, C.POINTER(C.c_uint16)), shape=(int(lo[-1] + nt[-1]) + 1,))
            labels = [flat[int(lo[i]):int(lo[i]) + int(nt[i])].copy() for i in range(nq)]
        self.calls.append(dict(name=name, q=q, ops=ops.value, regs=regs, labels=labels, n_groups=n_groups, mem=mem, out=out.value, off=_u64(off, nq)))
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0

    def dcdf_raster_regress_time_batch(self, h, cubes, nq, ops, reg, roff, out, mem, off, stats, ms):
        return self._record("plain", cubes, nq, ops, reg, roff, None, None, None, out, mem, off, stats)

    def dcdf_raster_regress_time_groups_batch(self, h, cubes, nq, ops, reg, roff, lab, loff, n_groups, out, mem, off, stats, ms):
        return self._record("groups", cubes, nq, ops, reg, roff, lab, loff, n_groups.value, out, mem, off, stats)


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


def test_flat_forms_pass_the_regressor_as_given(stubbed):
    R, stub = stubbed
    regs = [1990.0 + np.arange(n) * 0.5 for n in NT]
    labels = [(np.arange(n) % 2).astype(np.uint16) for n in NT]
    for ops, n in ((15, 4), ("slope", 1), (("corr", "count"), 2), (6, 2)):
        stub.calls.clear()
        flat, off, ms, stats = R.regress_time_flat(CUBES, ops, regs)
        c = stub.calls[0]
        assert c["name"] == "plain" and c["ops"] == R.regress_ops(ops)[0] and c["mem"] == 0 and c["labels"] is None
        np.testing.assert_array_equal(c["q"], CUBES)  # (the library normalises reversed bounds itself)
        np.testing.assert_array_equal(off, [0, 35 * n, 175 * n, 175 * n, 3175 * n])
        np.testing.assert_array_equal(c["off"], off)
        assert flat.dtype == np.float64 and flat.size == 3175 * n and stats.tolist() == [5, 6, 7]
        for got, want in zip(c["regs"], regs):
            np.testing.assert_array_equal(got, want)  # as given: nothing subtracted
        flat, off, ms, stats = R.regress_time_groups_flat(CUBES, ops, labels, 3, regs)
        c = stub.calls[1]
        assert c["name"] == "groups" and c["ops"] == R.regress_ops(ops)[0] and c["n_groups"] == 3
        np.testing.assert_array_equal(off, [0, 105 * n, 525 * n, 525 * n, 9525 * n])
        assert flat.size == 9525 * n
        for got, want in zip(c["regs"], regs):
            np.testing.assert_array_equal(got, want)
        for got, want in zip(c["labels"], labels):
            np.testing.assert_array_equal(got, want)
    stub.calls.clear()
    R.regress_time_flat(CUBES, 15)  # no regressor: NULL and NULL, the instant index is the library's
    R.regress_time_groups_flat(CUBES, 15, labels, 2)
    assert stub.calls[0]["regs"] is None and stub.calls[1]["regs"] is None and stub.calls[1]["labels"] is not None
    R.regress_time_flat(CUBES, 2, [np.arange(n) for n in NT])  # integers are real numbers
    assert stub.calls[2]["regs"][3].dtype == np.float64 and stub.calls[2]["regs"][3].tolist() == list(range(10))
    # device form: the caller's offsets go through untouched
    stub.calls.clear()
    ms, stats = R.regress_time_groups_flat(CUBES, "corr", labels, 2, regs, out_device_ptr=4096, out_offset=[9, 200, 700, 701, 40000])
    c = stub.calls[0]
    assert (c["mem"], c["out"]) == (1, 4096) and c["off"].tolist() == [9, 200, 700, 701, 40000] and stats.tolist() == [5, 6, 7]


def test_whole_raster_forms_pass_the_regressor_less_its_first_value(stubbed):
    R, stub = stubbed
    years = 1979.25 + np.array([0, 1, 2, 4, 3, 5, 9, 7, 8, 6]) * 1.1
    d = R.regress_time(15, years)
    c = stub.calls[0]
    assert c["name"] == "plain" and c["q"].tolist() == [[0, 10, 0, 50, 0, 60]] and c["ops"] == 15
    np.testing.assert_array_equal(RM.bits(c["regs"][0]), RM.bits(RM.shifted(years)))
    assert c["regs"][0][0] == 0 and (c["regs"][0] != years).all()
    assert list(d) == list(RM.NAMES) and all(v.shape == (50, 60) and v.dtype == np.float64 for v in d.values())
    d = R.regress_time(regressor=years[2:7], start=2, stop=7, window=(3, 10, 20, 60))
    c = stub.calls[1]
    assert c["q"].tolist() == [[2, 7, 3, 10, 20, 60]] and c["ops"] == 2 and list(d) == ["slope"] and d["slope"].shape == (7, 40)
    np.testing.assert_array_equal(RM.bits(c["regs"][0]), RM.bits(years[2:7] - years[2]))
    R.regress_time("corr")  # the instant index: nothing to shift, NULL
    assert stub.calls[2]["regs"] is None
    lab = np.array([0, 2, 2, 0xffff, 0, 2, 0, 0, 2, 5], dtype=np.uint16)
    d = R.regress_time_groups(("intercept", "slope"), lab, years)
    c = stub.calls[3]
    assert c["name"] == "groups" and c["n_groups"] == 6 and c["ops"] == 6 and c["labels"][0].tolist() == lab.tolist()
    np.testing.assert_array_equal(RM.bits(c["regs"][0]), RM.bits(RM.shifted(years)))
    assert list(d) == ["slope", "intercept"] and all(v.shape == (6, 50, 60) for v in d.values())
    d = R.regress_time_groups("count", lab[1:4], None, 1, 4, n_groups=2)
    c = stub.calls[4]
    assert c["regs"] is None and c["n_groups"] == 2 and c["q"].tolist() == [[1, 4, 0, 50, 0, 60]] and d["count"].shape == (2, 50, 60)
    assert len(stub.calls) == 5


def test_every_refusal(stubbed):
    R, stub = stubbed
    f, g = R.regress_time, R.regress_time_groups
    lab = np.zeros(10, dtype=np.uint16)
    raises("regress_time: unknown statistic 'mean' (one of %s)" % NAMES, f, "mean")
    raises("regress_time: unknown statistic 'std' (one of %s)" % NAMES, f, ("slope", "std"))
    raises("regress_time: ops 16 is not a set of %s" % NAMES, f, 16)
    raises("regress_time: ops 32 is not a set of %s" % NAMES, f, 32)
    raises("regress_time: ops 0 is not a set of %s" % NAMES, f, 0)
    raises("regress_time: ops () is not a set of %s" % NAMES, f, ())
    raises("instants [5, 4) outside [0, 10)", f, "slope", np.zeros(3), 5, 4)
    raises("window (0:51, 0:60) outside the raster's 50 x 60 cells", f, "slope", np.zeros(3), window=(0, 51, 0, 60))
    raises("regress_time: the regressor is float64 (3,), the instants real numbers (10,)", f, "slope", np.zeros(3))
    raises("regress_time: the regressor is float64 (10,), the instants real numbers (4,)", f, "slope", np.zeros(10), 3, 7)
    raises("regress_time: the regressor is float64 (10, 1), the instants real numbers (10,)", f, "slope", np.zeros((10, 1)))
    raises("regress_time: the regressor is bool (10,), the instants real numbers (10,)", f, "slope", np.zeros(10, dtype=bool))
    raises("regress_time: the regressor is complex128 (10,), the instants real numbers (10,)", f, "slope", np.zeros(10, dtype=complex))
    raises("regress_time: the regressor is float64 (1,), the instants real numbers (0,)", f, "slope", np.zeros(1), 4, 4)
    for bad in (np.nan, np.inf, -np.inf):
        u = np.arange(10.0)
        u[6] = bad
        raises("regress_time: the regressor has a value that is not finite", f, "slope", u)
        raises("regress_time: the regressor has a value that is not finite", f, "slope", u, window=(5, 5, 0, 60))
        raises("regress_time_groups: the regressor has a value that is not finite", g, "slope", lab, u)
    # grouped: the statistics, the labels, n_groups, the regressor
    raises("regress_time: unknown statistic 'median' (one of %s)" % NAMES, g, "median", np.zeros(2), np.zeros(2), n_groups=0)
    raises("regress_time_groups: the labels are float64 (2,), the instants uint16 (10,)", g, "slope", np.zeros(2), np.zeros(2), n_groups=0)
    raises("regress_time_groups: n_groups 0 outside 1 .. 65535", g, "slope", lab, np.zeros(2), n_groups=0)
    raises("regress_time_groups: n_groups 65536 outside 1 .. 65535", g, "slope", lab, n_groups=65536)
    raises("regress_time_groups: the regressor is float64 (2,), the instants real numbers (10,)", g, "slope", lab, np.zeros(2))
    # the flat forms
    a = np.zeros(3, dtype=np.uint16)
    labels = [a, a, a[:0], lab, a[:1]]
    regs = [np.zeros(n) for n in NT]
    ff, gg = R.regress_time_flat, R.regress_time_groups_flat
    raises("regress_time: ops 16 is not a set of %s" % NAMES, ff, CUBES, 16, [])
    raises("regress_time: 0 regressors for 5 cubes", ff, CUBES, 15, [])
    raises("regress_time: 6 regressors for 5 cubes", ff, CUBES, 15, regs + regs[:1])
    raises("regress_time: the regressor 1 is float64 (4,), the instants real numbers (3,)", ff, CUBES, 15, [regs[0], np.zeros(4)] + regs[2:])
    raises("regress_time: the regressor 2 is float64 (1,), the instants real numbers (0,)", ff, CUBES, 15, regs[:2] + [np.zeros(1)] + regs[3:])
    raises("regress_time: the regressor 0 is <U1 (3,), the instants real numbers (3,)", ff, CUBES, 15, [np.array(["a", "b", "c"])] + regs[1:])
    raises("regress_time: the regressor 3 has a value that is not finite", ff, CUBES, 15, regs[:3] + [np.full(10, np.nan)] + regs[4:])
    raises("regress_time: ops 0 is not a set of %s" % NAMES, gg, CUBES, 0, [], 0, [])
    raises("regress_time_groups: n_groups 0 outside 1 .. 65535", gg, CUBES, 15, [], 0, [])
    raises("regress_time_groups: 0 label arrays for 5 cubes", gg, CUBES, 15, [], 3, [])
    raises("regress_time_groups: labels 1 are int64, not uint16", gg, CUBES, 15, [a, np.zeros(3, dtype=np.int64)] + labels[2:], 3, [])
    raises("regress_time_groups: 0 regressors for 5 cubes", gg, CUBES, 15, labels, 3, [])
    raises("regress_time_groups: the regressor 4 is float64 (2,), the instants real numbers (1,)", gg, CUBES, 15, labels, 3, regs[:4] + [np.zeros(2)])
    raises("regress_time_groups: the regressor 0 has a value that is not finite", gg, CUBES, 15, labels, 3, [np.array([0, np.inf, 1])] + regs[1:])
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
    for kw in (dict(start=3, stop=3), dict(start=10), dict(window=(5, 5, 0, 60)), dict(window=(0, 50, 60, 60))):
        rows, cols = (kw["window"][1] - kw["window"][0], kw["window"][3] - kw["window"][2]) if "window" in kw else (50, 60)
        lab = lab10 if "window" in kw else lab10[:0]
        u = np.arange(10.0) + 7 if "window" in kw else np.zeros(0)
        _filled(R.regress_time(15, **kw), list(RM.NAMES), (rows, cols))
        _filled(R.regress_time(regressor=u, **kw), ["slope"], (rows, cols))
        _filled(R.regress_time_groups(15, lab, u, n_groups=3, **kw), list(RM.NAMES), (3, rows, cols))
        _filled(R.regress_time_groups(("corr", "count"), lab, **kw), ["count", "corr"], (1, rows, cols))
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
        regress_time = D.Variable.regress_time
        regress_time_groups = D.Variable.regress_time_groups
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
        years = 2001.5 + np.arange(10) * np.array([1, -1] * 5)
        d = v.regress_time(15, years)
        c = stub.calls[0]
        assert c["name"] == "plain" and c["q"].tolist() == [[0, 10, 0, 50, 0, 60]] and list(d) == list(RM.NAMES)
        np.testing.assert_array_equal(RM.bits(c["regs"][0]), RM.bits(RM.shifted(years)))
        d = v.regress_time(start=2, stop=8, top=4, left=50)  # the default: the slope against the instant index
        c = stub.calls[1]
        assert c["regs"] is None and c["ops"] == 2 and c["q"].tolist() == [[2, 8, 4, 50, 50, 60]] and d["slope"].shape == (46, 10)
        ids_in = np.array([12, -1, 3, 12, 700000, 3, -5, 12, 3, 3])
        ids, d = v.regress_time_groups(ids_in, ("corr", "slope"), years)
        c = stub.calls[2]
        assert ids.tolist() == [3, 12, 700000] and c["name"] == "groups" and c["n_groups"] == 3 and c["ops"] == 10
        assert c["labels"][0].tolist() == [1, 0xffff, 0, 1, 2, 0, 0xffff, 1, 0, 0]
        np.testing.assert_array_equal(RM.bits(c["regs"][0]), RM.bits(RM.shifted(years)))
        assert list(d) == ["slope", "corr"] and all(x.shape == (3, 50, 60) for x in d.values())
        ids, d = v.regress_time_groups(ids_in[4:6], start=4, stop=6)
        assert ids.tolist() == [3, 700000] and stub.calls[3]["regs"] is None and stub.calls[3]["labels"][0].tolist() == [1, 0]
        assert len(stub.calls) == 4
        # nothing to read: the fills, after the checks
        _filled(v.regress_time(15, start=4, stop=4), list(RM.NAMES), (50, 60))
        _filled(v.regress_time(15, years[:0], start=4, stop=4), list(RM.NAMES), (50, 60))
        _filled(v.regress_time("corr", years, top=7, bottom=7), ["corr"], (0, 60))
        ids, d = v.regress_time_groups(np.full(10, -1), 15, years)
        assert ids.size == 0
        _filled(d, list(RM.NAMES), (0, 50, 60))
        ids, d = v.regress_time_groups(ids_in[:0], "count", start=10)
        assert ids.size == 0 and d["count"].shape == (0, 50, 60)
        ids, d = v.regress_time_groups(ids_in, 15, years, left=60)
        assert ids.tolist() == [3, 12, 700000]
        _filled(d, list(RM.NAMES), (3, 50, 0))
        assert len(stub.calls) == 4
        raises("regress_time: unknown statistic 'mean' (one of %s)" % NAMES, v.regress_time, "mean")
        raises("regress_time: the regressor is float64 (10,), the instants real numbers (4,)", v.regress_time, "slope", years, 3, 7)
        raises("regress_time: the regressor is float64 (10,), the instants real numbers (0,)", v.regress_time, "slope", years, 3, 3)
        raises("regress_time_groups: the labels are float64 (2,), the instants integers (10,)", v.regress_time_groups, np.zeros(2), "slope", years[:2])
        raises("regress_time_groups: the regressor is float64 (2,), the instants real numbers (10,)", v.regress_time_groups, ids_in, "slope", years[:2])
        raises("regress_time_groups: the regressor is float64 (2,), the instants real numbers (10,)", v.regress_time_groups, np.full(10, -1), "slope", years[:2])
        raises("regress_time_groups: the regressor is float64 (10,), the instants real numbers (0,)", v.regress_time_groups, ids_in[:0], "slope", years, 5, 5)
        with pytest.raises(IndexError):
            v.regress_time(stop=11)
        assert len(stub.calls) == 4
    finally:
        for R in made:
            R._native = None
