"""What the Python layer of the grouped folds over time (EncodedRaster.reduce_time_groups, moments_time, moments_time_groups, their
*_flat forms, zonal's label and n_zones checks, and Variable's methods of the same names) checks before the library is called,
without a GPU: every message, which one speaks when several arguments are wrong, and what comes back -- dtype, shape, fill
value -- when there is nothing to read."""
import re

import numpy as np
import pytest

from dcdf_amd import _lib
from dcdf_amd import dataset as D
from dcdf_amd.raster import EncodedRaster

NONE = _lib.GROUP_NONE
LAB = np.zeros(10, dtype=np.uint16)
ZLAB = np.zeros((50, 60), dtype=np.uint16)
REDUCE = "min, max, sum, count, mean"
MOMENT = "count, mean, var, std"


@pytest.fixture()
def raster():
    """10 instants of 50 x 60 cells; no test here reaches the library."""
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    yield R
    R._native = None


def raises(msg, f, *a, **k):
    with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
        f(*a, **k)


# ---- EncodedRaster: the whole-raster methods ---------------------------------------------------------------------------------------
# each call with arguments that are wrong in every later check too: instants, window, then the call's own in their order
def _calls(R):
    bad = np.zeros(2)
    return {
        "reduce_time_groups": lambda **k: R.reduce_time_groups("median", bad, n_groups=0, **k),
        "moments_time": lambda **k: R.moments_time("median", ddof=2, **k),
        "moments_time_groups": lambda **k: R.moments_time_groups("median", bad, n_groups=0, ddof=2, **k),
        "zonal": lambda **k: R.zonal("median", bad, n_zones=0, **k),
    }


@pytest.mark.parametrize("name", ["reduce_time_groups", "moments_time", "moments_time_groups", "zonal"])
def test_instants_then_window_come_first(raster, name):
    f = _calls(raster)[name]
    bad_window = (0, 51, 0, 60)
    raises("instants [5, 4) outside [0, 10)", f, start=5, stop=4, window=bad_window)
    raises("instants [0, 11) outside [0, 10)", f, stop=11, window=bad_window)
    raises("window (0:51, 0:60) outside the raster's 50 x 60 cells", f, window=bad_window)
    raises("window (0:50, 7:6) outside the raster's 50 x 60 cells", f, start=3, stop=3, window=(0, 50, 7, 6))


def test_reduce_time_groups_checks_in_order(raster):
    R = raster
    f = R.reduce_time_groups
    raises("reduce_time: unknown statistic 'median' (one of %s)" % REDUCE, f, "median", np.zeros(2), n_groups=0)
    raises("reduce_time: ops 0 is not a set of %s" % REDUCE, f, 0, np.zeros(2), n_groups=0)
    raises("reduce_time_groups: the labels are float64 (2,), the instants uint16 (10,)", f, "sum", np.zeros(2), n_groups=0)
    raises("reduce_time_groups: the labels are int32 (10,), the instants uint16 (10,)", f, "sum", LAB.astype(np.int32), n_groups=0)
    raises("reduce_time_groups: the labels are uint16 (10,), the instants uint16 (4,)", f, "sum", LAB, 3, 7, n_groups=0)
    raises("reduce_time_groups: the labels are uint16 (10, 1), the instants uint16 (10,)", f, "sum", LAB.reshape(10, 1))
    raises("reduce_time_groups: the labels are uint16 (1,), the instants uint16 (0,)", f, "sum", LAB[:1], 4, 4, n_groups=70000)
    raises("reduce_time_groups: n_groups 0 outside 1 .. 65535", f, "sum", LAB, n_groups=0)
    raises("reduce_time_groups: n_groups 65536 outside 1 .. 65535", f, "sum", LAB[:0], 2, 2, n_groups=65536)
    raises("reduce_time_groups: n_groups -3 outside 1 .. 65535", f, "sum", LAB, window=(5, 5, 0, 60), n_groups=-3)


def test_moments_checks_in_order(raster):
    R = raster
    f, g = R.moments_time, R.moments_time_groups
    raises("moments_time: unknown statistic 'median' (one of %s)" % MOMENT, f, "median", ddof=2)
    raises("moments_time: unknown statistic 'min' (one of %s)" % MOMENT, f, ("mean", "min"), ddof=2)
    raises("moments_time: ops 16 is not a set of %s" % MOMENT, f, 16, ddof=2)
    raises("moments_time: ops 32 is not a set of %s" % MOMENT, f, 32, ddof=2)
    raises("moments_time: ops 0 is not a set of %s" % MOMENT, f, 0)
    raises("moments_time: ops () is not a set of %s" % MOMENT, f, ())
    raises("moments_time: ddof 2 is neither 0 nor 1", f, "var", ddof=2)
    raises("moments_time: ddof True is neither 0 nor 1", f, "var", 3, 3, ddof=True)
    raises("moments_time: ddof 1.0 is neither 0 nor 1", f, "var", ddof=1.0)
    raises("moments_time: ddof -1 is neither 0 nor 1", f, "var", window=(5, 5, 0, 60), ddof=-1)
    # grouped: the statistics, ddof, the labels, n_groups
    raises("moments_time: unknown statistic 'median' (one of %s)" % MOMENT, g, "median", np.zeros(2), n_groups=0, ddof=2)
    raises("moments_time: ops 17 is not a set of %s" % MOMENT, g, 17, np.zeros(2), n_groups=0, ddof=2)
    raises("moments_time: ddof 2 is neither 0 nor 1", g, "var", np.zeros(2), n_groups=0, ddof=2)
    raises("moments_time_groups: the labels are float64 (2,), the instants uint16 (10,)", g, "var", np.zeros(2), n_groups=0)
    raises("moments_time_groups: the labels are int64 (10,), the instants uint16 (10,)", g, "var", LAB.astype(np.int64), n_groups=0)
    raises("moments_time_groups: the labels are uint16 (10,), the instants uint16 (4,)", g, "var", LAB, 3, 7, n_groups=0, ddof=1)
    raises("moments_time_groups: the labels are uint16 (1,), the instants uint16 (0,)", g, "var", LAB[:1], 4, 4, n_groups=70000)
    raises("moments_time_groups: n_groups 0 outside 1 .. 65535", g, "var", LAB, n_groups=0)
    raises("moments_time_groups: n_groups 65536 outside 1 .. 65535", g, "var", LAB[:0], 2, 2, n_groups=65536, ddof=1)
    assert EncodedRaster.moment_ops(15) == (15, ["count", "mean", "var", "std"]) and EncodedRaster.moment_ops(["std", "count"]) == (9, ["count", "std"])
    assert EncodedRaster.moment_ops(np.uint32(6)) == (6, ["mean", "var"]) and EncodedRaster.moment_ops("var") == (4, ["var"])


def test_zonal_label_and_n_zones_checks(raster):
    R = raster
    raises("reduce_time: unknown statistic 'median' (one of %s)" % REDUCE, R.zonal, "median", np.zeros((2, 2)), n_zones=0)
    raises("zonal: the labels are float64 (2, 2), the window uint16 (50, 60)", R.zonal, "sum", np.zeros((2, 2)), n_zones=0)
    raises("zonal: the labels are uint16 (50, 60), the window uint16 (7, 40)", R.zonal, "sum", ZLAB, window=(3, 10, 20, 60), n_zones=0)
    raises("zonal: the labels are int32 (50, 60), the window uint16 (50, 60)", R.zonal, "sum", ZLAB.astype(np.int32))
    raises("zonal: n_zones 0 outside 1 .. 65535", R.zonal, "sum", ZLAB, n_zones=0)
    raises("zonal: n_zones 65536 outside 1 .. 65535", R.zonal, "sum", ZLAB, 2, 2, n_zones=65536)
    raises("zonal: n_zones -1 outside 1 .. 65535", R.zonal, "sum", ZLAB, n_zones=-1)
    cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10]]
    a, b = np.zeros((5, 7), dtype=np.uint16), np.zeros((7, 20), dtype=np.uint16)
    raises("reduce_time: ops 0 is not a set of %s" % REDUCE, R.zonal_flat, cubes, 0, [], 0)
    raises("zonal: n_zones 0 outside 1 .. 65535", R.zonal_flat, cubes, "sum", [], 0)
    raises("zonal: n_zones 65536 outside 1 .. 65535", R.zonal_flat, cubes, "sum", [a], 65536)
    raises("zonal: 1 label arrays for 2 cubes", R.zonal_flat, cubes, "sum", [a], 3)
    raises("zonal: labels 1 are int64, not uint16", R.zonal_flat, cubes, "sum", [a, np.zeros((9, 9), dtype=np.int64)], 3)
    raises("zonal: labels 1 have shape (20, 7), their cube (7, 20)", R.zonal_flat, cubes, "sum", [a, b.T], 3)
    raises("zonal: labels 0 are uint8, not uint16", R.zonal_flat, cubes, "sum", [a.astype(np.uint8), b.T], 3)
    raises("zonal: 1 label offsets for 2 cubes", R.zonal_flat, cubes, "sum", (4096, [5]), 3)
    # n_zones defaults to the largest label below ZONE_NONE, plus 1; at least 1
    lab = ZLAB.copy()
    assert R.zonal("min", lab, 2, 2)["min"].shape == (1, 0)
    lab[3, 4], lab[0, 0] = 11, _lib.ZONE_NONE
    z = R.zonal(("count", "min"), lab, 2, 2)
    assert list(z) == ["min", "count"] and all(v.shape == (12, 0) and v.dtype == np.float64 for v in z.values())
    assert R.zonal("min", np.full((50, 60), _lib.ZONE_NONE, dtype=np.uint16), 2, 2)["min"].shape == (1, 0)
    assert R.zonal("min", lab, 2, 2, n_zones=4)["min"].shape == (4, 0)


# ---- EncodedRaster: the flat forms -------------------------------------------------------------------------------------------------
def test_flat_forms_check_before_the_call(raster):
    R = raster
    cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10]]  # 3 instants each, the second with reversed bounds
    a = np.zeros(3, dtype=np.uint16)
    f = R.reduce_time_groups_flat
    raises("reduce_time: ops 0 is not a set of %s" % REDUCE, f, cubes, 0, [], 0)
    raises("reduce_time: unknown statistic 'var' (one of %s)" % REDUCE, f, cubes, "var", [], 0)
    raises("reduce_time_groups: n_groups 0 outside 1 .. 65535", f, cubes, "sum", [], 0)
    raises("reduce_time_groups: n_groups 65536 outside 1 .. 65535", f, cubes, "sum", [a], 65536)
    raises("reduce_time_groups: 0 label arrays for 2 cubes", f, cubes, "sum", [], 3)
    raises("reduce_time_groups: 3 label arrays for 2 cubes", f, cubes, "sum", [a, a, a], 3)
    raises("reduce_time_groups: labels 1 are int64, not uint16", f, cubes, "sum", [a, np.zeros(9, dtype=np.int64)], 3)  # (the dtype first)
    raises("reduce_time_groups: labels 0 are float64, not uint16", f, cubes, "sum", [np.zeros(3), np.zeros(9, dtype=np.int64)], 3)
    raises("reduce_time_groups: labels 1 have shape (4,), their cube 3 instants", f, cubes, "sum", [a, np.zeros(4, dtype=np.uint16)], 3)
    raises("reduce_time_groups: labels 0 have shape (3, 1), their cube 3 instants", f, cubes, "sum", [a.reshape(3, 1), a[:2]], 3)
    raises("reduce_time_groups: labels 0 have shape (3,), their cube 0 instants", f, [[2, 2, 0, 5, 0, 7]], "sum", [a], 3)
    g = R.moments_time_flat
    raises("moments_time: ops 16 is not a set of %s" % MOMENT, g, cubes, 16, 2)
    raises("moments_time: unknown statistic 'sum' (one of %s)" % MOMENT, g, cubes, "sum", 2)
    raises("moments_time: ddof 2 is neither 0 nor 1", g, cubes, "std", 2)
    raises("moments_time: ddof None is neither 0 nor 1", g, cubes, "std", None)
    h = R.moments_time_groups_flat
    raises("moments_time: ops 0 is not a set of %s" % MOMENT, h, cubes, 0, [], 0, 2)
    raises("moments_time: ddof 2 is neither 0 nor 1", h, cubes, "std", [], 0, 2)
    raises("moments_time_groups: n_groups 0 outside 1 .. 65535", h, cubes, "std", [], 0)
    raises("moments_time_groups: n_groups 65536 outside 1 .. 65535", h, cubes, "std", [a], 65536, 1)
    raises("moments_time_groups: 1 label arrays for 2 cubes", h, cubes, "std", [a], 3)
    raises("moments_time_groups: labels 1 are int64, not uint16", h, cubes, "std", [a, np.zeros(9, dtype=np.int64)], 3)
    raises("moments_time_groups: labels 0 are int16, not uint16", h, cubes, "std", [a.astype(np.int16), a[:1]], 3)
    raises("moments_time_groups: labels 1 have shape (4,), their cube 3 instants", h, cubes, "std", [a, np.zeros(4, dtype=np.uint16)], 3)
    raises("moments_time_groups: labels 0 have shape (0,), their cube 3 instants", h, cubes, "std", [a[:0], a[:2]], 3, 1)


# ---- EncodedRaster: nothing to read ------------------------------------------------------------------------------------------------
def _filled(d, names, shape, zero):
    assert list(d) == names
    for n, v in d.items():
        assert v.shape == shape and v.dtype == np.float64, (n, v.shape, v.dtype)
        if n in zero:
            assert (v == 0).all() and not np.signbit(v).any(), n
        else:
            assert np.isnan(v).all(), n


def test_nothing_to_read(raster):
    R = raster
    for kw in (dict(start=3, stop=3), dict(start=10), dict(window=(5, 5, 0, 60)), dict(window=(0, 50, 60, 60))):
        rows, cols = (kw["window"][1] - kw["window"][0], kw["window"][3] - kw["window"][2]) if "window" in kw else (50, 60)
        lab = LAB if "window" in kw else LAB[:0]
        _filled(R.reduce_time_groups(31, lab, n_groups=3, **kw), REDUCE.split(", "), (3, rows, cols), ("sum", "count"))
        _filled(R.reduce_time_groups(("mean", "sum"), lab, **kw), ["sum", "mean"], (1, rows, cols), ("sum",))
        _filled(R.moments_time(15, **kw), MOMENT.split(", "), (rows, cols), ("count",))
        _filled(R.moments_time(**kw), ["mean", "std"], (rows, cols), ())
        _filled(R.moments_time_groups(15, lab, n_groups=65535 if rows * cols == 0 else 2, ddof=1, **kw), MOMENT.split(", "),
                (65535 if rows * cols == 0 else 2, rows, cols), ("count",))
        _filled(R.moments_time_groups(("var", "count"), lab, **kw), ["count", "var"], (1, rows, cols), ("count",))
    # n_groups defaults to the largest label present, GROUP_NONE apart, plus 1; at least 1
    lab = LAB.copy()
    lab[4], lab[0] = 6, NONE
    assert R.reduce_time_groups("min", lab, window=(5, 5, 0, 60))["min"].shape == (7, 0, 60)
    assert R.moments_time_groups("var", lab, window=(5, 5, 0, 60))["var"].shape == (7, 0, 60)
    allnone = np.full(10, NONE, dtype=np.uint16)
    assert R.reduce_time_groups("min", allnone, window=(0, 50, 7, 7))["min"].shape == (1, 50, 0)
    assert R.moments_time_groups("var", allnone, window=(0, 50, 7, 7))["var"].shape == (1, 50, 0)


# ---- Variable ----------------------------------------------------------------------------------------------------------------------
class FakeVar:
    """Variable's three methods over a shape alone: its raster is one no call here may take to the library."""
    reduce_time_groups = D.Variable.reduce_time_groups
    moments_time_groups = D.Variable.moments_time_groups
    zonal = D.Variable.zonal
    _region = D.Variable._region
    _check = D.Variable._check

    def __init__(self, shape):
        self.shape = shape

    def raster(self):
        return EncodedRaster(self.shape, [None] * (-(-self.shape[0] // 32)), tile=1 << 20, chunk_size=32)


def _outside(msg, f, *a, **k):
    with pytest.raises(IndexError, match="^" + re.escape(msg) + "$"):
        f(*a, **k)


def test_variable_checks_in_order():
    v = FakeVar((10, 50, 60))
    bad = np.zeros(2)
    for f in (lambda **k: v.reduce_time_groups(bad, "median", **k), lambda **k: v.moments_time_groups(bad, "median", ddof=2, **k),
              lambda **k: v.zonal(bad, "median", **k)):  # the bounds come before every other check
        _outside("window (0:11, 0:50, 0:60) outside the variable's shape (10, 50, 60)", f, stop=11)
        _outside("window (5:4, 0:50, 0:60) outside the variable's shape (10, 50, 60)", f, start=5, stop=4)
        _outside("window (0:10, 0:51, 0:60) outside the variable's shape (10, 50, 60)", f, bottom=51)
        _outside("window (0:10, 0:50, 3:2) outside the variable's shape (10, 50, 60)", f, left=3, right=2)
    ids10 = np.arange(10)
    f = v.reduce_time_groups
    raises("reduce_time: unknown statistic 'median' (one of %s)" % REDUCE, f, bad, "median")
    raises("reduce_time_groups: the labels are float64 (2,), the instants integers (10,)", f, bad)
    raises("reduce_time_groups: the labels are float64 (10,), the instants integers (10,)", f, ids10.astype(np.float64))
    raises("reduce_time_groups: the labels are int64 (10,), the instants integers (4,)", f, ids10, start=3, stop=7)
    raises("reduce_time_groups: the labels are bool (10,), the instants integers (10,)", f, ids10 > 4)
    f = v.moments_time_groups
    raises("moments_time: unknown statistic 'median' (one of %s)" % MOMENT, f, bad, "median", ddof=2)
    raises("moments_time: ops 16 is not a set of %s" % MOMENT, f, bad, 16, ddof=2)
    raises("moments_time: ddof 2 is neither 0 nor 1", f, bad, ddof=2)
    raises("moments_time_groups: the labels are float64 (2,), the instants integers (10,)", f, bad)
    raises("moments_time_groups: the labels are uint8 (10,), the instants integers (4,)", f, ids10.astype(np.uint8), start=3, stop=7, ddof=1)
    f = v.zonal
    raises("reduce_time: unknown statistic 'median' (one of %s)" % REDUCE, f, np.zeros((2, 2)), "median")
    raises("zonal: the labels are float64 (2, 2), the window integers (50, 60)", f, np.zeros((2, 2)))
    raises("zonal: the labels are int64 (50, 60), the window integers (10, 2)", f, np.zeros((50, 60), dtype=np.int64), top=40, left=1, right=3)
    # more distinct ids than dense labels: the shape is right, and there are no instants to read either
    big = FakeVar((65536, 1, 1))
    raises("reduce_time_groups: 65536 distinct group ids, at most 65535", big.reduce_time_groups, np.arange(65536))
    raises("moments_time_groups: 65536 distinct group ids, at most 65535", big.moments_time_groups, np.arange(65536) * 3, ddof=1)
    raises("reduce_time_groups: the labels are int64 (65536,), the instants integers (0,)", big.reduce_time_groups, np.arange(65536), start=9, stop=9)
    wide = FakeVar((4, 256, 257))
    raises("zonal: 65792 distinct zone ids, at most 65535", wide.zonal, np.arange(256 * 257).reshape(256, 257))
    raises("zonal: 65792 distinct zone ids, at most 65535", wide.zonal, np.arange(256 * 257).reshape(256, 257), start=2, stop=2)
    ids, got = big.reduce_time_groups(np.arange(65536) - 1, "count", top=1)  # 65535 ids are fine; no cells: the raster's own fill
    assert ids.size == 65535 and got["count"].shape == (65535, 0, 1) and got["count"].dtype == np.float64


def test_variable_empty_results():
    v = FakeVar((10, 50, 60))
    ids_in = np.array([12, -1, 3, 12, 700000, 3, -5, 12, 3, 3])
    for kw, lab, n_ids, shape in ((dict(start=4, stop=4), ids_in[:0], 0, (50, 60)), (dict(), np.full(10, -1), 0, (50, 60)),
                                  (dict(top=7, bottom=7), ids_in, 3, (0, 60)), (dict(left=60), ids_in.astype(np.int16), 2, (50, 0)),
                                  (dict(start=10, top=2, bottom=5, right=1), ids_in[:0].astype(np.uint8), 0, (3, 1))):
        ids, d = v.reduce_time_groups(lab, 31, **kw)
        assert ids.tolist() == sorted(set(x for x in lab.tolist() if x >= 0)) and ids.size == n_ids
        _filled(d, REDUCE.split(", "), (n_ids,) + shape, ("sum", "count"))
        assert list(v.reduce_time_groups(lab, **kw)[1]) == ["mean"]
        ids, d = v.moments_time_groups(lab, 15, ddof=1, **kw)
        assert ids.size == n_ids
        _filled(d, MOMENT.split(", "), (n_ids,) + shape, ("count",))
        assert list(v.moments_time_groups(lab, **kw)[1]) == ["mean", "std"]
    zl = np.zeros((50, 60), dtype=np.int64)
    zl[5, 1], zl[6, 2], zl[0, 0] = 40, 7, -2
    ids, z = v.zonal(zl, ("min", "count"), start=3, stop=3)  # no instants: empty matrices, a row per id
    assert ids.tolist() == [0, 7, 40] and list(z) == ["min", "count"] and all(x.shape == (3, 0) and x.dtype == np.float64 for x in z.values())
    ids, z = v.zonal(np.full((50, 60), -1))  # no zone: no row, a column per instant
    assert ids.size == 0 and list(z) == ["mean"] and z["mean"].shape == (0, 10) and z["mean"].dtype == np.float64
    ids, z = v.zonal(np.full((50, 60), -1), 31, start=2, stop=7)
    assert ids.size == 0 and list(z) == REDUCE.split(", ") and all(x.shape == (0, 5) and x.dtype == np.float64 for x in z.values())
    ids, z = v.zonal(np.full((3, 0), 4, dtype=np.int8), "sum", start=6, stop=6, top=1, bottom=4, left=9, right=9)
    assert ids.size == 0 and z["sum"].shape == (0, 0)
