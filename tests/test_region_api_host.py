"""What the Python layer of the region calls (EncodedRaster.reduce_time / spells / reduce_space / zonal / histogram, their *_flat
forms and Variable's methods of the same names) checks before the library is called, without a GPU: every message, the order of
the checks, and what comes back -- dtype, shape, fill value -- when there is nothing to read."""
import re

import numpy as np
import pytest

from dcdf_amd import _lib
from dcdf_amd import dataset as D
from dcdf_amd.raster import EncodedRaster

LAB = np.zeros((50, 60), dtype=np.uint16)
NAN = float("nan")


@pytest.fixture()
def raster():
    """10 instants of 50 x 60 cells; no test here reaches the library."""
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    yield R
    R._native = None


def raises(msg, f, *a, **k):
    with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
        f(*a, **k)


# the five whole-raster methods, each with arguments that are wrong in every later check too: the first check must be the one
# that speaks
def _calls(R):
    return {
        "reduce_time": lambda **k: R.reduce_time("median", **k),
        "spells": lambda **k: R.spells(NAN, 1.0, "median", **k),
        "reduce_space": lambda **k: R.reduce_space("median", mask=np.ones((2, 2)), **k),
        "zonal": lambda **k: R.zonal("median", np.zeros((2, 2)), n_zones=0, **k),
        "histogram": lambda **k: R.histogram([3.0, 1.0], mask=np.ones((2, 2)), **k),
    }


@pytest.mark.parametrize("name", ["reduce_time", "spells", "reduce_space", "zonal", "histogram"])
def test_instants_then_window_come_first(raster, name):
    f = _calls(raster)[name]
    bad_window = (0, 51, 0, 60)
    raises("instants [5, 4) outside [0, 10)", f, start=5, stop=4, window=bad_window)
    raises("instants [0, 11) outside [0, 10)", f, stop=11, window=bad_window)
    raises("instants [-1, 3) outside [0, 10)", f, start=-1, stop=3)
    raises("window (0:51, 0:60) outside the raster's 50 x 60 cells", f, window=bad_window)
    raises("window (4:3, 0:60) outside the raster's 50 x 60 cells", f, start=3, stop=3, window=(4, 3, 0, 60))
    raises("window (0:50, -1:60) outside the raster's 50 x 60 cells", f, window=(0, 50, -1, 60))
    raises("window (0:50, 7:6) outside the raster's 50 x 60 cells", f, window=np.array([0, 50, 7, 6]))


def test_own_checks_in_order(raster):
    R = raster
    # reduce_time: the statistics
    raises("reduce_time: unknown statistic 'median' (one of min, max, sum, count, mean)", R.reduce_time, "median")
    # spells: the statistics, then the bounds
    raises("spells: unknown statistic 'median' (one of count, longest, longest_start, first, last)", R.spells, NAN, 1.0, "median")
    raises("spells: a NaN bound", R.spells, NAN, 1.0)
    raises("spells: a NaN bound", R.spells, 0.0, NAN, start=4, stop=4)
    # reduce_space: the statistics (reduce_ops' own prefix), then the mask
    raises("reduce_time: unknown statistic 'median' (one of min, max, sum, count, mean)", R.reduce_space, "median", mask=np.ones((2, 2)))
    raises("reduce_space: the mask has shape (2, 2), the window (50, 60)", R.reduce_space, "sum", mask=np.ones((2, 2)))
    raises("reduce_space: the mask has shape (50, 60), the window (7, 40)", R.reduce_space, "sum", 3, 3, (3, 10, 20, 60), np.ones((50, 60)))
    # zonal: the statistics, the labels, n_zones
    raises("reduce_time: unknown statistic 'median' (one of min, max, sum, count, mean)", R.zonal, "median", np.zeros((2, 2)), n_zones=0)
    raises("zonal: the labels are float64 (2, 2), the window uint16 (50, 60)", R.zonal, "sum", np.zeros((2, 2)), n_zones=0)
    raises("zonal: the labels are uint16 (50, 60), the window uint16 (7, 40)", R.zonal, "sum", LAB, window=(3, 10, 20, 60), n_zones=0)
    raises("zonal: the labels are int32 (50, 60), the window uint16 (50, 60)", R.zonal, "sum", LAB.astype(np.int32))
    raises("zonal: n_zones 0 outside 1 .. 65535", R.zonal, "sum", LAB, n_zones=0)
    raises("zonal: n_zones 65536 outside 1 .. 65535", R.zonal, "sum", LAB, 2, 2, n_zones=65536)
    # histogram: the edges, then the mask
    raises("histogram: edges must be strictly increasing, without NaN", R.histogram, [3.0, 1.0], mask=np.ones((2, 2)))
    raises("histogram: edges must be 2 .. 257 increasing values", R.histogram, [3.0], mask=np.ones((2, 2)))
    raises("histogram: edges must be 2 .. 257 increasing values", R.histogram, np.arange(258.0))
    raises("histogram: edges must be 2 .. 257 increasing values", R.histogram, np.zeros((2, 2)))
    raises("histogram: edges must be strictly increasing, without NaN", R.histogram, [0.0, NAN, 2.0])
    raises("histogram: the mask has shape (2, 2), the window (50, 60)", R.histogram, [0.0, 1.0], mask=np.ones((2, 2)))


def test_ops_tables():
    for f, what, names in ((EncodedRaster.reduce_ops, "reduce_time", ["min", "max", "sum", "count", "mean"]),
                           (EncodedRaster.spell_ops, "spells", ["count", "longest", "longest_start", "first", "last"])):
        assert f(31) == (31, names) and f(np.uint32(5)) == (5, [names[0], names[2]]) and f(names[3]) == (8, [names[3]])
        assert f([names[4], names[0], names[4]]) == (17, [names[0], names[4]])  # plane order = bit order
        assert f(n for n in names[1:3]) == (6, names[1:3])
        joined = ", ".join(names)
        raises("%s: unknown statistic 'avg' (one of %s)" % (what, joined), f, "avg")
        raises("%s: unknown statistic 3 (one of %s)" % (what, joined), f, [names[0], 3])
        for bad in (0, 32, -1, [], ()):
            raises("%s: ops %r is not a set of %s" % (what, bad, joined), f, bad)
        with pytest.raises(TypeError):
            f(1.5)  # (neither a bitmask nor an iterable)


def test_nothing_to_read(raster):
    R = raster
    for kw in (dict(start=3, stop=3), dict(start=10), dict(window=(5, 5, 0, 60)), dict(window=(0, 50, 60, 60))):
        rows, cols = (kw["window"][1] - kw["window"][0], kw["window"][3] - kw["window"][2]) if "window" in kw else (50, 60)
        d = R.reduce_time(31, **kw)
        assert list(d) == ["min", "max", "sum", "count", "mean"]
        assert all(v.shape == (rows, cols) and v.dtype == np.float64 for v in d.values())
        assert all(np.isnan(d[n]).all() for n in ("min", "max", "mean")) and all((d[n] == 0).all() for n in ("sum", "count"))
        s = R.spells(0.0, 1.0, 31, **kw)
        assert list(s) == ["count", "longest", "longest_start", "first", "last"]
        assert all(v.shape == (rows, cols) and v.dtype == np.uint32 for v in s.values())
        assert all((s[n] == 0).all() for n in ("count", "longest")) and all((s[n] == _lib.SPELL_NONE).all() for n in ("longest_start", "first", "last"))
    assert list(R.spells(0.0, 1.0, start=1, stop=1)) == ["count", "longest"]  # (the default statistics)
    # the per-instant calls: no instants, whatever the window
    for kw in (dict(start=3, stop=3), dict(start=10), dict(start=0, stop=0, window=(5, 5, 0, 60))):
        m = None if "window" in kw else np.ones((50, 60), dtype=bool)
        d = R.reduce_space(("mean", "min"), mask=m, **kw)
        assert list(d) == ["min", "mean"] and all(v.shape == (0,) and v.dtype == np.float64 for v in d.values())
        h = R.histogram([0.0, 1.0, 2.0, np.inf], mask=m, **kw)
        assert h.shape == (0, 3) and h.dtype == np.uint64
        lab = np.full((0, 60) if "window" in kw else (50, 60), 6, dtype=np.uint16)
        z = R.zonal(("sum", "count"), lab, **kw)
        assert list(z) == ["sum", "count"] and all(v.shape == (1 if "window" in kw else 7, 0) and v.dtype == np.float64 for v in z.values())
        assert all(v.shape == (4, 0) for v in R.zonal(8, lab, n_zones=4, **kw).values())
    # n_zones defaults to the largest label below ZONE_NONE, plus 1; at least 1
    lab = LAB.copy()
    assert R.zonal("min", lab, 2, 2)["min"].shape == (1, 0)
    lab[3, 4], lab[0, 0] = 11, _lib.ZONE_NONE
    assert R.zonal("min", lab, 2, 2)["min"].shape == (12, 0)
    assert R.zonal("min", np.full((50, 60), _lib.ZONE_NONE, dtype=np.uint16), 2, 2)["min"].shape == (1, 0)


def test_flat_forms_check_before_the_call(raster):
    R = raster
    cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10]]
    raises("reduce_time: ops 0 is not a set of min, max, sum, count, mean", R.reduce_time_flat, cubes, 0)
    raises("spells: ops 32 is not a set of count, longest, longest_start, first, last", R.spells_flat, cubes, NAN, 1.0, 32)
    raises("spells: a NaN bound", R.spells_flat, cubes, [0.0, NAN], 1.0, "count")
    raises("spells: a NaN bound", R.spells_flat, cubes, 0.0, [1.0, NAN], "count")
    with pytest.raises(ValueError):  # (numpy's own: three bounds for two cubes)
        R.spells_flat(cubes, [0.0, 1.0, 2.0], 1.0, "count")
    raises("reduce_time: ops 0 is not a set of min, max, sum, count, mean", R.reduce_space_flat, cubes, 0, [None])
    raises("reduce_space: 1 masks for 2 cubes", R.reduce_space_flat, cubes, "sum", [None])
    raises("reduce_time: ops 0 is not a set of min, max, sum, count, mean", R.zonal_flat, cubes, 0, [], 0)
    raises("zonal: n_zones 0 outside 1 .. 65535", R.zonal_flat, cubes, "sum", [], 0)
    raises("zonal: n_zones 65536 outside 1 .. 65535", R.zonal_flat, cubes, "sum", [], 65536)
    raises("zonal: 0 label arrays for 2 cubes", R.zonal_flat, cubes, "sum", [], 3)
    raises("histogram: edges must be 2 .. 257 increasing values", R.histogram_flat, cubes, [1.0], [None])
    raises("histogram: 1 masks for 2 cubes", R.histogram_flat, cubes, [1.0, 2.0], [None])


def test_mask_arguments():
    q = np.array([[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 1, 3, 1, 4]], dtype=np.uint32)  # 5 x 7, reversed 7 x 20, 2 x 3
    f = EncodedRaster._mask_args
    assert f(q, None, "w") == (None, None, _lib.MEM_HOST, None)
    assert f(q, [None, None, None], "w") == (None, None, _lib.MEM_HOST, None)  # (no mask at all: nothing is staged)
    raises("w: 2 masks for 3 cubes", f, q, [None, None], "w")
    raises("w: mask 1 has shape (20, 7), its cube (7, 20)", f, q, [None, np.ones((20, 7)), np.ones((9, 9))], "w")
    raises("w: mask 0 has shape (35,), its cube (5, 7)", f, q, [np.ones(35), None, None], "w")
    m1 = np.zeros((7, 20))
    m1[2, 5], m1[6, 19] = -3.5, 2
    ptr, off, mem, keep = f(q, [None, m1, np.ones((2, 3), dtype=bool)], "w")
    flat, moff = keep
    assert mem == _lib.MEM_HOST and (ptr.value, off.value) == (flat.ctypes.data, moff.ctypes.data)
    assert flat.dtype == np.uint8 and flat.flags.c_contiguous and moff.dtype == np.uint64 and moff.tolist() == [0, 35, 175]
    want = np.concatenate([np.ones(35), (m1 != 0).ravel(), np.ones(6), [0]])  # all cells for None; one spare element at the end
    np.testing.assert_array_equal(flat, want)
    # masks already on the device: the pointer and the caller's offsets, kept alive as uint64
    ptr, off, mem, keep = f(q, (4096, [5, 1000, 7]), "w")
    assert (ptr.value, mem) == (4096, _lib.MEM_DEVICE) and keep.dtype == np.uint64 and keep.tolist() == [5, 1000, 7] and off.value == keep.ctypes.data
    ptr, off, mem, keep = f(q, (np.int64(8192), np.array([0, 1, 2], dtype=np.uint64)), "w")
    assert (ptr.value, mem) == (8192, _lib.MEM_DEVICE)
    raises("w: 2 mask offsets for 3 cubes", f, q, (4096, [5, 1000]), "w")
    raises("w: 6 mask offsets for 3 cubes", f, q, (4096, np.zeros((3, 2))), "w")


def test_label_arguments():
    q = np.array([[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10]], dtype=np.uint32)  # 5 x 7, reversed 7 x 20
    f = EncodedRaster._label_args
    a = np.arange(35, dtype=np.uint16).reshape(5, 7)
    b = np.full((7, 20), _lib.ZONE_NONE, dtype=np.uint16)
    raises("w: 1 label arrays for 2 cubes", f, q, [a], "w")
    raises("w: labels 1 are int64, not uint16", f, q, [a, np.zeros((9, 9), dtype=np.int64)], "w")  # (the dtype before the shape)
    raises("w: labels 1 have shape (20, 7), their cube (7, 20)", f, q, [a, b.T], "w")
    raises("w: labels 0 are uint8, not uint16", f, q, [a.astype(np.uint8), b.T], "w")
    ptr, off, mem, keep, top = f(q, [a, b], "w")
    flat, loff = keep
    assert mem == _lib.MEM_HOST and (ptr.value, off.value) == (flat.ctypes.data, loff.ctypes.data) and top == 34
    assert flat.dtype == np.uint16 and flat.flags.c_contiguous and loff.dtype == np.uint64 and loff.tolist() == [0, 35]
    np.testing.assert_array_equal(flat, np.concatenate([a.ravel(), b.ravel(), [0]]))  # one spare element at the end
    assert f(q[1:], [b], "w")[4] == -1 and f(q[:0], [], "w")[4] == -1  # no label below ZONE_NONE; no cube
    ptr, off, mem, keep, top = f(q, (4096, [5, 1000]), "w")
    assert (ptr.value, mem, top) == (4096, _lib.MEM_DEVICE, -1) and keep.dtype == np.uint64 and keep.tolist() == [5, 1000] and off.value == keep.ctypes.data
    raises("w: 1 label offsets for 2 cubes", f, q, (4096, [5]), "w")
    with pytest.raises(TypeError):
        f(q, None, "w")  # (labels are mandatory)


# ---- Variable: the defaults of stop / bottom / right, the bounds (IndexError), then the call's own checks ------------------------
@pytest.fixture(scope="module")
def variable():
    """A variable of 360 x 4 cells without a stored instant: every call on it ends before a chunk is opened."""
    t = D.Coordinate.time("t", np.datetime64("1979-01-01"), np.timedelta64(1, "D"))
    ds = D.Dataset.new([t, D.Coordinate.range("y", -89.75, 0.5, 360, np.float32), D.Coordinate.range("x", 0, 1, 4, np.int32)], [360, 4], D.Resolver())
    return ds.add_variable("v", 10, 20, [4, 5], True, 3, np.float64).v


def _outside(msg, f, *a, **k):
    with pytest.raises(IndexError, match="^" + re.escape(msg) + "$"):
        f(*a, **k)


def test_variable_defaults_bounds_and_empty_results(variable):
    v = variable
    assert v.shape == (0, 360, 4)
    lab = np.zeros((360, 4), dtype=np.int64)
    calls = {
        "decode": lambda **k: v.decode(**k),
        "reduce_time": lambda **k: v.reduce_time("median", **k),
        "spells": lambda **k: v.spells(NAN, 1.0, "median", **k),
        "reduce_space": lambda **k: v.reduce_space("median", **k),
        "zonal": lambda **k: v.zonal(np.zeros((2, 2)), "median", **k),
        "histogram": lambda **k: v.histogram([3.0, 1.0], **k),
    }
    for name, f in calls.items():  # the bounds come before every other check
        _outside("window (0:1, 0:360, 0:4) outside the variable's shape (0, 360, 4)", f, stop=1)
        _outside("window (1:0, 0:360, 0:4) outside the variable's shape (0, 360, 4)", f, start=1)
        if name != "decode":
            _outside("window (0:0, 0:361, 0:4) outside the variable's shape (0, 360, 4)", f, bottom=361)
            _outside("window (0:0, 0:360, 3:2) outside the variable's shape (0, 360, 4)", f, left=3, right=2)
            _outside("window (0:0, -1:360, 0:4) outside the variable's shape (0, 360, 4)", f, top=-1)
    raises("reduce_time: unknown statistic 'median' (one of min, max, sum, count, mean)", calls["reduce_time"])
    raises("spells: a NaN bound", v.spells, NAN, 1.0)
    raises("spells: unknown statistic 'median' (one of count, longest, longest_start, first, last)", v.spells, 0.0, 1.0, "median")
    raises("reduce_time: unknown statistic 'median' (one of min, max, sum, count, mean)", calls["reduce_space"])
    raises("reduce_time: unknown statistic 'median' (one of min, max, sum, count, mean)", calls["zonal"])
    raises("zonal: the labels are float64 (2, 2), the window integers (360, 4)", v.zonal, np.zeros((2, 2)))
    raises("zonal: the labels are int64 (360, 4), the window integers (10, 2)", v.zonal, lab, top=350, left=1, right=3)
    raises("histogram: edges must be strictly increasing, without NaN", calls["histogram"])
    raises("histogram: the mask has shape (2, 2), the window (360, 4)", v.histogram, [0.0, 1.0], mask=np.ones((2, 2)))
    # nothing stored: what comes back
    d = v.decode()
    assert d.shape == (0, 360, 4) and d.dtype == np.float64
    d = v.reduce_time(31, top=350, left=1, right=3)
    assert list(d) == ["min", "max", "sum", "count", "mean"] and all(x.shape == (10, 2) and x.dtype == np.float64 for x in d.values())
    assert all(np.isnan(d[n]).all() for n in ("min", "max", "mean")) and all((d[n] == 0).all() for n in ("sum", "count"))
    assert list(v.reduce_time()) == ["mean"] and v.reduce_time()["mean"].shape == (360, 4)
    s = v.spells(0.0, 1.0, 31, top=350, left=1, right=3)
    assert all(x.shape == (10, 2) and x.dtype == np.uint32 for x in s.values())
    assert all((s[n] == 0).all() for n in ("count", "longest")) and all((s[n] == _lib.SPELL_NONE).all() for n in ("longest_start", "first", "last"))
    assert list(v.spells(0.0, 1.0)) == ["count", "longest"]
    d = v.reduce_space(("max", "mean"), mask=np.ones((9, 9)))  # (without instants the mask is not looked at)
    assert list(d) == ["max", "mean"] and all(x.shape == (0,) and x.dtype == np.float64 for x in d.values())
    lab[5, 1], lab[6, 2], lab[0, 0] = 40, 7, -2
    ids, z = v.zonal(lab, ("min", "count"))
    assert ids.tolist() == [0, 7, 40] and list(z) == ["min", "count"] and all(x.shape == (3, 0) and x.dtype == np.float64 for x in z.values())
    ids, z = v.zonal(np.full((360, 4), -1))
    assert ids.size == 0 and z["mean"].shape == (0, 0)
    h = v.histogram([0.0, 1.0, 5.0])
    assert h.shape == (0, 2) and h.dtype == np.uint64
