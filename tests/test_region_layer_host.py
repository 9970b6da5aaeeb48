"""What the other host modules of the region statistics' Python layer leave open, without a GPU and without a library call:
quantile_time's checks and empty results in both layers, Variable's grouped folds and moments on a variable without instants, what
every *_flat method hands to _region_call -- literally --, EncodedRaster.decode, and the unevenness the layer keeps on purpose."""
import ctypes as C
import re

import numpy as np
import pytest

from dcdf_amd import _lib
from dcdf_amd import dataset as D
from dcdf_amd.raster import EncodedRaster

NAN = float("nan")
REDUCE = "min, max, sum, count, mean"
MOMENT = "count, mean, var, std"
HOST, DEVICE = _lib.MEM_HOST, _lib.MEM_DEVICE


def raises(msg, f, *a, **k):
    with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
        f(*a, **k)


def outside(msg, f, *a, **k):
    with pytest.raises(IndexError, match="^" + re.escape(msg) + "$"):
        f(*a, **k)


def peek(ptr, dtype, n):
    """n elements of dtype behind a c_void_p, as a list"""
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr.value), dtype=dtype).tolist()


class Recorder(EncodedRaster):
    """An EncodedRaster whose _region_call notes what it is handed and answers 0, 1, 2, ... in the real one's return forms.
    peek = {position in the C tuple: (dtype, elements)}: pointers to read while the call's arrays are alive."""

    def __init__(self, shape=(10, 50, 60)):
        super().__init__(shape, [None], tile=256, chunk_size=32)
        self.seen, self.peek = [], {}

    def _region_call(self, name, q, counts, dtype, args, zeroed=False, stats=True, out_device_ptr=None, out_offset=None):
        own = list(args("n", "out", "mem", "off", "stats"))
        for i, a in enumerate(own):
            if i in self.peek:
                own[i] = peek(a, *self.peek[i])
            elif isinstance(a, C.c_void_p):
                own[i] = "pointer"
            elif isinstance(a, (C.c_uint32, C.c_int32)):
                own[i] = (type(a).__name__, a.value)
        vol = counts()
        self.seen.append(dict(name=name, q=q.tolist(), q_dtype=q.dtype, dtype=np.dtype(dtype), zeroed=zeroed, stats=stats, counts=vol.tolist(), args=own,
                              ptr=out_device_ptr, offset=None if out_offset is None else list(out_offset)))
        tail = (0.5, np.zeros(3, dtype=np.uint64)) if stats else (0.5,)
        if out_device_ptr is not None:
            return tail
        off = np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64)
        return (np.arange(max(1, int(vol.sum()))).astype(dtype), off) + tail


@pytest.fixture()
def raster():
    """10 instants of 50 x 60 cells; no test here reaches the library."""
    return Recorder()


@pytest.fixture(scope="module")
def variable():
    """A variable of 360 x 4 cells without a stored instant (test_region_api_host.py's): every call ends before a chunk is opened."""
    t = D.Coordinate.time("t", np.datetime64("1979-01-01"), np.timedelta64(1, "D"))
    ds = D.Dataset.new([t, D.Coordinate.range("y", -89.75, 0.5, 360, np.float32), D.Coordinate.range("x", 0, 1, 4, np.int32)], [360, 4], D.Resolver())
    return ds.add_variable("v", 10, 20, [4, 5], True, 3, np.float64).v


# ---- quantile_time ---------------------------------------------------------------------------------------------------------------------
def _probs_messages(f):
    """f(probs, method): every message of the probabilities and the method, the probabilities first"""
    raises("quantile_time: 0 probabilities, not 1 .. 16", f, [], "median")
    raises("quantile_time: 17 probabilities, not 1 .. 16", f, np.linspace(0, 1, 17), "median")
    raises("quantile_time: probabilities must lie in [0, 1]", f, [0.5, 1.5], "median")
    raises("quantile_time: probabilities must lie in [0, 1]", f, -0.1, 9)
    raises("quantile_time: probabilities must lie in [0, 1]", f, [0.5, NAN], "linear")
    raises("quantile_time: unknown method 'median' (one of lower, higher, nearest, linear)", f, 0.5, "median")
    raises("quantile_time: unknown method 4", f, [0.5], 4)
    raises("quantile_time: unknown method -1", f, [[0.1, 0.2], [0.3, 0.4]], -1)


def test_quantile_time_checks_in_order(raster, variable):
    R, v = raster, variable
    bad_window = (0, 51, 0, 60)
    raises("instants [5, 4) outside [0, 10)", R.quantile_time, [], 5, 4, bad_window, "median")
    raises("instants [0, 11) outside [0, 10)", R.quantile_time, [], stop=11, window=bad_window, method="median")
    raises("window (0:51, 0:60) outside the raster's 50 x 60 cells", R.quantile_time, [], window=bad_window, method="median")
    raises("window (0:50, 7:6) outside the raster's 50 x 60 cells", R.quantile_time, [], 3, 3, (0, 50, 7, 6), "median")
    _probs_messages(lambda p, m: R.quantile_time(p, method=m))
    _probs_messages(lambda p, m: R.quantile_time(p, 3, 3, method=m))
    _probs_messages(lambda p, m: R.quantile_time(p, window=(5, 5, 0, 60), method=m))
    _probs_messages(lambda p, m: R.quantile_time_flat([[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10]], p, m))
    assert R.seen == []
    # Variable without a stored instant: the bounds (IndexError), then the own checks
    assert v.shape == (0, 360, 4)
    f = lambda **k: v.quantile_time([], method="median", **k)  # noqa: E731
    outside("window (0:1, 0:360, 0:4) outside the variable's shape (0, 360, 4)", f, stop=1)
    outside("window (1:0, 0:360, 0:4) outside the variable's shape (0, 360, 4)", f, start=1)
    outside("window (0:0, 0:361, 0:4) outside the variable's shape (0, 360, 4)", f, bottom=361)
    outside("window (0:0, 0:360, 3:2) outside the variable's shape (0, 360, 4)", f, left=3, right=2)
    _probs_messages(lambda p, m: v.quantile_time(p, method=m))


def _all_nan(a, shape):
    assert a.shape == shape and a.dtype == np.float64 and np.isnan(a).all()


def test_quantile_time_results(raster, variable):
    R, v = raster, variable
    # nothing to read -- no instants, or no cells --: NaN, the leading axis squeezed for a scalar `probs` only
    for kw, (rows, cols) in ((dict(start=3, stop=3), (50, 60)), (dict(start=10), (50, 60)), (dict(window=(5, 5, 0, 60)), (0, 60)),
                             (dict(window=(0, 50, 60, 60)), (50, 0)), (dict(start=2, stop=2, window=(1, 4, 2, 9)), (3, 7))):
        _all_nan(R.quantile_time(0.5, **kw), (rows, cols))
        _all_nan(R.quantile_time(np.float64(0.5), method=0, **kw), (rows, cols))
        _all_nan(R.quantile_time([0.5], method="lower", **kw), (1, rows, cols))
        _all_nan(R.quantile_time([[0.1, 0.9], [0.2, 0.8]], method=2, **kw), (4, rows, cols))
    assert R.seen == []
    _all_nan(v.quantile_time(0.5), (360, 4))
    _all_nan(v.quantile_time([0.5], top=350, left=1, right=3, method=1), (1, 10, 2))
    _all_nan(v.quantile_time(np.linspace(0, 1, 16), bottom=0, method="nearest"), (16, 0, 4))
    # one cube: the method by name or by code, the planes cut from the flat result
    got = R.quantile_time(0.5, 2, 7, (1, 3, 4, 7), "higher")
    assert got.shape == (2, 3) and got.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert R.seen[-1]["q"] == [[2, 7, 1, 3, 4, 7]] and R.seen[-1]["args"][3] == ("c_int", 1) and R.seen[-1]["counts"] == [6]
    got = R.quantile_time([0.5], 2, 7, (1, 3, 4, 7), 1)
    assert got.shape == (1, 2, 3) and got[0].tolist() == [[0, 1, 2], [3, 4, 5]] and R.seen[-1]["args"][3] == ("c_int", 1)
    got = R.quantile_time([0.1, 0.9], window=(1, 3, 4, 7))
    assert got.shape == (2, 2, 3) and got[1].tolist() == [[6, 7, 8], [9, 10, 11]] and R.seen[-1]["args"][2:4] == [("c_uint", 2), ("c_int", 3)]


# ---- Variable's grouped folds and moments on the variable without instants ---------------------------------------------------------------
def test_variable_without_instants_checks_in_order(variable):
    v = variable
    bad, none = np.zeros(2), np.zeros(0, dtype=np.int64)
    calls = (lambda **k: v.reduce_time_groups(bad, "median", **k), lambda **k: v.moments_time("median", ddof=2, **k),
             lambda **k: v.moments_time_groups(bad, "median", ddof=2, **k))
    for f in calls:  # the bounds come before every other check
        outside("window (0:1, 0:360, 0:4) outside the variable's shape (0, 360, 4)", f, stop=1)
        outside("window (1:0, 0:360, 0:4) outside the variable's shape (0, 360, 4)", f, start=1)
        outside("window (0:0, 0:361, 0:4) outside the variable's shape (0, 360, 4)", f, bottom=361)
        outside("window (0:0, 0:360, 3:2) outside the variable's shape (0, 360, 4)", f, left=3, right=2)
        outside("window (0:0, -1:360, 0:4) outside the variable's shape (0, 360, 4)", f, top=-1)
    # the statistics, ddof, the labels
    raises("reduce_time: unknown statistic 'median' (one of %s)" % REDUCE, v.reduce_time_groups, bad, "median")
    raises("reduce_time: ops 0 is not a set of %s" % REDUCE, v.reduce_time_groups, bad, 0)
    raises("reduce_time_groups: the labels are float64 (2,), the instants integers (0,)", v.reduce_time_groups, bad)
    raises("reduce_time_groups: the labels are int64 (1,), the instants integers (0,)", v.reduce_time_groups, np.zeros(1, dtype=np.int64), "sum")
    raises("reduce_time_groups: the labels are float32 (0,), the instants integers (0,)", v.reduce_time_groups, none.astype(np.float32))
    raises("reduce_time_groups: the labels are int64 (0, 1), the instants integers (0,)", v.reduce_time_groups, none.reshape(0, 1))
    raises("moments_time: unknown statistic 'median' (one of %s)" % MOMENT, v.moments_time, "median", ddof=2)
    raises("moments_time: ops 16 is not a set of %s" % MOMENT, v.moments_time, 16, ddof=2)
    raises("moments_time: ddof 2 is neither 0 nor 1", v.moments_time, ddof=2)
    raises("moments_time: ddof True is neither 0 nor 1", v.moments_time, "var", ddof=True)
    raises("moments_time: unknown statistic 'median' (one of %s)" % MOMENT, v.moments_time_groups, bad, "median", ddof=2)
    raises("moments_time: ops 17 is not a set of %s" % MOMENT, v.moments_time_groups, bad, 17, ddof=2)
    raises("moments_time: ddof 2 is neither 0 nor 1", v.moments_time_groups, bad, ddof=2)
    raises("moments_time: ddof 1.0 is neither 0 nor 1", v.moments_time_groups, bad, "var", ddof=1.0)
    raises("moments_time_groups: the labels are float64 (2,), the instants integers (0,)", v.moments_time_groups, bad, ddof=1)
    raises("moments_time_groups: the labels are bool (0,), the instants integers (0,)", v.moments_time_groups, none > 0)


def _filled(d, names, shape, zero):
    assert list(d) == names
    for n, a in d.items():
        assert a.shape == shape and a.dtype == np.float64, (n, a.shape, a.dtype)
        if n in zero:
            assert (a == 0).all() and not np.signbit(a).any(), n
        else:
            assert np.isnan(a).all(), n


def test_variable_without_instants_results(variable):
    v = variable
    _filled(v.moments_time(), ["mean", "std"], (360, 4), ())
    _filled(v.moments_time(15, top=350, left=1, right=3, ddof=1), MOMENT.split(", "), (10, 2), ("count",))
    _filled(v.moments_time(("std", "count"), bottom=0), ["count", "std"], (0, 4), ("count",))
    # no instants, so no non-negative id either: (ids, planes) with no plane
    for lab in (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8)):
        ids, d = v.reduce_time_groups(lab)
        assert ids.shape == (0,) and ids.dtype == lab.dtype
        _filled(d, ["mean"], (0, 360, 4), ())
        ids, d = v.reduce_time_groups(lab, 31, top=350, left=1, right=3)
        assert ids.size == 0
        _filled(d, REDUCE.split(", "), (0, 10, 2), ("sum", "count"))
        ids, d = v.moments_time_groups(lab)
        assert ids.shape == (0,) and ids.dtype == lab.dtype
        _filled(d, ["mean", "std"], (0, 360, 4), ())
        ids, d = v.moments_time_groups(lab, ("var", "count"), right=0, ddof=1)
        assert ids.size == 0
        _filled(d, ["count", "var"], (0, 360, 0), ("count",))


# ---- what every *_flat method hands to _region_call ---------------------------------------------------------------------------------------
#         reversed: 3 instants of 7 x 20 cells    no instants, 5 x 7 cells
CUBES = [[4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 7]]
TAIL = ["out", "mem", "off", "stats"]
U32, I32 = "c_uint", "c_int"
LAB3 = np.array([2, 0xffff, 0], dtype=np.uint16)
NOLAB = np.zeros(0, dtype=np.uint16)
ZL = [np.full((7, 20), 3, dtype=np.uint16), np.full((5, 7), 0xffff, dtype=np.uint16)]
MASK = np.zeros((5, 7))
MASK[1, 2] = -2.5

#    method, its arguments behind the cubes, peek, then what _region_call must see: name, dtype, zeroed, stats, counts, the C tuple
FLAT = [
    ("fill_windows_flat", (np.float32,), {}, "fill_window", np.float32, False, False, [420, 0], ["n", "out", _lib.DCDF_F32, "mem", "off"]),
    ("fill_windows_flat", (), {}, "fill_window", np.int64, False, False, [420, 0], ["n", "out", _lib.DCDF_I64, "mem", "off"]),
    ("decode_flat", (np.int32,), {}, "decode", np.int32, False, True, [420, 0], ["n", "out", _lib.DCDF_I32, "mem", "off", "stats"]),
    ("decode_flat", (), {}, "decode", np.int64, False, True, [420, 0], ["n", "out", _lib.DCDF_I64, "mem", "off", "stats"]),
    ("reduce_time_flat", (("mean", "min"),), {}, "reduce_time", np.float64, False, True, [280, 0], ["n", (U32, 17)] + TAIL),
    ("reduce_time_groups_flat", ("sum", [LAB3, NOLAB], 3), {2: (np.uint16, 4), 3: (np.uint64, 2)}, "reduce_time_groups", np.float64, False, True,
     [420, 0], ["n", (U32, 4), [2, 0xffff, 0, 0], [0, 3], (U32, 3)] + TAIL),
    ("moments_time_flat", (15, 1), {}, "moments_time", np.float64, False, True, [560, 0], ["n", (U32, 15), (U32, 1)] + TAIL),
    ("moments_time_flat", ("std",), {}, "moments_time", np.float64, False, True, [140, 0], ["n", (U32, 8), (U32, 0)] + TAIL),
    ("moments_time_groups_flat", (("var",), [LAB3, NOLAB], 2, 1), {3: (np.uint16, 4), 4: (np.uint64, 2)}, "moments_time_groups", np.float64, False,
     True, [280, 0], ["n", (U32, 4), (U32, 1), [2, 0xffff, 0, 0], [0, 3], (U32, 2)] + TAIL),
    ("moments_time_groups_flat", (6, [LAB3, NOLAB], 300), {}, "moments_time_groups", np.float64, False, True, [2 * 300 * 140, 0],
     ["n", (U32, 6), (U32, 0), "pointer", "pointer", (U32, 300)] + TAIL),
    ("spells_flat", ([0.5, 1.5], 2.0, ("count", "last")), {0: (np.float64, 2), 1: (np.float64, 2)}, "spells", np.uint32, False, True, [280, 0],
     [[0.5, 1.5], [2.0, 2.0], "n", (U32, 17)] + TAIL),
    ("quantile_time_flat", ([0.25, 0.5, 1.0], "nearest"), {1: (np.float64, 3)}, "quantile_time", np.float64, False, True, [420, 0],
     ["n", [0.25, 0.5, 1.0], (U32, 3), (I32, 2)] + TAIL),
    ("quantile_time_flat", (0.5,), {1: (np.float64, 1)}, "quantile_time", np.float64, False, True, [140, 0], ["n", [0.5], (U32, 1), (I32, 3)] + TAIL),
    ("reduce_space_flat", ("max",), {}, "reduce_space", np.float64, False, True, [3, 0], ["n", (U32, 2), None, None, HOST] + TAIL),
    ("reduce_space_flat", (("sum", "count"), [None, MASK]), {2: (np.uint8, 176), 3: (np.uint64, 2)}, "reduce_space", np.float64, False, True, [6, 0],
     ["n", (U32, 12), [1] * 140 + [0] * 9 + [1] + [0] * 25 + [0], [0, 140], HOST] + TAIL),
    ("reduce_space_flat", (31, (8192, [0, 140])), {3: (np.uint64, 2)}, "reduce_space", np.float64, False, True, [15, 0],
     ["n", (U32, 31), "pointer", [0, 140], DEVICE] + TAIL),
    ("zonal_flat", (("min", "sum"), ZL, 4), {2: (np.uint16, 176), 3: (np.uint64, 2)}, "zonal", np.float64, False, True, [24, 0],
     ["n", (U32, 5), [3] * 140 + [0xffff] * 35 + [0], [0, 140], HOST, (U32, 4)] + TAIL),
    ("zonal_flat", ("mean", (8192, [7, 900]), 65535), {3: (np.uint64, 2)}, "zonal", np.float64, False, True, [3 * 65535, 0],
     ["n", (U32, 16), "pointer", [7, 900], DEVICE, (U32, 65535)] + TAIL),
    ("histogram_flat", ([0.0, 1.0, 2.0, 4.0],), {1: (np.float64, 4)}, "histogram", np.uint64, True, True, [9, 0],
     ["n", [0.0, 1.0, 2.0, 4.0], (U32, 3), None, None, HOST] + TAIL),
    ("histogram_flat", ([-np.inf, np.inf], [None, MASK]), {3: (np.uint8, 176)}, "histogram", np.uint64, True, True, [3, 0],
     ["n", "pointer", (U32, 1), [1] * 140 + [0] * 9 + [1] + [0] * 25 + [0], "pointer", HOST] + TAIL),
]


@pytest.mark.parametrize("case", range(len(FLAT)))
def test_flat_methods_hand_down(raster, case):
    method, own, pk, name, dtype, zeroed, stats, counts, args = FLAT[case]
    R = raster
    R.peek = pk
    got = getattr(R, method)(CUBES, *own)
    seen = R.seen.pop()
    assert R.seen == [] and seen["q"] == CUBES and seen["q_dtype"] == np.uint32 and (seen["ptr"], seen["offset"]) == (None, None)
    assert (seen["name"], seen["dtype"], seen["zeroed"], seen["stats"]) == (name, np.dtype(dtype), zeroed, stats)
    assert seen["counts"] == counts and seen["args"] == args
    # the host form: (flat, offsets, kernel ms[, stats])
    assert len(got) == (4 if stats else 3) and got[0].dtype == np.dtype(dtype) and got[1].tolist() == [0, counts[0]] and got[2] == 0.5
    # the device form: the caller's pointer and offsets go down; (kernel ms, stats), or the kernel ms alone
    R.peek = {}
    got = getattr(R, method)(CUBES, *own, out_device_ptr=4096, out_offset=[16, 0])
    seen = R.seen.pop()
    assert (seen["name"], seen["ptr"], seen["offset"], seen["counts"]) == (name, 4096, [16, 0], counts)
    assert got == 0.5 if not stats else (len(got) == 2 and got[0] == 0.5 and got[1].dtype == np.uint64)


# ---- EncodedRaster.decode -----------------------------------------------------------------------------------------------------------------
def test_decode(raster):
    R = raster
    raises("instants [5, 4) outside [0, 10)", R.decode, 5, 4)
    raises("instants [0, 11) outside [0, 10)", R.decode, stop=11)
    raises("instants [-1, 3) outside [0, 10)", R.decode, -1, 3, np.float32)
    raises("instants [11, 10) outside [0, 10)", R.decode, 11)
    for kw in (dict(start=3, stop=3), dict(start=10), dict(start=0, stop=0, dtype=np.float32)):
        d = R.decode(**kw)
        assert d.shape == (0, 50, 60) and d.dtype == np.dtype(kw.get("dtype", np.int64))
    assert R.seen == []
    d = R.decode(2, 4, np.float32)
    assert d.shape == (2, 50, 60) and d.dtype == np.float32 and d[1, 0, :3].tolist() == [3000.0, 3001.0, 3002.0]
    assert R.seen[-1]["name"] == "decode" and R.seen[-1]["q"] == [[2, 4, 0, 50, 0, 60]] and R.seen[-1]["args"][2] == _lib.DCDF_F32
    assert R.decode(7).shape == (3, 50, 60) and R.seen[-1]["q"] == [[7, 10, 0, 50, 0, 60]] and R.seen[-1]["args"][2] == _lib.DCDF_I64


# ---- the unevenness the layer keeps ---------------------------------------------------------------------------------------------------------
def test_ops_prefixes(raster):
    R = raster
    lab, zl = np.zeros(10, dtype=np.uint16), np.zeros((50, 60), dtype=np.uint16)
    raises("reduce_time: ops 32 is not a set of %s" % REDUCE, R.reduce_space, 32)
    raises("reduce_time: ops 32 is not a set of %s" % REDUCE, R.zonal, 32, zl)
    raises("reduce_time: ops 32 is not a set of %s" % REDUCE, R.reduce_time_groups, 32, lab)
    raises("moments_time: ops 32 is not a set of %s" % MOMENT, R.moments_time_groups, 32, lab)


def test_spells_checks_statistics_first_but_variable_without_instants_the_bounds(raster, variable):
    raises("spells: unknown statistic 'median' (one of count, longest, longest_start, first, last)", raster.spells, NAN, 1.0, "median", 3, 3)
    raises("spells: a NaN bound", variable.spells, NAN, 1.0, "median")


def test_who_looks_at_the_mask_without_instants(raster, variable):
    wrong = np.ones((9, 9))
    assert list(variable.reduce_space(mask=wrong)) == ["mean"]
    raises("histogram: the mask has shape (9, 9), the window (360, 4)", variable.histogram, [0.0, 1.0], mask=wrong)
    raises("reduce_space: the mask has shape (9, 9), the window (50, 60)", raster.reduce_space, "sum", 3, 3, mask=wrong)
    raises("histogram: the mask has shape (9, 9), the window (50, 60)", raster.histogram, [0.0, 1.0], 3, 3, mask=wrong)


def test_per_instant_statistics_are_empty_only_without_instants(raster):
    """Without cells the per-instant statistics still make their call (every instant gets its value over nothing); the statistics
    over time answer themselves, n_groups kept in the shape."""
    R = raster
    rows = (5, 5, 0, 60)
    d = R.reduce_space(("sum", "min"), 2, 6, rows)
    assert list(d) == ["min", "sum"] and d["sum"].tolist() == [4, 5, 6, 7] and R.seen[-1]["q"] == [[2, 6, 5, 5, 0, 60]] and R.seen[-1]["counts"] == [8]
    z = R.zonal("count", np.zeros((0, 60), dtype=np.uint16), window=rows, n_zones=3)
    assert z["count"].shape == (3, 10) and R.seen[-1]["name"] == "zonal" and R.seen[-1]["counts"] == [30]
    h = R.histogram([0.0, 1.0, 2.0], 4, 6, rows, np.ones((0, 60)))
    assert h.shape == (2, 2) and h.dtype == np.uint64 and h.tolist() == [[0, 1], [2, 3]] and R.seen[-1]["name"] == "histogram" and len(R.seen) == 3
    lab = np.zeros(10, dtype=np.uint16)
    assert R.reduce_time("sum", window=rows)["sum"].shape == (0, 60) and R.spells(0.0, 1.0, window=rows)["count"].shape == (0, 60)
    assert R.reduce_time_groups("sum", lab, window=rows, n_groups=6)["sum"].shape == (6, 0, 60)
    assert R.moments_time_groups("var", lab, window=rows, n_groups=6)["var"].shape == (6, 0, 60) and len(R.seen) == 3


def test_group_and_zone_counts_default_to_the_largest_label_plus_one(raster):
    R = raster
    lab = np.array([0, 4, 0xffff, 1, 1, 0, 0, 0, 0, 0], dtype=np.uint16)
    assert R.reduce_time_groups("sum", lab, window=(0, 1, 0, 2))["sum"].shape == (5, 1, 2) and R.seen[-1]["args"][4] == (U32, 5)
    assert R.moments_time_groups("var", lab[2:3], 2, 3, (0, 1, 0, 2))["var"].shape == (1, 1, 2) and R.seen[-1]["args"][5] == (U32, 1)
    zl = np.array([[7, 0xffff]], dtype=np.uint16)
    assert R.zonal("sum", zl, window=(0, 1, 0, 2))["sum"].shape == (8, 10) and R.seen[-1]["args"][5] == (U32, 8)
    assert R.zonal("sum", zl[:, 1:], window=(0, 1, 0, 1))["sum"].shape == (1, 10) and R.seen[-1]["args"][5] == (U32, 1)


def test_variable_grouped_calls_return_ids_and_as_many_planes(variable):
    zl = np.full((360, 4), -1)
    ids, z = variable.zonal(zl, 31)
    assert ids.size == 0 and list(z) == REDUCE.split(", ") and all(a.shape == (0, 0) and a.dtype == np.float64 for a in z.values())
    zl[3, 1], zl[9, 0] = 900000, 5
    ids, z = variable.zonal(zl[2:20], "count", top=2, bottom=20)
    assert ids.tolist() == [5, 900000] and z["count"].shape == (2, 0)
    ids, d = variable.reduce_time_groups(np.zeros(0, dtype=np.int32), "count")
    assert ids.size == 0 and d["count"].shape == (0, 360, 4)
