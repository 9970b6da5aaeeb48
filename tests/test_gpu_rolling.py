"""Rolling windows over time (dcdf_raster_rolling_time_batch, dcdf_raster_rolling_time_groups_batch, EncodedRaster.rolling_time* and
Variable.rolling_time*) on the GPU.  Every comparison is on bit patterns against rolling_model.py: Python integers at the 2^-63
scale, every window summed again from its own values, the sums compared as integers, one correctly rounded division; a window
belongs to the group of its last instant."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rolling_model as WM
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
import test_gpu_reduce_time_groups as GT
from test_gpu_bulk_decode import assert_same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ALL = 31
NONE = WM.NONE
SHAPE, TILE, CS, CUBES = RT.FOLD_SHAPE, RT.FOLD_TILE, RT.FOLD_CS, RT.FOLD_CUBES  # (20, 70, 70), 64, 8; the second cube unaligned in every edge
FLAT_CELL = (50, 50)  # a constant cell, set here: the shared sources have none
WINDOWS = (1, 2, 5, 8, 9, 16, 17)  # 17 exceeds the second cube's 16 instants


def source(kind):
    a = RT.fold_source(kind).copy()
    a[:, FLAT_CELL[0], FLAT_CELL[1]] = 7
    return a


def sub(a, cube):
    t0, t1, r0, r1, c0, c1 = RT.norm(cube)
    return a[t0:t1, r0:r1, c0:c1]


def as_mean(d, w):
    """the MEAN kind of a model result: the rounded extreme sums divided by (double)w, one division each"""
    return {n: (v / float(w) if n in ("max", "min") else v) for n, v in d.items()}


def planes(flat, off, q, mask, rows, cols, n_groups=None):
    """Cube q of a rolling_time_flat (n_groups None) or rolling_time_groups_flat result as {name: planes} in plane order."""
    shape = (rows, cols) if n_groups is None else (n_groups, rows, cols)
    n = int(np.prod(shape))
    o = int(off[q])
    return {name: flat[o + i * n:o + (i + 1) * n].reshape(shape) for i, name in enumerate(WM.names_of(mask))}


def check(flat, off, q, ops, cube, want, n_groups=None):
    """want: the model's {name: [n_groups, rows, cols]}; the plain call is its group 0"""
    t0, t1, r0, r1, c0, c1 = RT.norm(cube)
    got = planes(flat, off, q, ops, r1 - r0, c1 - c0, n_groups)
    assert list(got) == WM.names_of(ops)
    for n in got:
        assert_same(got[n], want[n][0] if n_groups is None else want[n])


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


@pytest.fixture(scope="module")
def rasters(dc):
    made = {}

    def get(kind):
        if kind not in made:
            a = source(kind)
            made[kind] = (a, BD.build_raster(dc, a, TILE, CS))
        return made[kind]

    yield get
    for _, r in made.values():
        r.close()


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_and_piece(rasters, kind):
    """Bulk chunks, two strips and the 6 x 6 corner chunk on the fallback walk, three segments with the last one short, the NaN
    cells and patch; plain and every label set, every window of WINDOWS, min_count 1 and the window, SUM and MEAN.  The model's
    outputs are made first and shown to hold the cases that matter."""
    a, R = rasters(kind)
    nts = [c[1] - c[0] for c in CUBES]
    sets = [[("plain", None, 1)] + GT.label_sets(nt) for nt in nts]
    seen = dict(none=False, one=False, empty_group=False, differ=False, tie=False)
    wants = {}
    for w in WINDOWS:
        sums = [WM.window_sums(sub(a, c), w) for c in CUBES]
        for s in range(len(sets[0])):
            for mc in sorted({1, w}):
                wants[w, s, mc] = [WM.fold(*sums[q], w, mc, False, sets[q][s][1], sets[q][s][2]) for q in range(len(CUBES))]
                for q, d in enumerate(wants[w, s, mc]):
                    seen["none"] |= bool((d["count"][0] == 0).any()) and s == 0
                    seen["one"] |= bool((d["count"] == 1).any())
                    seen["differ"] |= bool((d["argmax"] != d["argmin"])[d["count"] > 0].any())
                    if sets[q][s][0] == "odd":
                        assert (d["count"][[1, 3]] == 0).all() and np.isnan(d["max"][[1, 3]]).all()
                        seen["empty_group"] = True
                    if s == 0 and q == 0 and w < nts[0]:
                        r, c = FLAT_CELL
                        assert d["count"][0, r, c] == nts[0] - w + 1 > 1 and d["argmax"][0, r, c] == d["argmin"][0, r, c] == w - 1
                        assert d["max"][0, r, c] == d["min"][0, r, c] == 7.0 * w
                        seen["tie"] = True
    assert all(seen.values()), seen
    _, _, _, dstats = R.decode_flat(CUBES, dtype=a.dtype)
    for w in WINDOWS:
        for s in range(len(sets[0])):
            sname, _, n_groups = sets[0][s]
            labels = None if s == 0 else [sets[q][s][1].astype(np.uint16) for q in range(len(CUBES))]
            for mc, mean in [(m, False) for m in sorted({1, w})] + [(w, True)]:
                if s == 0:
                    flat, off, ms, stats = R.rolling_time_flat(CUBES, ALL, w, mc, mean)
                    assert ms > 0
                else:
                    flat, off, ms, stats = R.rolling_time_groups_flat(CUBES, ALL, labels, n_groups, w, mc, mean)
                np.testing.assert_array_equal(stats, dstats)  # neither the window nor the labels change what is read
                for q, c in enumerate(CUBES):
                    want = wants[w, s, mc][q]
                    check(flat, off, q, ALL, c, as_mean(want, w) if mean else want, None if s == 0 else n_groups)
                if sname == "one":
                    pflat, poff, _, _ = R.rolling_time_flat(CUBES, ALL, w, mc, mean)
                    np.testing.assert_array_equal(off, poff)
                    assert_same(flat, pflat)
    assert int(dstats[1]) > 0 and (kind[1:] == "64" or int(dstats[0]) > 0)
    # the whole-raster forms: instants counted from `start`
    d = R.rolling_time(("argmax", "max", "count"), 5, 2, start=2, stop=19, region=(60, 70, 3, 70))
    want = WM.rolling_time(a[2:19, 60:70, 3:70], 5, 2)
    assert list(d) == ["max", "argmax", "count"]
    for n in d:
        assert_same(d[n], want[n])
    lab = (np.arange(17) % 3).astype(np.uint16)
    d = R.rolling_time_groups(ALL, lab, 4, mean=True, start=2, stop=19, region=(60, 70, 3, 70))
    want = WM.rolling_time_groups(a[2:19, 60:70, 3:70], 4, lab, 3, mean=True)
    for n in WM.NAMES:
        assert_same(d[n], want[n])


def test_rounding_is_not_the_order(dc):
    """Sums that round to one double but differ are no tie: the comparison is on the exact integers.  Cells near +-2^62 need more
    than 64 bits at the 2^-63 scale and more than 53 for the sum."""
    a = np.zeros((8, 64, 64), dtype=np.int64)
    a[:, :, :] = (np.arange(8)[:, None, None] * 3 + np.arange(64)[None, :, None] - np.arange(64)[None, None, :]) % 11 - 5
    a[:4, 3, 5] = [2 ** 53, 2 ** 53, 2 ** 53 + 2, 0]
    a[4:, 3, 5] = 0
    a[:, 40, 41] = [2 ** 62 - 1, 2 ** 62 - 3, -(2 ** 62) + 1, 2 ** 62 - 5, -(2 ** 62) + 7, -(2 ** 62) + 9, 2 ** 61 + 1, 5]
    a[:, 41, 40] = [2 ** 53 + 1, 1, 1, -(2 ** 53) - 1, 2 ** 53 + 3, 1, 0, 2]
    x = a[:, 3, 5].astype(np.float64)
    rounded = x[1:] + x[:-1]
    assert rounded[0] == rounded[1] == 2.0 ** 54 and int(np.argmax(rounded)) + 1 == 1, "the input proves nothing"
    R = BD.build_raster(dc, a, 64, 8)
    dec, _, _, _ = R.decode_flat([[0, 8, 0, 64, 0, 64]], dtype=np.int64)
    np.testing.assert_array_equal(dec.reshape(a.shape), a)
    for w, mc in ((2, 2), (2, 1), (3, 3), (5, 5), (8, 8)):
        want = WM.rolling_time(a, w, mc)
        if w == 2:
            assert want["argmax"][3, 5] == 2 and want["max"][3, 5] == 2.0 ** 54
        flat, off, _, _ = R.rolling_time_flat([[0, 8, 0, 64, 0, 64]], ALL, w, mc)
        got = planes(flat, off, 0, ALL, 64, 64)
        for n in WM.NAMES:
            assert_same(got[n], want[n])
        flat, off, _, _ = R.rolling_time_flat([[0, 8, 0, 64, 0, 64]], 5, w, w, True)
        got = planes(flat, off, 0, 5, 64, 64)
        want = WM.rolling_time(a, w, w, True)
        assert_same(got["max"], want["max"])
        assert_same(got["min"], want["min"])
    R.close()


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_window_of_one_is_reduce_time(rasters, kind):
    """No model: window 1 with SUM gives reduce_time's max, min and count bit for bit; for i32 the whole range as one window with
    min_count 1 gives reduce_time's sum (every partial sum is below 2^53)."""
    a, R = rasters(kind)
    flat, off, _, _ = R.rolling_time_flat(CUBES, 1 | 4 | 16, 1)
    rflat, roff, _, _ = R.reduce_time_flat(CUBES, 1 | 2 | 8)  # min, max, count
    for q, c in enumerate(CUBES):
        t0, t1, r0, r1, c0, c1 = RT.norm(c)
        got = planes(flat, off, q, 21, r1 - r0, c1 - c0)
        n = (r1 - r0) * (c1 - c0)
        red = rflat[int(roff[q]):int(roff[q]) + 3 * n].reshape(3, r1 - r0, c1 - c0)
        assert_same(got["max"], red[1])
        assert_same(got["min"], red[0])
        assert_same(got["count"], red[2])
    if kind == "i32":
        for q, c in enumerate(CUBES):
            t0, t1, r0, r1, c0, c1 = RT.norm(c)
            flat, off, _, _ = R.rolling_time_flat([c], 1 | 16, t1 - t0, 1)
            sflat, soff, _, _ = R.reduce_time_flat([c], 4)
            got = planes(flat, off, 0, 17, r1 - r0, c1 - c0)
            assert_same(got["max"], sflat[:(r1 - r0) * (c1 - c0)].reshape(r1 - r0, c1 - c0))
            assert (got["count"] == 1).all()


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_every_ops(rasters, kind):
    """Every `ops` in 1 .. 31 with a change of group at every instant: the planes in their places, whichever are asked for."""
    a, R = rasters(kind)
    labels = [(np.arange(c[1] - c[0]) % 3).astype(np.uint16) for c in CUBES]
    want = [WM.rolling_time_groups(sub(a, c), 3, labels[q], 3, 2) for q, c in enumerate(CUBES)]
    plain = [WM.rolling_time_groups(sub(a, c), 3, None, 1, 2) for c in CUBES]
    for ops in range(1, 32):
        flat, off, _, stats = R.rolling_time_groups_flat(CUBES, ops, labels, 3, 3, 2)
        assert int(stats[0]) > 0 and int(stats[1]) > 0 and int(stats.sum()) == BD.volume(CUBES)
        pflat, poff, _, _ = R.rolling_time_flat(CUBES, ops, 3, 2)
        for q, c in enumerate(CUBES):
            check(flat, off, q, ops, c, want[q], 3)
            check(pflat, poff, q, ops, c, plain[q])


def test_one_group_is_the_plain_call(rasters):
    a, R = rasters("f32")
    for w, mc, mean in ((5, 2, False), (4, 4, True), (17, 1, False)):
        flat, off, _, stats = R.rolling_time_flat(CUBES, ALL, w, mc, mean)
        gflat, goff, _, gstats = R.rolling_time_groups_flat(CUBES, ALL, [np.zeros(c[1] - c[0], dtype=np.uint16) for c in CUBES], 1, w, mc, mean)
        np.testing.assert_array_equal(off, goff)
        np.testing.assert_array_equal(stats, gstats)
        assert_same(flat, gflat)


def _device_form(R, a, cubes, ops, labels, w, mc, skip):
    """Both output forms of the plain and the grouped call over `cubes` (those of `skip` write nothing): the host form against the
    model; the device form with odd gaps between the cubes and a sentinel around the planes."""
    from dcdf_amd.encoder import DeviceBuffer
    nb = np.array([RT.norm(c) for c in cubes], dtype=np.int64)
    n_ops = len(WM.names_of(ops))
    for n_groups in (None, 3):
        if n_groups is None:
            call = lambda **kw: R.rolling_time_flat(cubes, ops, w, mc, **kw)
        else:
            call = lambda **kw: R.rolling_time_groups_flat(cubes, ops, labels, n_groups, w, mc, **kw)
        flat, off, _, stats = call()
        for q, c in enumerate(cubes):
            if q not in skip:
                check(flat, off, q, ops, c, WM.rolling_time_groups(sub(a, c), w, None if n_groups is None else labels[q], n_groups or 1, mc), n_groups)
        vol = (n_ops * (n_groups or 1) * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
        assert all(vol[q] == 0 for q in skip)
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64))
        doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)  # odd gaps: the planes meet misaligned addresses
        total = int(doff[-1] + vol[-1]) + 7
        buf = DeviceBuffer(total * 8)
        buf.write(0, np.full(total, -77.25, dtype=np.float64))
        ms, dvstats = call(out_device_ptr=buf.ptr, out_offset=doff)
        g = buf.read(0, total * 8, np.float64)
        buf.free()
        np.testing.assert_array_equal(dvstats, stats)
        inside = np.zeros(total, dtype=bool)
        for q in range(len(cubes)):
            o, n = int(doff[q]), int(vol[q])
            inside[o:o + n] = True
            assert_same(g[o:o + n], flat[int(off[q]):int(off[q]) + n])
        assert (g[~inside] == -77.25).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's planes


def test_both_output_forms(rasters):
    a, R = rasters("f32")
    cubes = CUBES + [[6, 6, 0, 30, 0, 30], [19, 2, 69, 50, 1, 0]]  # one without instants: writes nothing; one with reversed bounds
    labels = [(np.arange(abs(c[1] - c[0])) % 3).astype(np.uint16) for c in cubes]
    _device_form(R, a, cubes, 2 | 4 | 16, labels, 5, 3, skip=(2,))


def test_batch_with_cubes_that_write_nothing(rasters):
    """[cube with cells, cube without instants, cube without cells, cube with cells], every cube with a label array of its own:
    those of the two that write nothing are the caller's alone."""
    a, R = rasters("f32")
    cubes = [CUBES[1], [6, 6, 0, 30, 0, 30], [2, 9, 40, 40, 3, 50], [19, 1, 66, 2, 69, 4]]
    i = np.arange(20)
    labels = [(i[:16] % 3).astype(np.uint16), np.zeros(0, dtype=np.uint16), np.full(7, 1, dtype=np.uint16), (2 - i[:18] // 7).astype(np.uint16)]
    labels[3][[0, 11]] = NONE
    _device_form(R, a, cubes, ALL, labels, 4, 1, skip=(1, 2))


CHILD = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import dcdf_amd
import rolling_model as WM
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
assert os.environ["K2R_QUANTILE_SLAB_BYTES"] == "400000"
a = RT.source("f32")
R = BD.build_raster(dcdf_amd, a, RT.TILE, RT.CS)
T, Rr, Cc = RT.SHAPE
cubes = [[0, T, 0, Rr, 0, Cc], [3, 19, 17, 260, 5, 133]]
labels = [(np.arange(c[1] - c[0]) // 6).astype(np.uint16) for c in cubes]
labels[0][0] = 0xffff
# 400 000 bytes: 2 500 cells of 20 instants.  The 256 x 256 columns are cut into 64 x 64 parts of 655 360 bytes, each over the cap
# and alone in its band; the 8-row and 8-column strips (2 048 cells) fit whole, one a band; the corner chunk shares one.
calls = (lambda: R.rolling_time_flat(cubes, 31, 5, 3), lambda: R.rolling_time_groups_flat(cubes, 31, labels, 4, 5, 3))
small = [f() for f in calls]
del os.environ["K2R_QUANTILE_SLAB_BYTES"]
same = lambda x, y: np.array_equal(WM.bits(x), WM.bits(y))
sums = [WM.window_sums(a[t0:t1, r0:r1, c0:c1], 5) for t0, t1, r0, r1, c0, c1 in cubes]  # (once per cube: both calls fold them)
for n_groups, f, (flat, off, _, stats) in zip((None, 4), calls, small):
    dflat, doff, _, dstats = f()
    assert np.array_equal(off, doff) and np.array_equal(stats, dstats)
    assert same(flat, dflat)
    for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes):
        want = WM.fold(*sums[q], 5, 3, False, None if n_groups is None else labels[q], n_groups or 1)
        n = (n_groups or 1) * (r1 - r0) * (c1 - c0)
        for i, name in enumerate(WM.NAMES):
            assert same(flat[int(off[q]) + i * n:int(off[q]) + (i + 1) * n], want[name].ravel()), (n_groups, q, name)
print("STATS", int(stats[0]), int(stats[1]), int(stats[2]))
"""


def test_a_small_slab_in_a_child_process():
    """K2R_QUANTILE_SLAB_BYTES so small that the (20, 264, 264) cube takes many bands and its 64 x 64 parts are over the cap alone:
    the results equal the default's, bit for bit, and the model's."""
    env = dict(os.environ, K2R_QUANTILE_SLAB_BYTES="400000")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    walk = 20 * 8 * 8  # the corner chunk: it lies in the first cube alone
    assert "STATS %d %d 0" % (20 * 264 * 264 + 16 * 243 * 128 - walk, walk) in out.stdout, out.stdout[-500:]


def test_segments_of_one_cell_with_different_fractional_bits(dc, dtype=np.float64):
    """Three segments built apart with 0, 25 and 12 fractional bits (the reduce_time test's raster): the same stored integer means
    another value in every segment, so head and tail must each be widened with their own segment's entry -- windows and groups
    that cross the segment boundaries."""
    a, chunks, EncodedRaster = RT.order_raster(dc, dtype)
    want = WM.rolling_time(a, 5, 5)
    as_first = np.concatenate([a[0:8], a[8:16] * 2.0 ** 25, a[16:24] * 2.0 ** 12]).astype(dtype)
    assert (WM.bits(WM.rolling_time(as_first, 5, 5)["max"]) != WM.bits(want["max"])).any(), "one segment's bits give the same sums: the input proves nothing"
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    cubes = [[0, 24, 0, 64, 0, 64], [3, 21, 5, 64, 0, 59], [8, 24, 0, 64, 0, 64]]
    for w in (5, 9):
        flat, off, _, stats = R.rolling_time_flat(cubes, ALL, w)
        assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0
        for q, c in enumerate(cubes):
            check(flat, off, q, ALL, c, WM.rolling_time_groups(sub(a, c), w, None, 1))
    lab = (np.arange(24) // 5 % 2).astype(np.uint16)  # groups that cross the segment boundaries
    flat, off, _, _ = R.rolling_time_groups_flat(cubes[:1], ALL, [lab], 2, 7, 7, True)
    check(flat, off, 0, ALL, cubes[0], WM.rolling_time_groups(a, 7, lab, 2, 7, True), 2)
    R.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
@pytest.mark.parametrize("levels,shape", [([4, 8], (34, 300, 2060)), ([1, 6, 5], (40, 40, 2112))], ids=["4x8", "1x6x5_offset_leaves"])
def test_stored_variable(dtype, levels, shape):
    """Elided tiles, nested levels, offset leaves, a short last segment; signed ids, negative = no group."""
    import test_gpu_stored_raster as SR
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    rng = np.random.default_rng(sum(shape))
    a = SR.var_data(rng, shape, dtype, 1 << levels[-1])
    v = SR.make_var(dataset, a, levels, 32)
    T, Rr, Cc = shape
    win = (7, T - 1, 5, Rr - 3, 250, 400)  # instants 7 .. T - 2: across the segment boundary at 32; columns across a tile's edge
    x = v.window(*win)
    got = v.rolling_time(5, WM.NAMES, 3, False, *win)
    want = WM.rolling_time(x, 5, 3)
    assert list(got) == list(WM.NAMES)
    for n in WM.NAMES:
        assert_same(got[n], want[n])
    _, _, _, stats = v.raster().rolling_time_flat([[0, T, 0, Rr, 0, Cc]], 16, 3)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    ids_in = rng.choice(np.array([-7, -1, 2, 40, 100000]), size=T)
    ids_in[:5] = [-1, 40, 2, 100000, 40]
    sel = ids_in[7:T - 1]
    ids, got = v.rolling_time_groups(sel, 4, ("min", "argmin", "count"), None, True, *win)
    present = [g for g in (2, 40, 100000) if (sel == g).any()]
    assert ids.tolist() == present and list(got) == ["min", "argmin", "count"]
    dense = np.full(T - 8, NONE)
    for i, g in enumerate(ids):
        dense[sel == g] = i
    want = WM.rolling_time_groups(x, 4, dense, len(ids), 4, True)
    for n in got:
        assert_same(got[n], want[n])
    # the whole variable, the cheap statistic of it: an elided leaf's cells come from its per-instant values
    whole = v.rolling_time(2, "count", 1)
    dec = v.decode()
    ok = ~np.isnan(dec.astype(np.float64))
    assert_same(whole["count"], ((ok[1:] | ok[:-1]).sum(axis=0)).astype(np.float64))
    none_ids, none = v.rolling_time_groups(np.full(T, -4), 3, ("count", "max"))
    assert none_ids.size == 0 and none["count"].shape == (0, Rr, Cc)
    with pytest.raises(ValueError):
        v.rolling_time_groups(ids_in[1:], 3)
    with pytest.raises(ValueError):
        v.rolling_time(0)
    with pytest.raises(IndexError):
        v.rolling_time(3, stop=T + 1)


def test_edges_and_errors(dc, rasters):
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(4096, dtype=np.float64)
    off = np.zeros(1, dtype=np.uint64)
    loff = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()
    lab = np.array([1, 0, 1, NONE], dtype=np.uint16)
    o, f, lp, lo = (C.c_void_p(x.ctypes.data) for x in (out, off, lab, loff))
    st0 = C.c_void_p(stats.ctypes.data)

    def cubes_of(cubes):
        return None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))

    def plain(h, cubes, nq, ops, w, mc, kind, outp, offp, mem=L.MEM_HOST, st=st0, msp=C.byref(ms)):
        q = cubes_of(cubes)
        return lib.dcdf_raster_rolling_time_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops), C.c_uint32(w),
                                                  C.c_uint32(mc), C.c_int32(kind), outp, mem, offp, st, msp)

    def grouped(h, cubes, nq, ops, w, mc, kind, labp, loffp, n_groups, outp, offp, mem=L.MEM_HOST, st=st0, msp=C.byref(ms)):
        q = cubes_of(cubes)
        return lib.dcdf_raster_rolling_time_groups_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops),
                                                         C.c_uint32(w), C.c_uint32(mc), C.c_int32(kind), labp, loffp, C.c_uint32(n_groups), outp, mem,
                                                         offp, st, msp)

    h = R._handle()
    small = [[0, 3, 0, 2, 0, 2]]
    x = a[0:3, :2, :2]
    out[:] = -1
    assert plain(h, small, 1, 1 | 8, 2, 2, 0, o, f) == 0 and int(stats.sum()) == 12
    want = WM.rolling_time(x, 2)
    assert_same(out[:8], np.concatenate([want["max"].ravel(), want["argmin"].ravel()]))
    assert (out[8:] == -1).all()
    out[:] = -1
    assert grouped(h, small, 1, 2 | 16, 2, 1, 0, lp, lo, 2, o, f) == 0 and int(stats.sum()) == 12
    want = WM.rolling_time_groups(x, 2, lab[:3], 2, 1)
    assert_same(out[:16], np.concatenate([want["argmax"].ravel(), want["count"].ravel()]))
    assert (out[16:] == -1).all()
    out[:] = -1
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert plain(h, bad, 1, 1, 1, 1, 0, o, f) == -5 and grouped(h, bad, 1, 1, 1, 1, 0, lp, lo, 2, o, f) == -5  # DCDF_ERR_BOUNDS
    # DCDF_ERR_BAD_ARG: the statistics, the window, min_count, the kind, the mean over a varying count
    for ops, w, mc, kind in ((0, 2, 1, 0), (32, 2, 1, 0), (33, 2, 1, 0), (1 << 20, 2, 1, 0), (1, 0, 1, 0), (1, 0, 0, 0), (1, 65536, 1, 0),
                             (1, 1 << 31, 1, 0), (1, 2, 0, 0), (1, 2, 3, 0), (1, 2, 1, 2), (1, 2, 1, -1), (1, 2, 1, 1), (1, 3, 2, 1)):
        assert plain(h, small, 1, ops, w, mc, kind, o, f) == -1, (ops, w, mc, kind)
        assert grouped(h, small, 1, ops, w, mc, kind, lp, lo, 2, o, f) == -1, (ops, w, mc, kind)
    for ng in (0, 65536, 1 << 31):
        assert grouped(h, small, 1, 1, 2, 1, 0, lp, lo, ng, o, f) == -1
    assert plain(h, small, 1, 1, 2, 1, 0, o, f, mem=7) == -1 and grouped(h, small, 1, 1, 2, 1, 0, lp, lo, 65535, o, f, mem=7) == -1
    assert plain(None, small, 1, 1, 2, 1, 0, o, f) == -1 and grouped(None, small, 1, 1, 2, 1, 0, lp, lo, 2, o, f) == -1  # NULL arguments
    assert plain(h, None, 1, 1, 2, 1, 0, o, f) == -1 and grouped(h, None, 1, 1, 2, 1, 0, lp, lo, 2, o, f) == -1
    assert plain(h, small, 1, 1, 2, 1, 0, None, f) == -1 and grouped(h, small, 1, 1, 2, 1, 0, lp, lo, 2, None, f) == -1
    assert plain(h, small, 1, 1, 2, 1, 0, o, None) == -1 and grouped(h, small, 1, 1, 2, 1, 0, lp, lo, 2, o, None) == -1
    assert grouped(h, small, 1, 1, 2, 1, 0, None, lo, 2, o, f) == -1 and grouped(h, small, 1, 1, 2, 1, 0, lp, None, 2, o, f) == -1
    assert plain(h, small, 0, 1, 2, 1, 0, o, f) == 0 and grouped(h, small, 0, 1, 2, 1, 0, None, None, 2, o, f) == 0  # nq == 0 is fine
    assert (out == -1).all()  # nothing written on any refusal
    assert plain(h, small, 1, 31, 65535, 65535, 1, o, f, st=None, msp=None) == 0  # the widest window: no window, every element written
    assert_same(out[:20], np.concatenate([np.full(16, np.nan), np.zeros(4)]))
    assert (out[20:] == -1).all()
    out[:] = -1
    # stats and kernel_ms may be NULL; a cube without instants, rows or columns writes nothing
    for empty in ([[2, 2, 0, 5, 0, 5]], [[0, 3, 4, 4, 0, 5]], [[0, 3, 0, 5, 7, 7]]):
        assert plain(h, empty, 1, 31, 2, 1, 0, o, f, st=None, msp=None) == 0
        assert grouped(h, empty, 1, 31, 2, 1, 0, lp, lo, 2, o, f, st=None, msp=None) == 0
    assert (out == -1).all()
    # every label NONE, or beyond n_groups: NaN, NaN, NaN, NaN, 0 everywhere, every element written
    none = np.array([NONE, 2, NONE, 5], dtype=np.uint16)
    assert grouped(h, [[0, 4, 3, 5, 60, 67]], 1, 31, 2, 1, 0, C.c_void_p(none.ctypes.data), lo, 2, o, f, st=None, msp=None) == 0
    p = out[:5 * 2 * 14].reshape(5, 2 * 14)
    assert_same(p, np.concatenate([np.full((4, 28), np.nan), np.zeros((1, 28))]))
    assert (out[140:] == -1).all()
    # the wrappers' own refusals
    good = (np.arange(20) % 2).astype(np.uint16)
    for labels, ng in (([good.astype(np.int32)], 2), ([good[:19]], 2), ([good], 0), ([good], 65536), ([good, good], 2)):
        with pytest.raises(ValueError):
            R.rolling_time_groups_flat(CUBES[:1], 1, labels, ng, 3)
    for w, mc, mean in ((0, None, False), (65536, None, False), (3, 0, False), (3, 4, False), (3, 2, True)):
        with pytest.raises(ValueError):
            R.rolling_time_flat(CUBES[:1], 1, w, mc, mean)
        with pytest.raises(ValueError):
            R.rolling_time_groups_flat(CUBES[:1], 1, [good], 2, w, mc, mean)
    with pytest.raises(ValueError):
        R.rolling_time("mean", 3)
    # a raster holding a k * k > 64 chunk: DCDF_ERR_UNSUPPORTED, as for quantiles
    a9 = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R9 = BD.build_raster(dc, a9, 20, 4, k=9)
    for call in (lambda: R9.rolling_time_flat([[0, 4, 0, 20, 0, 20]], ALL, 2),
                 lambda: R9.rolling_time_groups_flat([[0, 4, 0, 20, 0, 20]], ALL, [np.zeros(4, dtype=np.uint16)], 1, 2)):
        with pytest.raises(L.DcdfError) as e:
            call()
        assert e.value.code == -8
    R9.close()
