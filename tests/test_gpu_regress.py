"""Regression over time (dcdf_raster_regress_time_batch, dcdf_raster_regress_time_groups_batch, EncodedRaster.regress_time* and
Variable.regress_time*) on the GPU.  Every comparison is on bit patterns against regress_model.py: the shifted sums (c, K, sy, syy,
se, see, sey) in instant order, per group the plain model over the group's instants, each with its own regressor value.  The flat
forms take the regressor as given, the whole-raster and Variable forms less its first value (regress_model.shifted)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import regress_model as RM
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
import test_gpu_reduce_time_groups as GT
from test_gpu_bulk_decode import assert_same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ALL = 15
NONE = RM.NONE
SHAPE, TILE, CS, CUBES = RT.FOLD_SHAPE, RT.FOLD_TILE, RT.FOLD_CS, RT.FOLD_CUBES  # (20, 70, 70), 64, 8; the second cube unaligned in every edge
SMALL = GT.SMALL  # 5 x 7 cells across the tile boundary at column 64
FLAT_CELL = (50, 50)  # a constant cell, set here: the shared sources have none


def regressor(nt, q=0):
    """neither monotone nor integer, and not near zero at its first instant"""
    return np.sin(np.arange(nt) * 1.7 + q) * 3.25 + 0.375 * (np.arange(nt) % 4) - 1.5


def source(kind):
    a = RT.fold_source(kind).copy()
    a[:, FLAT_CELL[0], FLAT_CELL[1]] = 7
    return a


def sub(a, cube):
    t0, t1, r0, r1, c0, c1 = RT.norm(cube)
    return a[t0:t1, r0:r1, c0:c1]


def planes(flat, off, q, mask, rows, cols, n_groups=None):
    """Cube q of a regress_time_flat (n_groups None) or regress_time_groups_flat result as {name: planes} in plane order."""
    shape = (rows, cols) if n_groups is None else (n_groups, rows, cols)
    n = int(np.prod(shape))
    o = int(off[q])
    return {name: flat[o + i * n:o + (i + 1) * n].reshape(shape) for i, name in enumerate(RM.names_of(mask))}


def check(flat, off, q, ops, cube, want, n_groups=None):
    t0, t1, r0, r1, c0, c1 = RT.norm(cube)
    got = planes(flat, off, q, ops, r1 - r0, c1 - c0, n_groups)
    assert list(got) == RM.names_of(ops)
    for n in got:
        assert_same(got[n], want[n])


def branches(wants):
    """Which branches of regress_finish a list of model outputs shows: {name: bool}."""
    seen = dict(count0=False, count1=False, all_finite=False, flat=False)
    for w in wants:
        c = w["count"]
        seen["count0"] |= bool((c == 0).any())
        seen["count1"] |= bool((c == 1).any())
        seen["all_finite"] |= bool((np.isfinite(w["slope"]) & np.isfinite(w["intercept"]) & np.isfinite(w["corr"])).any())
        seen["flat"] |= bool(((w["slope"] == 0) & ~np.signbit(w["slope"]) & (w["intercept"] == 7) & np.isnan(w["corr"]) & (c >= 2)).any())
    return seen


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
    """Bulk chunks, two strips and the 6 x 6 corner chunk on the fallback walk, three segments with the last one short; plain and
    every label set, against the instant index and against a regressor that is neither monotone nor integer.  The model's outputs
    are made first and shown to hold every branch of the finish."""
    a, R = rasters(kind)
    nts = [c[1] - c[0] for c in CUBES]
    sets = [GT.label_sets(nt) for nt in nts]
    pairs = [i // 2 for i in (np.arange(nts[0]), np.arange(nts[1]))]  # labels i // 2 with the regressor i // 2: See == 0 in every group
    regs = {"index": None, "series": [regressor(nt, q) for q, nt in enumerate(nts)]}
    e_of = lambda name, q: np.arange(nts[q], dtype=np.float64) if regs[name] is None else regs[name][q]
    want_plain = {name: [RM.regress_time(sub(a, c), e_of(name, q)) for q, c in enumerate(CUBES)] for name in regs}
    want_sets = {(name, s): [RM.regress_time_groups(sub(a, c), e_of(name, q), sets[q][s][1], sets[q][s][2]) for q, c in enumerate(CUBES)]
                 for name in regs for s in range(len(sets[0]))}
    want_pairs = [RM.regress_time_groups(sub(a, c), pairs[q].astype(np.float64), pairs[q], 10) for q, c in enumerate(CUBES)]
    seen = branches([w for ws in list(want_plain.values()) + list(want_sets.values()) for w in ws])
    assert all(seen.values()), seen
    for w in want_pairs:  # >= 2 valid instants and See == 0: NaN but for the count
        full = w["count"] == 2
        assert full.any() and all(np.isnan(w[n][full]).all() for n in ("slope", "intercept", "corr"))
    odd = [s for s in range(len(sets[0])) if sets[0][s][0] == "odd"][0]
    assert (want_sets["series", odd][0]["count"][[1, 3]] == 0).all() and np.isnan(want_sets["series", odd][0]["slope"][[1, 3]]).all()
    _, _, _, dstats = R.decode_flat(CUBES, dtype=a.dtype)
    for name, given in regs.items():
        flat, off, ms, stats = R.regress_time_flat(CUBES, ALL, given)
        assert ms > 0
        np.testing.assert_array_equal(stats, dstats)
        assert int(stats[1]) > 0 and (kind[1:] == "64" or int(stats[0]) > 0)
        for q, c in enumerate(CUBES):
            check(flat, off, q, ALL, c, want_plain[name][q])
        for s in range(len(sets[0])):
            sname, _, n_groups = sets[0][s]
            labels = [sets[q][s][1].astype(np.uint16) for q in range(len(CUBES))]
            gflat, goff, _, gstats = R.regress_time_groups_flat(CUBES, ALL, labels, n_groups, given)
            np.testing.assert_array_equal(gstats, dstats)  # neither the labels nor the regressor change what is read
            for q, c in enumerate(CUBES):
                check(gflat, goff, q, ALL, c, want_sets[name, s][q], n_groups)
            if sname == "one":
                np.testing.assert_array_equal(goff, off)
                assert_same(gflat, flat)
    gflat, goff, _, _ = R.regress_time_groups_flat(CUBES, ALL, [p.astype(np.uint16) for p in pairs], 10, [p.astype(np.float64) for p in pairs])
    for q, c in enumerate(CUBES):
        check(gflat, goff, q, ALL, c, want_pairs[q], 10)
    # the whole-raster forms pass the regressor less its first value; None is the instant index
    u = regressor(17) + 1990.0
    d = R.regress_time(("corr", "slope", "intercept"), u, 2, 19, window=(60, 70, 3, 70))
    want = RM.regress_time(a[2:19, 60:70, 3:70], RM.shifted(u))
    assert list(d) == ["slope", "intercept", "corr"]
    for n in d:
        assert_same(d[n], want[n])
    assert (RM.bits(RM.regress_time(a[2:19, 60:70, 3:70], u)["slope"]) != RM.bits(want["slope"])).any()  # (as given: other bits)
    d = R.regress_time(start=3, stop=19, window=(3, 66, 5, 68))
    assert list(d) == ["slope"]
    assert_same(d["slope"], want_plain["index"][1]["slope"])
    lab = (np.arange(17) % 3).astype(np.uint16)
    d = R.regress_time_groups(ALL, lab, u, 2, 19, window=(60, 70, 3, 70))
    want = RM.regress_time_groups(a[2:19, 60:70, 3:70], RM.shifted(u), lab, 3)
    for n in RM.NAMES:
        assert_same(d[n], want[n])


def test_small_with_300_groups(rasters):
    a, R = rasters("f32")
    lab = np.array([0, 150, 299], dtype=np.uint16)[np.arange(20) % 3]
    e = regressor(20)
    want = RM.regress_time_groups(sub(a, SMALL[0]), e, lab, 300)
    assert (want["count"][[1, 149, 151, 298]] == 0).all() and np.isfinite(want["corr"][[0, 150, 299]]).any()
    flat, off, _, stats = R.regress_time_groups_flat(SMALL, ALL, [lab], 300, [e])
    assert int(stats.sum()) == 20 * 5 * 7
    check(flat, off, 0, ALL, SMALL[0], want, 300)


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_every_ops(rasters, kind):
    """Every `ops` in 1 .. 15 with a change of group at every instant: the planes in their places, whichever are asked for."""
    a, R = rasters(kind)
    labels = [(np.arange(c[1] - c[0]) % 3).astype(np.uint16) for c in CUBES]
    regs = [regressor(c[1] - c[0], q) for q, c in enumerate(CUBES)]
    want = [RM.regress_time_groups(sub(a, c), regs[q], labels[q], 3) for q, c in enumerate(CUBES)]
    plain = [RM.regress_time(sub(a, c), np.arange(c[1] - c[0], dtype=np.float64)) for c in CUBES]
    if kind == "f32":
        assert (want[0]["count"] == 0).any() and (want[0]["count"] == 1).any() and (want[0]["count"] > 2).any()
    for ops in range(1, 16):
        flat, off, _, stats = R.regress_time_groups_flat(CUBES, ops, labels, 3, regs)
        assert int(stats[0]) > 0 and int(stats[1]) > 0 and int(stats.sum()) == BD.volume(CUBES)
        pflat, poff, _, _ = R.regress_time_flat(CUBES, ops)
        for q, c in enumerate(CUBES):
            check(flat, off, q, ops, c, want[q], 3)
            check(pflat, poff, q, ops, c, plain[q])


def test_one_group_is_the_plain_call_and_the_host_function(rasters):
    from dcdf_amd import _lib
    a, R = rasters("f32")
    regs = [regressor(c[1] - c[0], q) for q, c in enumerate(CUBES)]
    flat, off, _, stats = R.regress_time_flat(CUBES, ALL, regs)
    gflat, goff, _, gstats = R.regress_time_groups_flat(CUBES, ALL, [np.zeros(c[1] - c[0], dtype=np.uint16) for c in CUBES], 1, regs)
    np.testing.assert_array_equal(off, goff)
    np.testing.assert_array_equal(stats, gstats)
    assert_same(flat, gflat)
    # dcdf_regress_host over the series fill_cell returns: a bulk cell, the all-NaN cell, the cell with one value, one inside the
    # NaN patch, one in the right strip, one in the corner chunk
    cells = [(5, 9), (17, 23), (40, 5), (12, 31), (33, 68), (66, 67)]
    series, soff, _ = R.fill_cells_flat([[0, 20, r, c] for r, c in cells], dtype=np.float32)
    got = planes(flat, off, 0, ALL, 70, 70)
    for i, (r, c) in enumerate(cells):
        x = series[int(soff[i]):int(soff[i]) + 20]
        np.testing.assert_array_equal(x.view(np.uint32), a[:, r, c].view(np.uint32))
        _, o = _lib.regress_host(x.astype(np.float64), regs[0])
        assert_same(np.array([got[n][r, c] for n in RM.NAMES]), o)


def _device_form(R, a, cubes, ops, labels, regs, skip):
    """Both output forms of the plain and the grouped call over `cubes` (those of `skip` write nothing): the host form against the
    model; the device form with odd gaps between the cubes and a sentinel around the planes."""
    from dcdf_amd.encoder import DeviceBuffer
    nb = np.array([RT.norm(c) for c in cubes], dtype=np.int64)
    n_ops = len(RM.names_of(ops))
    for n_groups in (None, 3):
        if n_groups is None:
            call = lambda **kw: R.regress_time_flat(cubes, ops, regs, **kw)
        else:
            call = lambda **kw: R.regress_time_groups_flat(cubes, ops, labels, n_groups, regs, **kw)
        flat, off, _, stats = call()
        for q, c in enumerate(cubes):
            if q not in skip:
                want = RM.regress_time(sub(a, c), regs[q]) if n_groups is None else RM.regress_time_groups(sub(a, c), regs[q], labels[q], n_groups)
                check(flat, off, q, ops, c, want, n_groups)
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
    regs = [regressor(abs(c[1] - c[0]), q) for q, c in enumerate(cubes)]
    _device_form(R, a, cubes, 14, labels, regs, skip=(2,))


def test_batch_with_cubes_that_write_nothing(rasters):
    """[cube with cells, cube without instants, cube without cells, cube with cells], every cube with label and regressor arrays of
    its own: those of the two that write nothing are the caller's alone."""
    a, R = rasters("f32")
    cubes = [CUBES[1], [6, 6, 0, 30, 0, 30], [2, 9, 40, 40, 3, 50], [19, 1, 66, 2, 69, 4]]
    i = np.arange(20)
    labels = [(i[:16] % 3).astype(np.uint16), np.zeros(0, dtype=np.uint16), np.full(7, 1, dtype=np.uint16), (2 - i[:18] // 7).astype(np.uint16)]
    labels[3][[0, 11]] = NONE
    regs = [regressor(16), np.zeros(0), regressor(7, 2), regressor(18, 3)]
    _device_form(R, a, cubes, ALL, labels, regs, skip=(1, 2))


CHILD = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import dcdf_amd
import regress_model as RM
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
assert os.environ["K2R_QUANTILE_SLAB_BYTES"] == "400000"
a = RT.source("f32")
R = BD.build_raster(dcdf_amd, a, RT.TILE, RT.CS)
T, Rr, Cc = RT.SHAPE
cubes = [[0, T, 0, Rr, 0, Cc], [3, 19, 17, 260, 5, 133]]
regs = [np.cos(np.arange(c[1] - c[0]) * 2.3) * 1.75 + 0.5 for c in cubes]
labels = [(np.arange(c[1] - c[0]) %% 3).astype(np.uint16) for c in cubes]
labels[0][0] = 0xffff
# 400 000 bytes: 2 500 cells of 20 instants.  The 256 x 256 columns are cut into 64 x 64 parts of 655 360 bytes, each over the cap
# and alone in its band; the 8-row and 8-column strips (2 048 cells) fit whole, one a band; the corner chunk shares one.
calls = (lambda: R.regress_time_flat(cubes, 15, regs), lambda: R.regress_time_groups_flat(cubes, 15, labels, 3, regs))
small = [f() for f in calls]
del os.environ["K2R_QUANTILE_SLAB_BYTES"]
same = lambda x, y: np.array_equal(RM.bits(x), RM.bits(y))
for n_groups, f, (flat, off, _, stats) in zip((None, 3), calls, small):
    dflat, doff, _, dstats = f()
    assert np.array_equal(off, doff) and np.array_equal(stats, dstats)
    assert same(flat, dflat)
    for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes):
        x = a[t0:t1, r0:r1, c0:c1]
        want = RM.regress_time(x, regs[q]) if n_groups is None else RM.regress_time_groups(x, regs[q], labels[q], n_groups)
        n = (n_groups or 1) * (r1 - r0) * (c1 - c0)
        for i, name in enumerate(RM.NAMES):
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
    another value in every segment, so the values must be widened with their own segment's entry."""
    a, chunks, EncodedRaster = RT.order_raster(dc, dtype)
    e = regressor(24)
    want = RM.regress_time(a, e)
    # were every instant widened with the first segment's bits, the slopes would be others
    as_first = np.concatenate([a[0:8], a[8:16] * 2.0 ** 25, a[16:24] * 2.0 ** 12]).astype(dtype)
    assert (RM.bits(RM.regress_time(as_first, e)["slope"]) != RM.bits(want["slope"])).any(), "one segment's bits give the same slopes: the input proves nothing"
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    cubes = [[0, 24, 0, 64, 0, 64], [3, 21, 5, 64, 0, 59], [8, 24, 0, 64, 0, 64]]
    regs = [e, e[3:21], e[8:24]]
    flat, off, _, stats = R.regress_time_flat(cubes, ALL, regs)
    assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0
    for q, c in enumerate(cubes):
        check(flat, off, q, ALL, c, RM.regress_time(sub(a, c), regs[q]))
    lab = (np.arange(24) // 5 % 2).astype(np.uint16)  # groups that cross the segment boundaries
    flat, off, _, _ = R.regress_time_groups_flat(cubes[:1], ALL, [lab], 2, [e])
    check(flat, off, 0, ALL, cubes[0], RM.regress_time_groups(a, e, lab, 2), 2)
    R.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
@pytest.mark.parametrize("levels,shape", [([4, 8], (34, 300, 2060)), ([1, 6, 5], (40, 40, 2112))], ids=["4x8", "1x6x5_offset_leaves"])
def test_stored_variable(dtype, levels, shape):
    """Elided tiles, nested levels, offset leaves, a short last segment; signed ids, negative = no group.  An elided leaf has one
    value per instant: its cells' line comes from those."""
    import test_gpu_stored_raster as SR
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    rng = np.random.default_rng(sum(shape))
    a = SR.var_data(rng, shape, dtype, 1 << levels[-1])
    v = SR.make_var(dataset, a, levels, 32)
    T, Rr, Cc = shape
    dec = v.decode()
    years = 1979.0 + regressor(T)
    got = v.regress_time(RM.NAMES, years)
    want = RM.regress_time(dec, RM.shifted(years))
    assert list(got) == list(RM.NAMES)
    for n in RM.NAMES:
        assert_same(got[n], want[n])
    _, _, _, stats = v.raster().regress_time_flat([[0, T, 0, Rr, 0, Cc]], 1)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    win = (7, T - 1, 5, Rr - 3, 250, Cc - 9)
    got = v.regress_time(("slope",), None, *win)
    assert_same(got["slope"], RM.regress_time(v.window(*win), RM.shifted(None, T - 8))["slope"])
    ids_in = rng.choice(np.array([-7, -1, 2, 40, 100000]), size=T)
    ids_in[:5] = [-1, 40, 2, 100000, 40]
    ids, got = v.regress_time_groups(ids_in, RM.NAMES, years)
    assert ids.tolist() == [2, 40, 100000] and list(got) == list(RM.NAMES)
    dense = np.full(T, NONE)
    for i, g in enumerate(ids):
        dense[ids_in == g] = i
    want = RM.regress_time_groups(dec, RM.shifted(years), dense, 3)
    for n in RM.NAMES:
        assert_same(got[n], want[n])
    ids, got = v.regress_time_groups(ids_in[7:T - 1], ("corr", "count"), years[7:T - 1], *win)
    present = [g for g in (2, 40, 100000) if (ids_in[7:T - 1] == g).any()]
    assert ids.tolist() == present and list(got) == ["count", "corr"]
    dense = np.full(T - 8, NONE)
    for i, g in enumerate(ids):
        dense[ids_in[7:T - 1] == g] = i
    want = RM.regress_time_groups(v.window(*win), RM.shifted(years[7:T - 1]), dense, len(ids))
    assert_same(got["count"], want["count"])
    assert_same(got["corr"], want["corr"])
    none_ids, none = v.regress_time_groups(np.full(T, -4), ("count", "slope"))
    assert none_ids.size == 0 and none["count"].shape == (0, Rr, Cc)
    with pytest.raises(ValueError):
        v.regress_time_groups(ids_in[1:])
    with pytest.raises(ValueError):
        v.regress_time(regressor=years[1:])
    with pytest.raises(IndexError):
        v.regress_time(stop=T + 1)


def test_edges_and_errors(dc, rasters):
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(4096, dtype=np.float64)
    off = np.zeros(1, dtype=np.uint64)
    loff = np.zeros(1, dtype=np.uint64)
    roff = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()
    lab = np.array([1, 0, 1, NONE], dtype=np.uint16)
    reg = np.array([0.5, -1.25, 3.0, 2.0])
    o, f, lp, lo, rp, ro = (C.c_void_p(x.ctypes.data) for x in (out, off, lab, loff, reg, roff))
    st0 = C.c_void_p(stats.ctypes.data)

    def cubes_of(cubes):
        return None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))

    def plain(h, cubes, nq, ops, regp, roffp, outp, offp, mem=L.MEM_HOST, st=st0, msp=C.byref(ms)):
        q = cubes_of(cubes)
        return lib.dcdf_raster_regress_time_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops), regp, roffp,
                                                  outp, mem, offp, st, msp)

    def grouped(h, cubes, nq, ops, regp, roffp, labp, loffp, n_groups, outp, offp, mem=L.MEM_HOST, st=st0, msp=C.byref(ms)):
        q = cubes_of(cubes)
        return lib.dcdf_raster_regress_time_groups_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops), regp,
                                                         roffp, labp, loffp, C.c_uint32(n_groups), outp, mem, offp, st, msp)

    h = R._handle()
    small = [[0, 3, 0, 2, 0, 2]]
    x = a[0:3, :2, :2]
    out[:] = -1
    assert plain(h, small, 1, 1 | 4, None, None, o, f) == 0 and int(stats.sum()) == 12
    want = RM.regress_time(x, [0.0, 1.0, 2.0])
    assert_same(out[:8], np.concatenate([want["count"].ravel(), want["intercept"].ravel()]))
    assert (out[8:] == -1).all()
    out[:] = -1
    assert grouped(h, small, 1, 2 | 8, rp, ro, lp, lo, 2, o, f) == 0 and int(stats.sum()) == 12
    want = RM.regress_time_groups(x, reg[:3], lab[:3], 2)
    assert_same(out[:16], np.concatenate([want["slope"].ravel(), want["corr"].ravel()]))
    assert (out[16:] == -1).all()
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert plain(h, bad, 1, 1, None, None, o, f) == -5 and grouped(h, bad, 1, 1, None, None, lp, lo, 2, o, f) == -5  # DCDF_ERR_BOUNDS
    for ops in (0, 16, 17, 1 << 20):
        assert plain(h, small, 1, ops, None, None, o, f) == -1 and grouped(h, small, 1, ops, None, None, lp, lo, 2, o, f) == -1  # DCDF_ERR_BAD_ARG
    for ng in (0, 65536, 1 << 31):
        assert grouped(h, small, 1, 1, None, None, lp, lo, ng, o, f) == -1
    assert plain(h, small, 1, 1, None, None, o, f, mem=7) == -1 and grouped(h, small, 1, 1, None, None, lp, lo, 65535, o, f, mem=7) == -1
    assert plain(None, small, 1, 1, None, None, o, f) == -1 and grouped(None, small, 1, 1, None, None, lp, lo, 2, o, f) == -1  # NULL arguments
    assert plain(h, None, 1, 1, None, None, o, f) == -1 and grouped(h, None, 1, 1, None, None, lp, lo, 2, o, f) == -1
    assert plain(h, small, 1, 1, None, None, None, f) == -1 and grouped(h, small, 1, 1, None, None, lp, lo, 2, None, f) == -1
    assert plain(h, small, 1, 1, None, None, o, None) == -1 and grouped(h, small, 1, 1, None, None, lp, lo, 2, o, None) == -1
    assert grouped(h, small, 1, 1, None, None, None, lo, 2, o, f) == -1 and grouped(h, small, 1, 1, None, None, lp, None, 2, o, f) == -1
    # the regressor and its offsets: both or neither
    assert plain(h, small, 1, 1, rp, None, o, f) == -1 and plain(h, small, 1, 1, None, ro, o, f) == -1
    assert grouped(h, small, 1, 1, rp, None, lp, lo, 2, o, f) == -1 and grouped(h, small, 1, 1, None, ro, lp, lo, 2, o, f) == -1
    assert plain(h, small, 0, 1, None, None, o, f) == 0 and grouped(h, small, 0, 1, None, None, None, None, 2, o, f) == 0  # nq == 0 is fine
    # a regressor value that is not finite, wherever it stands among the cube's instants: refused, nothing written
    out[:] = -1
    for at in range(3):
        for v in (np.nan, np.inf, -np.inf):
            bad = reg.copy()
            bad[at] = v
            bp = C.c_void_p(bad.ctypes.data)
            assert plain(h, small, 1, 15, bp, ro, o, f) == -1 and grouped(h, small, 1, 15, bp, ro, lp, lo, 2, o, f) == -1
    assert (out == -1).all()
    # stats and kernel_ms may be NULL; a cube without instants, rows or columns writes nothing
    for empty in ([[2, 2, 0, 5, 0, 5]], [[0, 3, 4, 4, 0, 5]], [[0, 3, 0, 5, 7, 7]]):
        assert plain(h, empty, 1, 15, rp, ro, o, f, st=None, msp=None) == 0
        assert grouped(h, empty, 1, 15, rp, ro, lp, lo, 2, o, f, st=None, msp=None) == 0
    assert (out == -1).all()
    # every label NONE, or beyond n_groups: 0, NaN, NaN, NaN everywhere, every element written
    none = np.array([NONE, 2, NONE, 5], dtype=np.uint16)
    assert grouped(h, [[0, 4, 3, 5, 60, 67]], 1, 15, rp, ro, C.c_void_p(none.ctypes.data), lo, 2, o, f, st=None, msp=None) == 0
    p = out[:4 * 2 * 14].reshape(4, 2 * 14)
    assert_same(p, np.concatenate([np.zeros((1, 28)), np.full((3, 28), np.nan)]))
    assert (out[112:] == -1).all()
    # the wrappers' own refusals
    good = (np.arange(20) % 2).astype(np.uint16)
    for labels, ng in (([good.astype(np.int32)], 2), ([good[:19]], 2), ([good], 0), ([good], 65536), ([good, good], 2)):
        with pytest.raises(ValueError):
            R.regress_time_groups_flat(CUBES[:1], 1, labels, ng)
    for regs in ([np.zeros(19)], [np.zeros(20), np.zeros(20)], [np.full(20, np.inf)], [np.zeros(20, dtype=bool)], [np.zeros((20, 1))]):
        with pytest.raises(ValueError):
            R.regress_time_flat(CUBES[:1], 1, regs)
        with pytest.raises(ValueError):
            R.regress_time_groups_flat(CUBES[:1], 1, [good], 2, regs)
    with pytest.raises(ValueError):
        R.regress_time("mean")
    with pytest.raises(ValueError):
        R.regress_time("slope", np.zeros(19))
    # a raster holding a k * k > 64 chunk: DCDF_ERR_UNSUPPORTED, as for quantiles
    a9 = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R9 = BD.build_raster(dc, a9, 20, 4, k=9)
    for call in (lambda: R9.regress_time_flat([[0, 4, 0, 20, 0, 20]], ALL),
                 lambda: R9.regress_time_groups_flat([[0, 4, 0, 20, 0, 20]], ALL, [np.zeros(4, dtype=np.uint16)], 1)):
        with pytest.raises(L.DcdfError) as e:
            call()
        assert e.value.code == -8
    R9.close()
