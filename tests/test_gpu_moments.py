"""Moments over time (dcdf_raster_moments_time_batch, dcdf_raster_moments_time_groups_batch, EncodedRaster.moments_time* and
Variable.moments_time*) on the GPU.  Every comparison is on bit patterns against moment_model.py: the shifted sums (c, K, s1, s2)
in instant order, per group the plain model over the group's instants."""
import ctypes as C

import numpy as np
import pytest

import moment_model as MM
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
import test_gpu_reduce_time_groups as GT
from test_gpu_bulk_decode import assert_same
from test_moments_host import shift_source

pytestmark = pytest.mark.gpu
ALL = 15
NONE = MM.NONE
SHAPE, TILE, CS, CUBES = RT.FOLD_SHAPE, RT.FOLD_TILE, RT.FOLD_CS, RT.FOLD_CUBES  # (20, 70, 70), 64, 8; the second cube unaligned in every edge
SMALL = GT.SMALL  # 5 x 7 cells across the tile boundary at column 64


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
            a = RT.fold_source(kind)
            made[kind] = (a, BD.build_raster(dc, a, TILE, CS))
        return made[kind]

    yield get
    for _, r in made.values():
        r.close()


def sub(a, cube):
    t0, t1, r0, r1, c0, c1 = RT.norm(cube)
    return a[t0:t1, r0:r1, c0:c1]


def check(flat, off, q, ops, cube, want, n_groups=None):
    t0, t1, r0, r1, c0, c1 = RT.norm(cube)
    got = MM.planes(flat, off, q, ops, r1 - r0, c1 - c0, n_groups)
    assert list(got) == MM.names_of(ops)
    for n in got:
        assert_same(got[n], want[n])


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_and_piece(rasters, kind):
    """Bulk chunks, two strips and the 6 x 6 corner chunk on the fallback walk, three segments with the last one short; the float
    sources have all-NaN cells and cells whose first value -- K -- comes at a later instant, in a later segment."""
    a, R = rasters(kind)
    _, _, _, dstats = R.decode_flat(CUBES, dtype=a.dtype)
    sets = [GT.label_sets(c[1] - c[0]) for c in CUBES]
    if kind[0] == "f":
        first = np.argmax(~np.isnan(a), axis=0)  # (0 for an all-NaN cell)
        later = CUBES[1][0] + np.argmax(~np.isnan(sub(a, CUBES[1])), axis=0)
        assert np.isnan(a).all(axis=0).any() and (later >= CS).any() and ((first > 0) & (first < CS)).any()
    for ddof in (0, 1):
        flat, off, ms, stats = R.moments_time_flat(CUBES, ALL, ddof)
        assert ms > 0
        np.testing.assert_array_equal(stats, dstats)
        assert int(stats[1]) > 0 and (kind[1:] == "64" or int(stats[0]) > 0)
        for q, c in enumerate(CUBES):
            check(flat, off, q, ALL, c, MM.moments_time(sub(a, c), ddof))
        for s in range(len(sets[0])):
            name, _, n_groups = sets[0][s]
            labels = [sets[q][s][1].astype(np.uint16) for q in range(len(CUBES))]
            gflat, goff, _, gstats = R.moments_time_groups_flat(CUBES, ALL, labels, n_groups, ddof)
            np.testing.assert_array_equal(gstats, dstats)  # the labels do not change what is read
            for q, c in enumerate(CUBES):
                want = MM.moments_time_groups(sub(a, c), labels[q], n_groups, ddof)
                check(gflat, goff, q, ALL, c, want, n_groups)
                if name == "odd":
                    assert (want["count"][[1, 3]] == 0).all() and np.isnan(want["std"][[1, 3]]).all()
            if name == "one":
                np.testing.assert_array_equal(goff, off)
                assert_same(gflat, flat)
    lab = np.array([0, 150, 299], dtype=np.uint16)[np.arange(20) % 3]
    flat, off, _, stats = R.moments_time_groups_flat(SMALL, ALL, [lab], 300, 1)
    assert int(stats.sum()) == 20 * 5 * 7
    want = MM.moments_time_groups(sub(a, SMALL[0]), lab, 300, 1)
    check(flat, off, 0, ALL, SMALL[0], want, 300)
    assert (want["count"][[1, 149, 151, 298]] == 0).all()
    d = R.moments_time(("std", "mean"), 2, 19, window=(60, 70, 3, 70), ddof=1)
    want = MM.moments_time(a[2:19, 60:70, 3:70], 1)
    assert list(d) == ["mean", "std"]
    assert_same(d["mean"], want["mean"])
    assert_same(d["std"], want["std"])


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_every_ops(rasters, kind):
    """Every `ops` in 1 .. 15 with a change of group at every instant: COUNT in its output plane or in scratch, the derived planes
    in their places."""
    a, R = rasters(kind)
    labels = [(np.arange(c[1] - c[0]) % 3).astype(np.uint16) for c in CUBES]
    want = [MM.moments_time_groups(sub(a, c), labels[q], 3, 1) for q, c in enumerate(CUBES)]
    plain = [MM.moments_time(sub(a, c), 0) for c in CUBES]
    if kind == "f32":
        assert (want[0]["count"] == 0).any() and (want[0]["count"] == 1).any() and (want[0]["count"] > 2).any()
    for ops in range(1, 16):
        flat, off, _, stats = R.moments_time_groups_flat(CUBES, ops, labels, 3, 1)
        assert int(stats[0]) > 0 and int(stats[1]) > 0 and int(stats.sum()) == BD.volume(CUBES)
        pflat, poff, _, _ = R.moments_time_flat(CUBES, ops)
        for q, c in enumerate(CUBES):
            check(flat, off, q, ops, c, want[q], 3)
            check(pflat, poff, q, ops, c, plain[q])


def test_one_group_is_the_plain_call_and_the_host_function(rasters):
    from dcdf_amd import _lib
    a, R = rasters("f32")
    flat, off, _, stats = R.moments_time_flat(CUBES, ALL, 1)
    gflat, goff, _, gstats = R.moments_time_groups_flat(CUBES, ALL, [np.zeros(c[1] - c[0], dtype=np.uint16) for c in CUBES], 1, 1)
    np.testing.assert_array_equal(off, goff)
    np.testing.assert_array_equal(stats, gstats)
    assert_same(flat, gflat)
    # dcdf_moments_host over the series fill_cell returns: a bulk cell, the all-NaN cell, the cell with one value, one inside the
    # NaN patch, one in the right strip, one in the corner chunk
    cells = [(5, 9), (17, 23), (40, 5), (12, 31), (33, 68), (66, 67)]
    series, soff, _ = R.fill_cells_flat([[0, 20, r, c] for r, c in cells], dtype=np.float32)
    got = MM.planes(flat, off, 0, ALL, 70, 70)
    for i, (r, c) in enumerate(cells):
        x = series[int(soff[i]):int(soff[i]) + 20]
        np.testing.assert_array_equal(x.view(np.uint32), a[:, r, c].view(np.uint32))
        _, o = _lib.moments_host(x.astype(np.float64), ddof=1)
        assert_same(np.array([got[n][r, c] for n in MM.NAMES]), o)


def test_the_shift_is_there(dc):
    """int32 values 2^30 +- 3, three segments: the model's bits (the unshifted sums of squares give others:
    tests/test_moments_host.py), VAR and STD unchanged by a constant added to every value, STD correctly rounded.  Values of 2^30
    and more are beyond the bulk kernel's chunks; the same noise around 2^30 - 8 takes it."""
    cube = [[0, 24, 0, 64, 0, 64]]
    labels = [(np.arange(24) % 2).astype(np.uint16)]
    got = {}
    for base in (1 << 30, (1 << 30) - 8, (1 << 30) - 8 - 1_000_000):
        a = shift_source(base)
        R = BD.build_raster(dc, a, 64, 8)
        for ddof in (0, 1):
            flat, off, _, stats = R.moments_time_flat(cube, ALL, ddof)
            assert int(stats.sum()) == a.size and (base == 1 << 30 or int(stats[0]) == a.size)
            want = MM.moments_time(a, ddof)
            check(flat, off, 0, ALL, cube[0], want)
            got[base, ddof] = MM.planes(flat, off, 0, ALL, 64, 64)
            assert_same(got[base, ddof]["std"], np.sqrt(want["var"]))
            assert (want["var"] > 0).all()
        gflat, goff, _, _ = R.moments_time_groups_flat(cube, ALL, labels, 2, 1)
        check(gflat, goff, 0, ALL, cube[0], MM.moments_time_groups(a, labels[0], 2, 1), 2)
        R.close()
    for ddof in (0, 1):
        x, y, z = (got[b, ddof] for b in (1 << 30, (1 << 30) - 8, (1 << 30) - 8 - 1_000_000))
        for n in ("var", "std"):
            assert_same(x[n], y[n])
            assert_same(y[n], z[n])


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
@pytest.mark.parametrize("levels,shape", [([4, 8], (34, 300, 2060)), ([1, 6, 5], (40, 40, 2112))], ids=["4x8", "1x6x5_offset_leaves"])
def test_stored_variable(dtype, levels, shape):
    """Elided tiles, nested levels, offset leaves, a short last segment; signed ids, negative = no group.  An elided leaf has one
    value per instant: its cells' VAR comes from those."""
    import test_gpu_stored_raster as SR
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    rng = np.random.default_rng(sum(shape))
    a = SR.var_data(rng, shape, dtype, 1 << levels[-1])
    v = SR.make_var(dataset, a, levels, 32)
    T, Rr, Cc = shape
    dec = v.decode()
    got = v.moments_time(MM.NAMES, ddof=1)
    want = MM.moments_time(dec, 1)
    assert list(got) == list(MM.NAMES)
    for n in MM.NAMES:
        assert_same(got[n], want[n])
    _, _, _, stats = v.raster().moments_time_flat([[0, T, 0, Rr, 0, Cc]], 8)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    win = (7, T - 1, 5, Rr - 3, 250, Cc - 9)
    got = v.moments_time(("var",), *win)
    assert_same(got["var"], MM.moments_time(v.window(*win))["var"])
    ids_in = rng.choice(np.array([-7, -1, 2, 40, 100000]), size=T)
    ids_in[:5] = [-1, 40, 2, 100000, 40]
    ids, got = v.moments_time_groups(ids_in, MM.NAMES)
    assert ids.tolist() == [2, 40, 100000] and list(got) == list(MM.NAMES)
    dense = np.full(T, NONE)
    for i, g in enumerate(ids):
        dense[ids_in == g] = i
    want = MM.moments_time_groups(dec, dense, 3)
    for n in MM.NAMES:
        assert_same(got[n], want[n])
    ids, got = v.moments_time_groups(ids_in[7:T - 1], ("std", "count"), *win, ddof=1)
    present = [g for g in (2, 40, 100000) if (ids_in[7:T - 1] == g).any()]
    assert ids.tolist() == present and list(got) == ["count", "std"]
    dense = np.full(T - 8, NONE)
    for i, g in enumerate(ids):
        dense[ids_in[7:T - 1] == g] = i
    want = MM.moments_time_groups(v.window(*win), dense, len(ids), 1)
    assert_same(got["count"], want["count"])
    assert_same(got["std"], want["std"])
    none_ids, none = v.moments_time_groups(np.full(T, -4), ("count", "var"))
    assert none_ids.size == 0 and none["count"].shape == (0, Rr, Cc)
    with pytest.raises(ValueError):
        v.moments_time_groups(ids_in[1:])
    with pytest.raises(IndexError):
        v.moments_time(stop=T + 1)


def test_both_output_forms(rasters):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters("f32")
    cubes = CUBES + [[6, 6, 0, 30, 0, 30], [19, 2, 69, 50, 1, 0]]  # one without instants: writes nothing; one with reversed bounds
    labels = [(np.arange(abs(c[1] - c[0])) % 3).astype(np.uint16) for c in cubes]
    ops = 14  # mean, var, std: the count lives in scratch
    nb = np.array([RT.norm(c) for c in cubes], dtype=np.int64)
    for n_groups in (None, 3):
        if n_groups is None:
            call = lambda **kw: R.moments_time_flat(cubes, ops, 1, **kw)
        else:
            call = lambda **kw: R.moments_time_groups_flat(cubes, ops, labels, n_groups, 1, **kw)
        flat, off, _, stats = call()
        for q, c in enumerate(cubes):
            if q != 2:
                want = MM.moments_time(sub(a, c), 1) if n_groups is None else MM.moments_time_groups(sub(a, c), labels[q], n_groups, 1)
                check(flat, off, q, ops, c, want, n_groups)
        vol = (3 * (n_groups or 1) * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
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


def test_batch_with_cubes_that_write_nothing(rasters):
    """[cube with cells, cube without instants, cube without cells, cube with cells], every cube with a label array of its own: the
    labels of the two that write nothing are the caller's alone, so the last cube's lie elsewhere on the device than on the host."""
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters("f32")
    cubes = [CUBES[1], [6, 6, 0, 30, 0, 30], [2, 9, 40, 40, 3, 50], [19, 1, 66, 2, 69, 4]]
    i = np.arange(20)
    labels = [(i[:16] % 3).astype(np.uint16), np.zeros(0, dtype=np.uint16), np.full(7, 1, dtype=np.uint16), (2 - i[:18] // 7).astype(np.uint16)]
    labels[3][[0, 11]] = NONE
    ops = ALL
    nb = np.array([RT.norm(c) for c in cubes], dtype=np.int64)
    for n_groups in (None, 3):
        if n_groups is None:
            call = lambda **kw: R.moments_time_flat(cubes, ops, 1, **kw)
        else:
            call = lambda **kw: R.moments_time_groups_flat(cubes, ops, labels, n_groups, 1, **kw)
        flat, off, _, stats = call()
        for q in (0, 3):
            c = cubes[q]
            want = MM.moments_time(sub(a, c), 1) if n_groups is None else MM.moments_time_groups(sub(a, c), labels[q], n_groups, 1)
            check(flat, off, q, ops, c, want, n_groups)
        vol = (4 * (n_groups or 1) * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
        assert vol[1] == 0 and vol[2] == 0 and vol[0] and vol[3]
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64))
        doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
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


def test_small_fold_slabs(rasters, monkeypatch):
    """The fallback walk's slab capped at two instants of the raster (the cap is read on every call): pieces cut in time inside a
    segment, same bits."""
    a, R = rasters("f64")
    labels = [(np.arange(c[1] - c[0]) // 3 % 2).astype(np.uint16) for c in CUBES]
    before = (R.moments_time_flat(CUBES, ALL, 1), R.moments_time_groups_flat(CUBES, ALL, labels, 2, 1))
    monkeypatch.setenv("K2R_REDUCE_SLAB_CELLS", str(2 * 70 * 70))
    after = (R.moments_time_flat(CUBES, ALL, 1), R.moments_time_groups_flat(CUBES, ALL, labels, 2, 1))
    for (f0, o0, _, s0), (f1, o1, _, s1) in zip(before, after):
        np.testing.assert_array_equal(o0, o1)
        np.testing.assert_array_equal(s0, s1)
        assert_same(f0, f1)
    for q, c in enumerate(CUBES):
        check(after[0][0], after[0][1], q, ALL, c, MM.moments_time(sub(a, c), 1))
        check(after[1][0], after[1][1], q, ALL, c, MM.moments_time_groups(sub(a, c), labels[q], 2, 1), 2)


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

    def plain(h, cubes, nq, ops, ddof, outp, offp, mem=L.MEM_HOST, st=st0, msp=C.byref(ms)):
        q = cubes_of(cubes)
        return lib.dcdf_raster_moments_time_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops), C.c_uint32(ddof),
                                                  outp, mem, offp, st, msp)

    def grouped(h, cubes, nq, ops, ddof, labp, loffp, n_groups, outp, offp, mem=L.MEM_HOST, st=st0, msp=C.byref(ms)):
        q = cubes_of(cubes)
        return lib.dcdf_raster_moments_time_groups_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops),
                                                         C.c_uint32(ddof), labp, loffp, C.c_uint32(n_groups), outp, mem, offp, st, msp)

    h = R._handle()
    small = [[0, 3, 0, 2, 0, 2]]
    x = a[0:3, :2, :2]
    out[:] = -1
    assert plain(h, small, 1, 1 | 4, 1, o, f) == 0 and int(stats.sum()) == 12
    want = MM.moments_time(x, 1)
    assert_same(out[:8], np.concatenate([want["count"].ravel(), want["var"].ravel()]))
    assert (out[8:] == -1).all()
    out[:] = -1
    assert grouped(h, small, 1, 2 | 8, 0, lp, lo, 2, o, f) == 0 and int(stats.sum()) == 12
    want = MM.moments_time_groups(x, lab[:3], 2, 0)
    assert_same(out[:16], np.concatenate([want["mean"].ravel(), want["std"].ravel()]))
    assert (out[16:] == -1).all()
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert plain(h, bad, 1, 1, 0, o, f) == -5 and grouped(h, bad, 1, 1, 0, lp, lo, 2, o, f) == -5  # DCDF_ERR_BOUNDS
    for ops in (0, 16, 17, 1 << 20):
        assert plain(h, small, 1, ops, 0, o, f) == -1 and grouped(h, small, 1, ops, 0, lp, lo, 2, o, f) == -1  # DCDF_ERR_BAD_ARG
    for ddof in (2, 1 << 31):
        assert plain(h, small, 1, 4, ddof, o, f) == -1 and grouped(h, small, 1, 4, ddof, lp, lo, 2, o, f) == -1
    for ng in (0, 65536, 1 << 31):
        assert grouped(h, small, 1, 1, 0, lp, lo, ng, o, f) == -1
    assert plain(h, small, 1, 1, 0, o, f, mem=7) == -1 and grouped(h, small, 1, 1, 0, lp, lo, 65535, o, f, mem=7) == -1
    assert plain(None, small, 1, 1, 0, o, f) == -1 and grouped(None, small, 1, 1, 0, lp, lo, 2, o, f) == -1  # NULL arguments
    assert plain(h, None, 1, 1, 0, o, f) == -1 and grouped(h, None, 1, 1, 0, lp, lo, 2, o, f) == -1
    assert plain(h, small, 1, 1, 0, None, f) == -1 and grouped(h, small, 1, 1, 0, lp, lo, 2, None, f) == -1
    assert plain(h, small, 1, 1, 0, o, None) == -1 and grouped(h, small, 1, 1, 0, lp, lo, 2, o, None) == -1
    assert grouped(h, small, 1, 1, 0, None, lo, 2, o, f) == -1 and grouped(h, small, 1, 1, 0, lp, None, 2, o, f) == -1
    assert plain(h, small, 0, 1, 0, o, f) == 0 and grouped(h, small, 0, 1, 0, None, None, 2, o, f) == 0  # nq == 0 is fine
    # stats and kernel_ms may be NULL; a cube without instants, rows or columns writes nothing
    out[:] = -1
    for empty in ([[2, 2, 0, 5, 0, 5]], [[0, 3, 4, 4, 0, 5]], [[0, 3, 0, 5, 7, 7]]):
        assert plain(h, empty, 1, 15, 1, o, f, st=None, msp=None) == 0
        assert grouped(h, empty, 1, 15, 1, lp, lo, 2, o, f, st=None, msp=None) == 0
    assert (out == -1).all()
    # every label NONE, or beyond n_groups: 0, NaN, NaN, NaN everywhere, every element written
    none = np.array([NONE, 2, NONE, 5], dtype=np.uint16)
    assert grouped(h, [[0, 4, 3, 5, 60, 67]], 1, 15, 0, C.c_void_p(none.ctypes.data), lo, 2, o, f, st=None, msp=None) == 0
    p = out[:4 * 2 * 14].reshape(4, 2 * 14)
    assert_same(p, np.concatenate([np.zeros((1, 28)), np.full((3, 28), np.nan)]))
    assert (out[112:] == -1).all()
    # the wrappers' own refusals
    good = (np.arange(20) % 2).astype(np.uint16)
    for labels, ng in (([good.astype(np.int32)], 2), ([good[:19]], 2), ([good], 0), ([good], 65536), ([good, good], 2)):
        with pytest.raises(ValueError):
            R.moments_time_groups_flat(CUBES[:1], 1, labels, ng)
    with pytest.raises(ValueError):
        R.moments_time("sum")
    with pytest.raises(ValueError):
        R.moments_time("var", ddof=2)
    # a raster holding a k * k > 64 chunk: DCDF_ERR_UNSUPPORTED, as reduce_time
    a9 = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R9 = BD.build_raster(dc, a9, 20, 4, k=9)
    for call in (lambda: R9.moments_time_flat([[0, 4, 0, 20, 0, 20]], ALL),
                 lambda: R9.moments_time_groups_flat([[0, 4, 0, 20, 0, 20]], ALL, [np.zeros(4, dtype=np.uint16)], 1)):
        with pytest.raises(L.DcdfError) as e:
            call()
        assert e.value.code == -8
    R9.close()
