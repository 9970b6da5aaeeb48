"""Reduce over space (dcdf_raster_reduce_space_batch, EncodedRaster.reduce_space / reduce_space_flat, Variable.reduce_space) on the
GPU.  Every comparison is on bit patterns against the model of space_model.py: the values widened to float64, the mask applied,
NaNs dropped, then per instant math.fsum (the exact sum rounded once), fmin / fmax, the count and one division."""
import ctypes as C
import math

import numpy as np
import pytest

import space_model as SM
import test_gpu_bulk_decode as BD
from test_gpu_bulk_decode import assert_same
from test_gpu_reduce_time import SHAPE, TILE, CS, norm, source

pytestmark = pytest.mark.gpu
ALL = 31


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


def check_series(flat, off, q, ops, want, nt):
    """Cube q of a reduce_space_flat result equals the model's series `want` (all five; the call's are those of `ops`)."""
    got = SM.series(flat, off, q, ops, nt)
    assert list(got) == SM.names_of(ops)
    for n in got:
        assert_same(np.ascontiguousarray(got[n]), want[n])


def cube_masks(rng, a, cube):
    """None, a random mask of about half the cells, a mask that selects only cells that are NaN at every instant of the cube (for
    integers: nothing)."""
    t0, t1, r0, r1, c0, c1 = norm(cube)
    w = a[t0:t1, r0:r1, c0:c1]
    half = rng.random((r1 - r0, c1 - c0)) < 0.5
    nan = np.isnan(w).all(0) if w.dtype.kind == "f" else np.zeros((r1 - r0, c1 - c0), dtype=bool)
    return [None, half, nan]


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_windows_and_masks(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    rng = np.random.default_rng(41 + len(kind))
    #        whole raster         segments, the tile edge, 64-regions, odd columns   one instant             one cell
    cubes = [[0, T, 0, Rr, 0, Cc], [5, 17, 250, 264, 3, 264], [9, 10, 0, Rr, 0, Cc], [0, T, 261, 262, 130, 131]]
    saw_nan_only = False
    for cube in cubes:
        t0, t1, r0, r1, c0, c1 = norm(cube)
        _, _, _, dstats = R.decode_flat([cube], dtype=a.dtype)
        for mask in cube_masks(rng, a, cube):
            want = SM.reduce_space(a[t0:t1, r0:r1, c0:c1], mask)
            if mask is not None and mask.any() and (want["count"] == 0).all():
                saw_nan_only = True
            for ops in (ALL, 1, 16):
                flat, off, ms, stats = R.reduce_space_flat([cube], ops, None if mask is None else [mask])
                assert ms > 0 and flat.size == bin(ops).count("1") * (t1 - t0) and off.tolist() == [0]
                check_series(flat, off, 0, ops, want, t1 - t0)
                np.testing.assert_array_equal(stats, dstats)  # (the mask does not change them)
    assert saw_nan_only == (kind[0] == "f")
    _, _, _, stats = R.reduce_space_flat([cubes[0]], ALL)
    assert int(stats[0]) > 0 and int(stats[1]) == T * 8 * 8 and int(stats[2]) == 0  # bulk chunks and the corner chunk's walk
    d = R.reduce_space(("max", "count"), 2, 19, window=(250, 264, 3, 264))
    want = SM.reduce_space(a[2:19, 250:264, 3:264])
    assert list(d) == ["max", "count"]
    assert_same(np.ascontiguousarray(d["max"]), want["max"])
    assert_same(np.ascontiguousarray(d["count"]), want["count"])


def exact_raster(dc, dtype, seed):
    """[8, 64, 128], tile 64, chunk_size 8: two leaves built apart with 0 and 25 fractional bits, values m / 2^bits with |m| < 2^28
    -- stored integers inside +-2^30, so both take the bulk kernel -- whose magnitudes mix in every instant's sum."""
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(seed)
    parts, chunks = [], []
    for fb in (0, 25):
        m = rng.integers(-(2 ** 28) + 1, 2 ** 28, size=(8, 64, 64))
        m[m == 0] = 1
        x = (m / 2.0 ** fb).astype(dtype)
        parts.append(x)
        (b,) = dc.build_batch([np.ascontiguousarray(x)], k=2, fractional_bits=fb)
        assert not isinstance(b, Exception)
        chunks.append(b.data)
    return np.concatenate(parts, axis=2), chunks, EncodedRaster


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sum_is_exact_not_ordered(dc, dtype):
    a, chunks, EncodedRaster = exact_raster(dc, dtype, 2025)
    x = a.astype(np.float64)
    exact = np.array([math.fsum(x[t].ravel().tolist()) for t in range(8)])
    # the condition is the model's: orders and cuts a kernel might have taken give other bits
    seq = np.zeros(8)
    for t in range(8):
        s = 0.0
        for v in x[t].ravel().tolist():
            s += v
        seq[t] = s
    assert (seq != exact).any(), "the row-major sequential sum equals the exact one: the input proves nothing"
    assert (x.reshape(8, -1).sum(1) != exact).any(), "np.sum equals the exact sum: the input proves nothing"
    # Partial sums rounded, then added.  With one partial per leaf this cannot differ: a leaf's own sum is exact in a double (one
    # scale, below 2^53), and one addition of two exact partials IS the correctly rounded sum.  The cut that shows it is finer:
    # every leaf's rows summed apart (exactly), the 128 partials added in order.
    leaves = np.array([math.fsum(x[t, :, :64].ravel().tolist()) + math.fsum(x[t, :, 64:].ravel().tolist()) for t in range(8)])
    assert (leaves == exact).all()
    rows = np.zeros(8)
    for t in range(8):
        for leaf in (x[t, :, :64], x[t, :, 64:]):
            for r in range(64):
                rows[t] += math.fsum(leaf[r].tolist())
    assert (rows != exact).any(), "per-row sums rounded, then added, equal the exact sum: the input proves nothing"
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    cube = [[0, 8, 0, 64, 0, 128]]
    flat, off, _, stats = R.reduce_space_flat(cube, ("sum",))
    assert int(stats[0]) == a.size and int(stats[1]) == 0
    assert_same(flat, exact)
    want = SM.reduce_space(a)
    flat, off, _, _ = R.reduce_space_flat(cube, ALL)
    check_series(flat, off, 0, ALL, want, 8)
    sub = [2, 7, 5, 64, 9, 123]
    mask = np.random.default_rng(5).random((59, 114)) < 0.5
    flat, off, _, _ = R.reduce_space_flat([sub], ("sum", "mean"), [mask])
    check_series(flat, off, 0, 20, SM.reduce_space(a[2:7, 5:64, 9:123], mask), 5)
    R.close()


def test_wide_values_take_the_walk(dc):
    """int64 near +-2^62 and float64 with 61 / 62 fractional bits: not narrow32, so the window walk and k_space_fold run -- sums
    beyond 64 bits in the records, and the negative divisor of 62 fractional bits.  The model is applied to what decode returns
    (with 62 bits that is the source negated: from_fixed's wrapped divisor)."""
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(62)
    wide = (rng.integers(2 ** 62 - 2 ** 20, 2 ** 62, size=(4, 32, 32)) * rng.choice([-1, 1], size=(4, 32, 32))).astype(np.int64)
    wide[:, :, :16] = np.abs(wide[:, :, :16])  # (half the cells of one sign: the sum passes 2^64 by far)
    (b,) = dc.build_batch([wide], k=2)
    assert not isinstance(b, Exception)
    Ri = EncodedRaster(wide.shape, [b.data], tile=32, chunk_size=4)
    chunks = []
    for fb in (61, 62):
        m = rng.integers(1, 2 ** 50, size=(4, 32, 32)) << rng.integers(0, 11, size=(4, 32, 32))  # 50 significant bits below 2^60, magnitudes mixed
        x = (m * rng.choice([-1, 1], size=m.shape)) / 2.0 ** fb
        (b,) = dc.build_batch([np.ascontiguousarray(x)], k=2, fractional_bits=fb)
        assert not isinstance(b, Exception)
        chunks.append(b.data)
    Rf = EncodedRaster((4, 32, 64), chunks, tile=32, chunk_size=4)
    mask = rng.random((32, 64)) < 0.5
    for R, dtype, cols in ((Ri, np.int64, 32), (Rf, np.float64, 64)):
        a = R.decode(dtype=dtype)
        assert not np.isnan(a.astype(np.float64)).any()
        for cube, m in (([0, 4, 0, 32, 0, cols], None), ([0, 4, 0, 32, 0, cols], mask[:, :cols]), ([1, 3, 7, 30, 5, cols - 3], None)):
            t0, t1, r0, r1, c0, c1 = cube
            flat, off, _, stats = R.reduce_space_flat([cube], ALL, None if m is None else [m])
            assert int(stats[0]) == 0 and int(stats[1]) == (t1 - t0) * (r1 - r0) * (c1 - c0)
            check_series(flat, off, 0, ALL, SM.reduce_space(a[t0:t1, r0:r1, c0:c1], m), t1 - t0)
        R.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_stored_variable_with_elided_tiles(dtype):
    """A Dataset.append'ed variable: uniform tiles elided, a nested level, offset leaves, a short last segment; the float one has an
    elided tile that is NaN at some instants only."""
    import test_gpu_stored_raster as SR
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    levels, shape = [1, 6, 5], (40, 40, 2112)
    L = 1 << levels[-1]
    rng = np.random.default_rng(sum(shape))
    a = SR.var_data(rng, shape, dtype, L)
    if np.dtype(dtype).kind == "f":
        a[5:9, L:2 * L, L:2 * L] = np.nan
        a[33, L:2 * L, L:2 * L] = np.nan
    v = SR.make_var(dataset, a, levels, 32)
    T, Rr, Cc = shape
    R = v.raster()
    assert any(t.chunk is None for t in R.tiles) and any(t.chunk is not None and (t.row0 or t.col0) for t in R.tiles)
    if np.dtype(dtype).kind == "f":
        assert any(t.chunk is None and (np.asarray(t.values) == 0).any() and (np.asarray(t.values) != 0).any() for t in R.tiles)
    dec = v.decode()
    np.testing.assert_array_equal(dec, a)
    got = v.reduce_space(SM.NAMES)
    want = SM.reduce_space(dec)
    assert list(got) == list(SM.NAMES)
    for n in SM.NAMES:
        assert_same(np.ascontiguousarray(got[n]), want[n])
    # a mask that straddles elided and stored tiles, over a window that cuts both
    win = (7, T - 1, 3, Rr - 3, 10, 900)
    mask = np.zeros((Rr - 6, 890), dtype=bool)
    rr, cc = np.mgrid[0:Rr - 6, 0:890]
    mask[(rr - 14) ** 2 + ((cc - 60) / 3.0) ** 2 < 15 ** 2] = True  # an ellipse over the first leaves, elided ones among them
    mask[:, 400:] = rng.random((Rr - 6, 490)) < 0.3
    got = v.reduce_space(("mean", "max", "count"), *win, mask=mask)
    want = SM.reduce_space(dec[win[0]:win[1], win[2]:win[3], win[4]:win[5]], mask)
    assert list(got) == ["max", "count", "mean"]
    for n in got:
        assert_same(np.ascontiguousarray(got[n]), want[n])
    only = np.zeros((Rr, Cc), dtype=bool)
    only[L:2 * L, L:2 * L] = True  # the elided tile alone: value x cells, or nothing at its NaN instants
    got = v.reduce_space(ALL, mask=only)
    want = SM.reduce_space(dec, only)
    for n in SM.NAMES:
        assert_same(np.ascontiguousarray(got[n]), want[n])
    assert list(v.reduce_space()) == ["mean"]
    _, _, _, stats = R.reduce_space_flat([[0, T, 0, Rr, 0, Cc]], ALL)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    none = v.reduce_space(("count", "min"), 4, 4)
    assert list(none) == ["min", "count"] and none["count"].shape == (0,) and none["min"].dtype == np.float64
    with pytest.raises(IndexError):
        v.reduce_space(stop=T + 1)
    with pytest.raises(ValueError):
        v.reduce_space(mask=np.ones((Rr, Cc + 1), dtype=bool))


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_single_cell_equals_fill_cell_and_batches(rasters, kind):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    cells = [[0, T, 17, 23], [3, 19, 200, 5], [0, T, 260, 261], [2, 11, 100, 100]]  # NaN at every instant, at all but one, the corner chunk
    series, soff, _ = R.fill_cells_flat(cells, dtype=a.dtype)
    cubes = [[s, e, r, r + 1, c, c + 1] for s, e, r, c in cells]
    flat, off, _, _ = R.reduce_space_flat(cubes, ("min", "max", "sum"))
    for q, (s, e, r, c) in enumerate(cells):
        x = series[int(soff[q]):int(soff[q]) + e - s].astype(np.float64)
        got = SM.series(flat, off, q, 7, e - s)
        nan = np.isnan(x)
        assert_same(np.ascontiguousarray(got["min"]), np.where(nan, np.nan, x))
        assert_same(np.ascontiguousarray(got["max"]), np.where(nan, np.nan, x))
        assert_same(np.ascontiguousarray(got["sum"]), np.where(nan, 0.0, x))
    # six cubes in one call, one of zero volume, one without rows, some reversed: the cubes one by one
    rng = np.random.default_rng(9)
    cubes = [[0, T, 0, Rr, 0, Cc], [17, 5, 264, 250, 3, 264], [6, 6, 0, 30, 0, 30], [2, 9, 40, 40, 0, 100], [9, 10, 0, Rr, 0, Cc], [0, T, 100, 101, 7, 8]]
    masks = [rng.random((abs(c[3] - c[2]), abs(c[5] - c[4]))) < 0.5 for c in cubes]
    masks[4] = None
    ops = 27  # min, max, count, mean: the sum is formed for the mean alone
    flat, off, _, stats = R.reduce_space_flat(cubes, ops, masks)
    _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
    np.testing.assert_array_equal(stats, dstats)
    nts = [abs(c[1] - c[0]) for c in cubes]
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(4 * np.array(nts))[:-1]]).astype(np.uint64))
    for q, c in enumerate(cubes):
        if nts[q] == 0:
            continue
        f1, o1, _, _ = R.reduce_space_flat([c], ops, [masks[q]])
        assert_same(flat[int(off[q]):int(off[q]) + 4 * nts[q]], f1[:4 * nts[q]])
        t0, t1, r0, r1, c0, c1 = norm(c)
        check_series(flat, off, q, ops, SM.reduce_space(a[t0:t1, r0:r1, c0:c1], masks[q]), nts[q])
    w = SM.series(flat, off, 3, ops, 7)  # instants but no rows: the "none" values
    assert (w["count"] == 0).all() and np.isnan(w["min"]).all() and np.isnan(w["mean"]).all()
    # device-resident: results at odd offsets over a sentinel, the masks on the device too
    parts = [np.ones(abs(c[3] - c[2]) * abs(c[5] - c[4]), dtype=np.uint8) if m is None else m.ravel().astype(np.uint8) * 3 for c, m in zip(cubes, masks)]
    moff = np.concatenate([[11], 11 + np.cumsum([p.size + 5 for p in parts])[:-1]]).astype(np.uint64)
    mbuf = DeviceBuffer(int(moff[-1]) + parts[-1].size + 16)
    for p, o in zip(parts, moff):
        if p.size:
            mbuf.write(int(o), p)
    vol = 4 * np.array(nts, dtype=np.uint64)
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1]) + 7
    buf = DeviceBuffer(total * 8)
    buf.write(0, np.full(total, -77.25, dtype=np.float64))
    ms, dvstats = R.reduce_space_flat(cubes, ops, masks=(mbuf.ptr, moff), out_device_ptr=buf.ptr, out_offset=doff)
    g = buf.read(0, total * 8, np.float64)
    buf.free()
    mbuf.free()
    np.testing.assert_array_equal(dvstats, stats)
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        o, n = int(doff[q]), int(vol[q])
        inside[o:o + n] = True
        assert_same(g[o:o + n], flat[int(off[q]):int(off[q]) + n])
    assert (g[~inside] == -77.25).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's series


def test_time_split_parts(dc):
    """One 64 x 64 unit over a chunk of 64 instants: too few units for the device, so bulk_parts cuts it in time and every part
    writes its own instants' records."""
    from dcdf_amd import synth
    a = synth.cells(BD.SEED, 0, 64, 0, 64, 0, 64, np.int32)
    R = BD.build_raster(dc, a, 64, 64)
    mask = np.random.default_rng(64).random((64, 64)) < 0.5
    for cube, m in (([0, 64, 0, 64, 0, 64], None), ([0, 64, 0, 64, 0, 64], mask), ([3, 61, 1, 64, 2, 63], None)):
        t0, t1, r0, r1, c0, c1 = cube
        flat, off, _, stats = R.reduce_space_flat([cube], ALL, None if m is None else [m])
        assert int(stats[0]) == (t1 - t0) * (r1 - r0) * (c1 - c0)
        check_series(flat, off, 0, ALL, SM.reduce_space(a[t0:t1, r0:r1, c0:c1], m), t1 - t0)
    R.close()


def test_record_scratch_and_slab_are_processed_in_batches(rasters, monkeypatch):
    """With room for 50 records and a slab of 100 cells the whole-raster cube (25 units and the corner piece per segment) is cut in
    time into many batches, and the corner piece's walk into one instant a slab: the same series."""
    a, R = rasters("f32")
    T, Rr, Cc = SHAPE
    monkeypatch.setenv("K2R_SPACE_RECORDS", "50")
    monkeypatch.setenv("K2R_REDUCE_SLAB_CELLS", "100")
    cubes = [[0, T, 0, Rr, 0, Cc], [5, 17, 250, 264, 3, 264]]
    mask = np.random.default_rng(50).random((14, 261)) < 0.5
    flat, off, _, stats = R.reduce_space_flat(cubes, ALL, [None, mask])
    _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
    np.testing.assert_array_equal(stats, dstats)
    check_series(flat, off, 0, ALL, SM.reduce_space(a), T)
    check_series(flat, off, 1, ALL, SM.reduce_space(a[5:17, 250:264, 3:264], mask), 12)


def test_rejects_bad_input(dc, rasters):
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(64, dtype=np.float64)
    off = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()
    mask = np.ones(16, dtype=np.uint8)

    def call(h, cubes, nq, ops, outp, offp, mem=L.MEM_HOST, m=None, mo=None, mmem=L.MEM_HOST):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        return lib.dcdf_raster_reduce_space_batch(h, None if q is None else q.ctypes.data, nq, ops, m, mo, mmem, outp, mem, offp, stats.ctypes.data, C.byref(ms))

    o, f = out.ctypes.data, off.ctypes.data
    small = [[0, 3, 0, 2, 0, 2]]
    assert call(R._handle(), small, 1, 4 | 8, o, f) == 0 and int(stats.sum()) == 12
    np.testing.assert_array_equal(out[:3], a[0:3, :2, :2].sum((1, 2)))
    np.testing.assert_array_equal(out[3:6], [4, 4, 4])
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, 1, o, f) == -5  # DCDF_ERR_BOUNDS
    for ops in (0, 32, 33, 1 << 20):
        assert call(R._handle(), small, 1, ops, o, f) == -1          # no statistic, or a bit above 16: DCDF_ERR_BAD_ARG
    assert call(R._handle(), small, 1, 1, o, f, m=mask.ctypes.data, mo=None) == -1   # a mask without offsets
    assert call(R._handle(), small, 1, 1, o, f, m=mask.ctypes.data, mo=f, mmem=7) == -1
    assert call(R._handle(), small, 1, 1, o, f, m=mask.ctypes.data, mo=f) == 0
    assert call(R._handle(), small, 1, 1, o, f, mem=7) == -1
    assert call(None, small, 1, 1, o, f) == -1                       # NULL arguments
    assert call(R._handle(), None, 1, 1, o, f) == -1
    assert call(R._handle(), small, 1, 1, None, f) == -1
    assert call(R._handle(), small, 1, 1, o, None) == -1
    assert call(R._handle(), small, 0, 1, o, f) == 0                 # nq == 0 is fine
    # stats and kernel_ms may be NULL; a cube without instants writes nothing
    q = np.array([[2, 2, 0, 5, 0, 5]], dtype=np.uint32)
    out[:] = -1
    assert lib.dcdf_raster_reduce_space_batch(R._handle(), q.ctypes.data, 1, 31, None, None, 0, o, L.MEM_HOST, f, None, None) == 0
    assert (out == -1).all()
    with pytest.raises(ValueError):
        R.reduce_space_flat(small, 0)
    # k = 3, side 27: k * k <= 64, the window walk serves it
    a3 = synth.cells(BD.SEED, 0, 4, 0, 27, 0, 27, np.int32)
    R3 = BD.build_raster(dc, a3, 27, 4, k=3)
    flat, off3, _, st3 = R3.reduce_space_flat([[0, 4, 0, 27, 0, 27], [1, 3, 2, 25, 3, 20]], ALL)
    assert int(st3[0]) == 0 and int(st3[1]) == 4 * 27 * 27 + 2 * 23 * 17
    check_series(flat, off3, 0, ALL, SM.reduce_space(a3), 4)
    check_series(flat, off3, 1, ALL, SM.reduce_space(a3[1:3, 2:25, 3:20]), 2)
    R3.close()
    # k = 9: k * k = 81 > 64
    a9 = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R9 = BD.build_raster(dc, a9, 20, 4, k=9)
    with pytest.raises(L.DcdfError) as e:
        R9.reduce_space_flat([[0, 4, 0, 20, 0, 20]], ALL)
    assert e.value.code == -8
    R9.close()
