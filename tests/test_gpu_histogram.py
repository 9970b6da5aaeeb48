"""Value histograms (dcdf_raster_histogram_batch, EncodedRaster.histogram / histogram_flat, Variable.histogram) on the GPU.  Counts
are integers, so every comparison is exact, against the model of hist_model.py: the values widened to float64, the mask applied,
NaN dropped, numpy.histogram's rule for explicit edges."""
import ctypes as C

import numpy as np
import pytest

import hist_model as HM
import test_gpu_bulk_decode as BD
from test_gpu_reduce_time import SHAPE, TILE, CS, norm, source
from test_gpu_reduce_space import cube_masks, exact_raster

pytestmark = pytest.mark.gpu


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


def value_edges(rng, a, n=17):
    """A sorted sample of about n of the values themselves: ties on edges certainly occur."""
    x = np.asarray(a).astype(np.float64).ravel()
    u = np.unique(x[~np.isnan(x)])
    return np.unique(rng.choice(u, size=min(n, u.size), replace=False))


def with_inf(e):
    return np.concatenate([[-np.inf], e, [np.inf]])


def check(R, cube, edges, a, mask=None):
    """One cube through histogram_flat against the model on the array `a` the raster holds; returns (counts, stats)."""
    t0, t1, r0, r1, c0, c1 = norm(cube)
    bins = len(edges) - 1
    flat, off, ms, stats = R.histogram_flat([cube], edges, None if mask is None else [mask])
    assert flat.dtype == np.uint64 and flat.size == max(1, (t1 - t0) * bins) and off.tolist() == [0]
    got = HM.cube(flat, off, 0, t1 - t0, bins)
    np.testing.assert_array_equal(got, HM.histogram(a[t0:t1, r0:r1, c0:c1], edges, mask))
    return got, stats


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_windows_and_masks(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    rng = np.random.default_rng(71 + len(kind))
    edges = value_edges(rng, a)
    assert edges.size == 17
    #        whole raster         segments, the tile edge, 64-regions, odd columns   one instant             one cell
    cubes = [[0, T, 0, Rr, 0, Cc], [5, 17, 250, 264, 3, 264], [9, 10, 0, Rr, 0, Cc], [0, T, 261, 262, 130, 131]]
    saw_nan_only = False
    for cube in cubes:
        t0, t1, r0, r1, c0, c1 = norm(cube)
        _, _, _, dstats = R.decode_flat([cube], dtype=a.dtype)
        for mask in cube_masks(rng, a, cube):
            for e in (with_inf(edges), edges):
                got, stats = check(R, cube, e, a, mask)
                np.testing.assert_array_equal(stats, dstats)  # decode's numbers; the mask does not change them
                if mask is not None and mask.any() and e.size == 19 and not got.any():
                    saw_nan_only = True
    assert saw_nan_only == (kind[0] == "f")
    # with infinite ends every non-NaN cell is somewhere: bins + NaN = cells, and the sum over the bins is reduce_space's count
    cube = cubes[0]
    got, stats = check(R, cube, with_inf(edges), a)
    assert int(stats[0]) > 0 and int(stats[1]) == T * 8 * 8 and int(stats[2]) == 0  # bulk chunks and the corner chunk's walk
    nan = np.isnan(a.astype(np.float64)).reshape(T, -1).sum(1)
    np.testing.assert_array_equal(got.sum(1) + nan.astype(np.uint64), np.full(T, Rr * Cc, dtype=np.uint64))
    np.testing.assert_array_equal(got.sum(1).astype(np.float64), R.reduce_space("count")["count"])
    h = R.histogram(edges, 2, 19, window=(250, 264, 3, 264))
    np.testing.assert_array_equal(h, HM.histogram(a[2:19, 250:264, 3:264], edges))
    assert R.histogram(edges, 4, 4).shape == (0, 16)


def test_bin_counts(rasters):
    from dcdf_amd import _lib as L
    a, R = rasters("i32")
    rng = np.random.default_rng(256)
    cube = [2, 19, 100, 264, 60, 264]  # bulk units, the corner chunk's walk, three segments
    u = np.unique(a[2:19, 100:264, 60:264])
    assert u.size > 300
    for bins in (1, 2, 63, 64, 65, 256):
        edges = np.sort(rng.choice(u, size=bins + 1, replace=False)).astype(np.float64)
        got, _ = check(R, cube, edges, a)
        assert got.shape == (17, bins) and got.any()
    mask = rng.random((164, 204)) < 0.5
    check(R, cube, with_inf(np.sort(rng.choice(u, size=255, replace=False)).astype(np.float64)), a, mask)  # 256 bins, both ends open
    # 0 and 257 bins: DCDF_ERR_BAD_ARG from the entry point itself
    lib = L.lib()
    q = np.array([cube], dtype=np.uint32)
    out = np.zeros(17 * 257, dtype=np.uint64)
    off = np.zeros(1, dtype=np.uint64)
    e = np.arange(258, dtype=np.float64)
    for bins, rc in ((0, -1), (257, -1), (256, 0)):
        assert lib.dcdf_raster_histogram_batch(R._handle(), q.ctypes.data, 1, e.ctypes.data, bins, None, None, 0, out.ctypes.data, L.MEM_HOST,
                                               off.ctypes.data, None, None) == rc


def test_one_bin_for_everything_and_one_bin_per_cell(dc):
    """A 64 x 64 unit constant over all instants: every lane of every wave adds to one LDS counter.  Beside it a unit whose rows
    hold 64 different values: with an edge between any two, every cell of a row lands in a bin of its own."""
    from dcdf_amd import synth
    a = synth.cells(BD.SEED, 0, 8, 0, 128, 0, 128, np.int32)
    a[:, 0:64, 0:64] = 7
    a[:, 64:128, 0:64] = 3 * np.arange(64, dtype=np.int32)[None, None, :] - 90
    R = BD.build_raster(dc, a, 128, 8)
    const = [0, 8, 0, 64, 0, 64]
    got, stats = check(R, const, [-np.inf, 7.0, 8.0, np.inf], a)
    assert int(stats[0]) == 8 * 4096 and (got == np.array([0, 4096, 0], dtype=np.uint64)).all()
    got, _ = check(R, const, [7.0, 7.5], a)
    assert (got == 4096).all()
    got, _ = check(R, const, [6.0, 7.0], a)  # the last bin is closed
    assert (got == 4096).all()
    got, _ = check(R, const, [7.5, 8.0], a)
    assert not got.any()
    fine = 3.0 * np.arange(65) - 91.5
    got, _ = check(R, [0, 8, 64, 128, 0, 64], fine, a)
    assert got.shape == (8, 64) and (got == 64).all()
    mask = np.random.default_rng(7).random((128, 128)) < 0.5
    check(R, [0, 8, 0, 128, 0, 128], np.concatenate([fine, [200.0, np.inf]]), a, mask)  # both units and their neighbours, 66 bins
    R.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_leaves_translate_one_edge_array_apart(dc, dtype):
    """Two leaves with 0 and 25 fractional bits, |m| < 2^28: in float32 many stored integers share one value beyond 2^24, and one
    edge array becomes two threshold tables.  Edges are decoded values of both leaves."""
    a, chunks, EncodedRaster = exact_raster(dc, dtype, 77)
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    rng = np.random.default_rng(25)
    edges = np.unique(np.concatenate([value_edges(rng, a[:, :, :64], 9), value_edges(rng, a[:, :, 64:], 9)]))
    for e in (edges, with_inf(edges)):
        got, stats = check(R, [0, 8, 0, 64, 0, 128], e, a)
        assert int(stats[0]) == a.size and int(stats[1]) == 0
    mask = rng.random((59, 114)) < 0.5
    check(R, [2, 7, 5, 64, 9, 123], with_inf(edges), a, mask)
    R.close()


def test_62_fractional_bits_in_the_bulk_kernel(dc):
    """A float64 leaf with 62 fractional bits whose stored integers stay inside +-2^30: it takes the bulk kernel, and from_fixed's
    wrapped divisor makes the decoded value fall as the stored integer rises -- the kernel's bins run against its thresholds."""
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(6262)
    m = rng.integers(-(2 ** 28), 2 ** 28, size=(8, 64, 64))  # (stored: 2 m + 1)
    m[:, 10:20, 30:50] = 12345  # (a smooth patch: runs of equal bins)
    x = m / 2.0 ** 62
    (b,) = dc.build_batch([np.ascontiguousarray(x)], k=2, fractional_bits=62)
    assert not isinstance(b, Exception)
    R = EncodedRaster(x.shape, [b.data], tile=64, chunk_size=8)
    a = R.decode(dtype=np.float64)
    assert not np.isnan(a).any() and (a == -x).all() and np.unique(a).size > 1000  # the source negated: the divisor is -2^63
    edges = value_edges(rng, a)
    mask = rng.random((50, 61)) < 0.5
    for e in (edges, with_inf(edges), value_edges(rng, a, 66), with_inf(value_edges(rng, a, 255))):
        got, stats = check(R, [0, 8, 0, 64, 0, 64], e, a)
        assert int(stats[0]) == a.size and int(stats[1]) == 0 and got.any()
        check(R, [1, 7, 3, 53, 2, 63], e, a, mask)
    R.close()


def test_wide_values_take_the_walk(dc):
    """int64 near +-2^62 and float64 with 61 / 62 fractional bits: not narrow32, so the window walk and k_hist_fold run -- (double)n
    rounds here, and 62 bits decode against the stored order.  The model is applied to what decode returns."""
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(62)
    wide = (rng.integers(2 ** 62 - 2 ** 20, 2 ** 62, size=(4, 32, 32)) * rng.choice([-1, 1], size=(4, 32, 32))).astype(np.int64)
    (b,) = dc.build_batch([wide], k=2)
    assert not isinstance(b, Exception)
    Ri = EncodedRaster(wide.shape, [b.data], tile=32, chunk_size=4)
    chunks = []
    for fb in (61, 62):
        m = rng.integers(1, 2 ** 50, size=(4, 32, 32)) << rng.integers(0, 11, size=(4, 32, 32))
        x = (m * rng.choice([-1, 1], size=m.shape)) / 2.0 ** fb
        (b,) = dc.build_batch([np.ascontiguousarray(x)], k=2, fractional_bits=fb)
        assert not isinstance(b, Exception)
        chunks.append(b.data)
    Rf = EncodedRaster((4, 32, 64), chunks, tile=32, chunk_size=4)
    mask = rng.random((32, 64)) < 0.5
    for R, dtype, cols in ((Ri, np.int64, 32), (Rf, np.float64, 64)):
        a = R.decode(dtype=dtype)
        assert not np.isnan(a.astype(np.float64)).any()
        if dtype == np.int64:
            assert np.unique(a.astype(np.float64)).size < np.unique(a).size  # (double)n rounds: several n, one value
        edges = value_edges(rng, a, 13)
        for cube, m in (([0, 4, 0, 32, 0, cols], None), ([0, 4, 0, 32, 0, cols], mask[:, :cols]), ([1, 3, 7, 30, 5, cols - 3], None)):
            t0, t1, r0, r1, c0, c1 = cube
            for e in (edges, with_inf(edges)):
                got, stats = check(R, cube, e, a, m)
                assert int(stats[0]) == 0 and int(stats[1]) == (t1 - t0) * (r1 - r0) * (c1 - c0)
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
    assert any(t.chunk is None for t in R.tiles)
    dec = v.decode()
    edges = with_inf(value_edges(rng, dec, 15))
    np.testing.assert_array_equal(v.histogram(edges), HM.histogram(dec, edges))
    _, _, _, stats = R.histogram_flat([[0, T, 0, Rr, 0, Cc]], edges)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    # a mask that straddles elided and stored tiles, over a window that cuts both
    win = (7, T - 1, 3, Rr - 3, 10, 900)
    mask = np.zeros((Rr - 6, 890), dtype=bool)
    rr, cc = np.mgrid[0:Rr - 6, 0:890]
    mask[(rr - 14) ** 2 + ((cc - 60) / 3.0) ** 2 < 15 ** 2] = True  # an ellipse over the first leaves, elided ones among them
    mask[:, 400:] = rng.random((Rr - 6, 490)) < 0.3
    np.testing.assert_array_equal(v.histogram(edges[1:-1], *win, mask=mask),
                                  HM.histogram(dec[win[0]:win[1], win[2]:win[3], win[4]:win[5]], edges[1:-1], mask))
    only = np.zeros((Rr, Cc), dtype=bool)
    only[L:2 * L, L:2 * L] = True  # the elided tile alone: its cells in one bin, or nothing at its NaN instants
    got = v.histogram(edges, mask=only)
    np.testing.assert_array_equal(got, HM.histogram(dec, edges, only))
    valid = ~np.isnan(dec[:, L, L].astype(np.float64))
    assert ((got != 0).sum(1) == valid).all() and (got.sum(1) == valid * np.uint64((min(2 * L, Rr) - L) * L)).all()
    if np.dtype(dtype).kind == "f":
        assert not valid.all()
    none = v.histogram(edges, 4, 4)
    assert none.shape == (0, edges.size - 1) and none.dtype == np.uint64
    with pytest.raises(IndexError):
        v.histogram(edges, stop=T + 1)
    with pytest.raises(ValueError):
        v.histogram(edges, mask=np.ones((Rr, Cc + 1), dtype=bool))
    with pytest.raises(ValueError):
        v.histogram([1.0, 1.0])


def test_time_split_parts(dc):
    """One 64 x 64 unit over a chunk of 64 instants: too few units for the device, so bulk_parts cuts it in time and every part adds
    to its own instants' rows."""
    from dcdf_amd import synth
    a = synth.cells(BD.SEED, 0, 64, 0, 64, 0, 64, np.int32)
    R = BD.build_raster(dc, a, 64, 64)
    rng = np.random.default_rng(64)
    mask = rng.random((64, 64)) < 0.5
    edges = value_edges(rng, a)
    for cube, m in (([0, 64, 0, 64, 0, 64], None), ([0, 64, 0, 64, 0, 64], mask), ([3, 61, 1, 64, 2, 63], None)):
        t0, t1, r0, r1, c0, c1 = cube
        _, stats = check(R, cube, edges, a, m)
        assert int(stats[0]) == (t1 - t0) * (r1 - r0) * (c1 - c0)
    check(R, [0, 64, 0, 64, 0, 64], with_inf(np.unique(a)[:255].astype(np.float64)), a)  # 256 bins: four instants a flush
    R.close()


def test_slab_is_processed_in_parts(rasters, monkeypatch):
    """With a slab of 100 cells the corner piece's walk is cut into one instant a slab: the same arrays."""
    a, R = rasters("f32")
    T, Rr, Cc = SHAPE
    monkeypatch.setenv("K2R_REDUCE_SLAB_CELLS", "100")
    rng = np.random.default_rng(50)
    edges = with_inf(value_edges(rng, a))
    check(R, [0, T, 0, Rr, 0, Cc], edges, a)
    check(R, [5, 17, 250, 264, 3, 264], edges, a, rng.random((14, 261)) < 0.5)


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_batches_and_device_resident_form(rasters, kind):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    rng = np.random.default_rng(9)
    edges = value_edges(rng, a)
    bins = edges.size - 1
    # six cubes in one call, one of zero volume, one without rows, some reversed: the cubes one by one
    cubes = [[0, T, 0, Rr, 0, Cc], [17, 5, 264, 250, 3, 264], [6, 6, 0, 30, 0, 30], [2, 9, 40, 40, 0, 100], [9, 10, 0, Rr, 0, Cc], [0, T, 100, 101, 7, 8]]
    masks = [rng.random((abs(c[3] - c[2]), abs(c[5] - c[4]))) < 0.5 for c in cubes]
    masks[4] = None
    flat, off, _, stats = R.histogram_flat(cubes, edges, masks)
    _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
    np.testing.assert_array_equal(stats, dstats)
    nts = [abs(c[1] - c[0]) for c in cubes]
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(bins * np.array(nts))[:-1]]).astype(np.uint64))
    for q, c in enumerate(cubes):
        t0, t1, r0, r1, c0, c1 = norm(c)
        np.testing.assert_array_equal(HM.cube(flat, off, q, nts[q], bins), HM.histogram(a[t0:t1, r0:r1, c0:c1], edges, masks[q]))
    assert not HM.cube(flat, off, 3, 7, bins).any()  # instants but no rows: zeros
    # device-resident: results at odd offsets over a sentinel, the masks on the device at odd byte offsets
    parts = [np.ones(abs(c[3] - c[2]) * abs(c[5] - c[4]), dtype=np.uint8) if m is None else m.ravel().astype(np.uint8) * 3 for c, m in zip(cubes, masks)]
    moff = np.concatenate([[11], 11 + np.cumsum([p.size + 5 for p in parts])[:-1]]).astype(np.uint64)
    mbuf = DeviceBuffer(int(moff[-1]) + parts[-1].size + 16)
    for p, o in zip(parts, moff):
        if p.size:
            mbuf.write(int(o), p)
    vol = bins * np.array(nts, dtype=np.uint64)
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1]) + 7
    SENTINEL = np.uint64(0xABCDEF0123456789)
    buf = DeviceBuffer(total * 8)
    buf.write(0, np.full(total, SENTINEL, dtype=np.uint64))
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        inside[int(doff[q]):int(doff[q]) + int(vol[q])] = True
    for run in range(2):  # twice into the same buffer: the zeroing is the call's own
        ms, dvstats = R.histogram_flat(cubes, edges, masks=(mbuf.ptr, moff), out_device_ptr=buf.ptr, out_offset=doff)
        g = buf.read(0, total * 8, np.uint64)
        np.testing.assert_array_equal(dvstats, stats)
        for q in range(len(cubes)):
            o, n = int(doff[q]), int(vol[q])
            np.testing.assert_array_equal(g[o:o + n], flat[int(off[q]):int(off[q]) + n])
        assert (g[~inside] == SENTINEL).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's array
    buf.free()
    mbuf.free()


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_bins_equal_value_search_hits(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    rng = np.random.default_rng(33)
    edges = value_edges(rng, a)
    cube = [3, 18, 20, 264, 0, 250]
    got, _ = check(R, cube, edges, a)
    _, _, counts, _ = R.search_values_flat([cube], edges[-2], edges[-1])  # the last bin: closed on both sides
    assert int(got[:, -1].sum()) == int(counts[0]) > 0
    b = 7
    _, _, counts, _ = R.search_values_flat([cube], edges[b], np.nextafter(edges[b + 1], -np.inf))
    assert int(got[:, b].sum()) == int(counts[0]) > 0


def test_rejects_bad_input(dc, rasters):
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(64, dtype=np.uint64)
    off = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()
    mask = np.ones(16, dtype=np.uint8)
    good = np.array([-np.inf, 0.0, np.inf])

    def call(h, cubes, nq, edges, outp, offp, mem=L.MEM_HOST, m=None, mo=None, mmem=L.MEM_HOST, bins=None):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        e = None if edges is None else np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
        nb = (0 if e is None else e.size - 1) if bins is None else bins
        return lib.dcdf_raster_histogram_batch(h, None if q is None else q.ctypes.data, nq, None if e is None else e.ctypes.data, nb, m, mo, mmem,
                                               outp, mem, offp, stats.ctypes.data, C.byref(ms))

    o, f = out.ctypes.data, off.ctypes.data
    small = [[0, 3, 0, 2, 0, 2]]
    assert call(R._handle(), small, 1, good, o, f) == 0 and int(stats.sum()) == 12
    np.testing.assert_array_equal(out[:6].reshape(3, 2), HM.histogram(a[0:3, :2, :2], good))
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, good, o, f) == -5  # DCDF_ERR_BOUNDS
    for bad in ([0.0, np.nan, 1.0], [np.nan, 1.0], [0.0, 0.0], [1.0, 0.0], [0.0, 1.0, 1.0], [np.inf, np.inf]):
        assert call(R._handle(), small, 1, bad, o, f) == -1          # a NaN edge, edges not strictly increasing: DCDF_ERR_BAD_ARG
    assert call(R._handle(), small, 1, good, o, f, bins=0) == -1
    assert call(R._handle(), small, 1, np.arange(258.0), o, f) == -1  # 257 bins
    assert call(R._handle(), small, 1, None, o, f, bins=2) == -1      # NULL edges
    assert call(R._handle(), small, 1, good, o, f, m=mask.ctypes.data, mo=None) == -1   # a mask without offsets
    assert call(R._handle(), small, 1, good, o, f, m=mask.ctypes.data, mo=f, mmem=7) == -1
    assert call(R._handle(), small, 1, good, o, f, m=mask.ctypes.data, mo=f) == 0
    assert call(R._handle(), small, 1, good, o, f, mem=7) == -1
    assert call(None, small, 1, good, o, f) == -1                     # NULL arguments
    assert call(R._handle(), None, 1, good, o, f) == -1
    assert call(R._handle(), small, 1, good, None, f) == -1
    assert call(R._handle(), small, 1, good, o, None) == -1
    assert call(R._handle(), small, 0, good, o, f) == 0               # nq == 0 is fine
    # stats and kernel_ms may be NULL; a cube without instants writes nothing
    q = np.array([[2, 2, 0, 5, 0, 5]], dtype=np.uint32)
    out[:] = 99
    assert lib.dcdf_raster_histogram_batch(R._handle(), q.ctypes.data, 1, good.ctypes.data, 2, None, None, 0, o, L.MEM_HOST, f, None, None) == 0
    assert (out == 99).all()
    # k = 3, side 27: k * k <= 64, the window walk serves it
    a3 = synth.cells(BD.SEED, 0, 4, 0, 27, 0, 27, np.int32)
    R3 = BD.build_raster(dc, a3, 27, 4, k=3)
    e3 = value_edges(np.random.default_rng(3), a3, 9)
    _, st3 = check(R3, [0, 4, 0, 27, 0, 27], e3, a3)
    assert int(st3[0]) == 0 and int(st3[1]) == 4 * 27 * 27
    check(R3, [1, 3, 2, 25, 3, 20], e3, a3)
    R3.close()
    # k = 9: k * k = 81 > 64
    a9 = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R9 = BD.build_raster(dc, a9, 20, 4, k=9)
    with pytest.raises(L.DcdfError) as e:
        R9.histogram_flat([[0, 4, 0, 20, 0, 20]], good)
    assert e.value.code == -8
    R9.close()
