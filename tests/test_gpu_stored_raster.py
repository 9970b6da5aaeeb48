"""Rasters over stored Superchunks (dcdf_raster_create_tiles, Variable.raster()): elided leaves, padded extents, nested levels,
chunks that span several leaves, time segments with a partial tail -- fill_window, get, fill_cell, integer and value search, all
on the device, against the source array, the Variable methods and a model of Superchunk::search."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")


@pytest.fixture(scope="module")
def ds():
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dataset


def make_var(ds, data, k2_levels, chunk_size, span_size=2, round=False, fractional_bits=0):
    T, R, Cc = data.shape
    t = ds.Coordinate.time("t", 0, np.timedelta64(100, "s"))
    y = ds.Coordinate.range("y", 0, 1, R, np.float64)
    x = ds.Coordinate.range("x", 0, 1, Cc, np.float64)
    d = ds.Dataset.new([t, y, x], [R, Cc], ds.Resolver())
    d = d.add_variable("v", span_size, chunk_size, k2_levels, round, fractional_bits, dtype=data.dtype.type)
    d = d.append("v", data[:T // 2])  # two appends: the tail segment is re-encoded (dataset.rs:171-189)
    d = d.append("v", data[T // 2:])
    return d.v


def var_data(rng, shape, dtype, leaf, bits=2):
    """Random values with leaves uniform at every instant (elided: constant, per-instant, all-NaN, the padded bottom row) -- no
    leaf uniform at only some instants, so the integer search has no reference quirk to reproduce and equals brute force."""
    T, R, Cc = shape
    L = leaf
    m = rng.integers(-400, 400, size=shape)
    m[:, :L, :L] = 9
    m[:, L:2 * L, L:2 * L] = rng.integers(-400, 400, size=(T, 1, 1))
    m[:, R // L * L:, :2 * L] = -3
    if np.dtype(dtype).kind == "f":
        x = (m / 2.0 ** bits).astype(dtype)
        x[rng.random(shape) < 0.03] = np.nan
        x[:, :L, :L] = 9.0
        x[:, L:2 * L, L:2 * L] = m[:, L:2 * L, L:2 * L] / 2.0 ** bits
        x[:, R // L * L:, :2 * L] = -3 / 2.0 ** bits  # (a NaN first in an otherwise uniform tile is lost by min_max_float: keep them out)
        x[:, L:2 * L, 0:L] = np.nan  # an all-NaN leaf
        return x
    return m.astype(dtype)


def rand_cubes(rng, shape, n, max_ext=(12, 24, 24)):
    T, R, Cc = shape
    t0, r0, c0 = rng.integers(0, T, n), rng.integers(0, R, n), rng.integers(0, Cc, n)
    t1 = np.minimum(T, t0 + rng.integers(1, max_ext[0] + 1, n))
    r1 = np.minimum(R, r0 + rng.integers(1, max_ext[1] + 1, n))
    c1 = np.minimum(Cc, c0 + rng.integers(1, max_ext[2] + 1, n))
    return np.stack([t0, t1, r0, r1, c0, c1], axis=1).astype(np.uint32)


def oracle(w, lo, hi, origin):
    w64 = np.asarray(w).astype(np.float64)
    return np.argwhere((w64 >= min(lo, hi)) & (w64 <= max(lo, hi))).astype(np.int64) + np.array(origin, dtype=np.int64)


def sort3(t):
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def check_order(t, cs, leaf):
    """Order contract: by piece (segment, leaf row, leaf col), sorted inside a piece."""
    t = np.asarray(t, dtype=np.int64)
    if len(t) < 2:
        return
    key = np.stack([t[:, 0] // cs, t[:, 1] // leaf, t[:, 2] // leaf, t[:, 0], t[:, 1], t[:, 2]], axis=1)
    d = np.diff(key, axis=0)
    first_nz = np.argmax(d != 0, axis=1)
    assert (d[np.arange(len(d)), first_nz] > 0).all()


def device_buf(nbytes):
    from dcdf_amd.encoder import DeviceBuffer
    return DeviceBuffer(max(16, nbytes))


def check_queries(v, a, R, rng, n_cubes=1500, n_points=3000, n_series=1000):
    dt = np.dtype(v.dtype)
    cubes = rand_cubes(rng, a.shape, n_cubes)
    flat, off, _ = R.fill_windows_flat(cubes, dtype=dt)
    for q, c in enumerate(cubes):
        t0, t1, r0, r1, c0, c1 = (int(x) for x in c)
        w = flat[int(off[q]):int(off[q]) + (t1 - t0) * (r1 - r0) * (c1 - c0)].reshape(t1 - t0, r1 - r0, c1 - c0)
        np.testing.assert_array_equal(w, a[t0:t1, r0:r1, c0:c1])
    for c in cubes[:10]:
        np.testing.assert_array_equal(v.window(*(int(x) for x in c)), a[c[0]:c[1], c[2]:c[3], c[4]:c[5]])
    # device output, windows at non-dense offsets
    sub = cubes[:300]
    vol = ((sub[:, 1] - sub[:, 0]) * (sub[:, 3] - sub[:, 2]) * (sub[:, 5] - sub[:, 4])).astype(np.uint64)
    doff = np.concatenate([[0], np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    buf = device_buf(int(doff[-1] + vol[-1]) * dt.itemsize)
    R.fill_windows_flat(sub, dtype=dt, out_device_ptr=buf.ptr, out_offset=doff)
    got = buf.read(0, int(doff[-1] + vol[-1]) * dt.itemsize, dt)
    for q, c in enumerate(sub):
        np.testing.assert_array_equal(got[int(doff[q]):int(doff[q] + vol[q])], a[c[0]:c[1], c[2]:c[3], c[4]:c[5]].ravel())
    buf.free()
    # points
    T, Rr, Cc = a.shape
    pts = np.stack([rng.integers(0, T, n_points), rng.integers(0, Rr, n_points), rng.integers(0, Cc, n_points)], axis=1).astype(np.uint32)
    vals, _ = R.get_flat(pts, dtype=dt)
    np.testing.assert_array_equal(vals, a[pts[:, 0], pts[:, 1], pts[:, 2]])
    for p in pts[:5]:
        np.testing.assert_array_equal(v.get(*(int(x) for x in p)), a[tuple(p)])
    buf = device_buf(n_points * dt.itemsize)
    R.get_flat(pts, dtype=dt, out_device_ptr=buf.ptr)
    np.testing.assert_array_equal(buf.read(0, n_points * dt.itemsize, dt), a[pts[:, 0], pts[:, 1], pts[:, 2]])
    buf.free()
    # series (some reversed, some empty)
    s0, s1 = rng.integers(0, T + 1, n_series), rng.integers(0, T + 1, n_series)
    cells = np.stack([s0, s1, rng.integers(0, Rr, n_series), rng.integers(0, Cc, n_series)], axis=1).astype(np.uint32)
    flat, off, _ = R.fill_cells_flat(cells, dtype=dt)
    for i, (x0, x1, r, c) in enumerate(cells.astype(int)):
        lo, hi = min(x0, x1), max(x0, x1)
        np.testing.assert_array_equal(flat[int(off[i]):int(off[i]) + hi - lo], a[lo:hi, r, c])
    for x0, x1, r, c in cells[:5].astype(int):
        np.testing.assert_array_equal(v.cell(min(x0, x1), max(x0, x1), r, c), a[min(x0, x1):max(x0, x1), r, c])
    ln = np.abs(cells[:, 1].astype(np.int64) - cells[:, 0])
    doff = np.concatenate([[0], np.cumsum(ln + 1)[:-1]]).astype(np.uint64)
    buf = device_buf(int(doff[-1] + ln[-1] + 1) * dt.itemsize)
    R.fill_cells_flat(cells, dtype=dt, out_device_ptr=buf.ptr, out_offset=doff)
    got = buf.read(0, int(doff[-1] + ln[-1] + 1) * dt.itemsize, dt)
    for i, (x0, x1, r, c) in enumerate(cells.astype(int)):
        lo, hi = min(x0, x1), max(x0, x1)
        np.testing.assert_array_equal(got[int(doff[i]):int(doff[i]) + hi - lo], a[lo:hi, r, c])
    buf.free()


def check_searches(v, a, R, rng, n_cubes=150):
    cubes = rand_cubes(rng, a.shape, n_cubes, (8, 40, 40))
    fin = a[np.isfinite(a)] if a.dtype.kind == "f" else a
    med = float(np.median(fin))
    bounds = [(med - 20, med + 20), (-INF, INF), (-1.0, 1.0), (9.0, 9.0), (2.5, -INF), (1e9, 2e9)]
    if a.dtype.kind == "f":
        bounds += [(-0.0, 0.0), (-3 / 4, 1 / 4)]
    for lo, hi in bounds:
        trip, offs, counts, _ = R.search_values_flat(cubes, lo, hi)
        for q, c in enumerate(cubes):
            t0, t1, r0, r1, c0, c1 = (int(x) for x in c)
            got = trip[int(offs[q]):int(offs[q]) + int(counts[q])].astype(np.int64)
            check_order(got, R.chunk_size, R.tile)
            want = oracle(a[t0:t1, r0:r1, c0:c1], lo, hi, (t0, r0, c0))
            assert np.array_equal(sort3(got), want), (lo, hi, c)
            if q < 4:
                assert np.array_equal(sort3(got), v.search_values(t0, t1, r0, r1, c0, c1, lo, hi))
    if a.dtype.kind == "i":
        for lo, hi in [(int(med) - 30, int(med) + 30), (9, 9), (-3, -3), (-10 ** 6, 10 ** 6), (50, -50), (401, 900)]:
            trip, offs, counts, _ = R.search_flat(cubes, np.full(len(cubes), lo), np.full(len(cubes), hi))
            for q, c in enumerate(cubes):
                t0, t1, r0, r1, c0, c1 = (int(x) for x in c)
                got = trip[int(offs[q]):int(offs[q]) + int(counts[q])].astype(np.int64)
                check_order(got, R.chunk_size, R.tile)
                assert np.array_equal(sort3(got), oracle(a[t0:t1, r0:r1, c0:c1], lo, hi, (t0, r0, c0))), (lo, hi, c)


CASES = [  # dtype, shape, k2_levels, chunk_size, round bits (None: no rounding)
    (np.int32, (23, 40, 37), [2, 4], 7, None),
    (np.int64, (17, 36, 64), [1, 2, 3], 5, None),
    (np.float32, (19, 40, 40), [2, 4], 6, None),
    (np.float64, (15, 33, 40), [1, 3, 2], 4, None),   # a top-level chunk of 1 x 8 spans two leaves of 4
    (np.float32, (13, 32, 32), [1, 4], 5, 2),         # round=True
]


@pytest.mark.parametrize("dtype,shape,levels,cs,rbits", CASES, ids=[c[0].__name__ + "_" + "x".join(map(str, c[2])) for c in CASES])
def test_variable_raster(ds, dtype, shape, levels, cs, rbits):
    rng = np.random.default_rng(sum(shape) + len(levels))
    a = var_data(rng, shape, dtype, 1 << levels[-1])
    v = make_var(ds, a, levels, cs, round=rbits is not None, fractional_bits=rbits or 0)
    R = v.raster()
    assert v.raster() is R and R.tile == 1 << levels[-1] and R.nseg == -(-shape[0] // cs) >= 3
    assert any(t.chunk is None for t in R.tiles) and any(t.chunk is not None for t in R.tiles)
    if levels == [1, 3, 2]:
        assert any(t.col0 for t in R.tiles)
    check_queries(v, a, R, rng)
    check_searches(v, a, R, rng)


def test_has_cells_prunes_quirk_pieces(ds):
    """A forced quirk chunk (a single-node uniform log over a multi-node snapshot) with its TRUE per-instant (min, max): the tiled
    raster's search equals Superchunk::search -- has_cells over the piece's instants, then the chunk's own (quirky) search -- and
    for some bounds that differs from the unpruned search of a plain raster."""
    import dcdf_amd
    from dcdf_amd import _lib as L
    from dcdf_amd.raster import EncodedRaster, RasterTile
    rng = np.random.default_rng(64)
    s64 = rng.integers(0, 40, size=(64, 64)).astype(np.int64)
    differs = 0
    for tv in (55, 17, -3):
        arr = np.stack([s64, np.zeros((64, 64), dtype=np.int64) + tv, s64 + 1])
        data = O.chunk_build_forced(arr, 2, 3)
        ch, oc = dcdf_amd.Chunk(data), O.Chunk(data)
        mm = np.stack([arr.min(axis=(1, 2)), arr.max(axis=(1, 2))], axis=1)
        tiled = EncodedRaster.from_tiles((3, 64, 64), [RasterTile(ch, 0, 0, None, mm, L.DCDF_I64, 0, True)], 64, 3)
        plain = EncodedRaster((3, 64, 64), [ch], tile=64, chunk_size=3)
        for lo, hi in [(-10, 100), (0, 39), (10, 20), (tv, tv), (tv - 5, tv + 5), (40, 60), (-8, -1), (16, 18), (39, 56)]:
            cubes = [(0, 3, 0, 64, 0, 64), (1, 2, 5, 40, 17, 64), (1, 3, 30, 34, 0, 7), (1, 2, 0, 64, 0, 64)]
            trip, offs, counts, _ = tiled.search_flat(cubes, [lo] * 4, [hi] * 4)
            ptrip, poffs, pcounts, _ = plain.search_flat(cubes, [lo] * 4, [hi] * 4)
            for q, cube in enumerate(cubes):
                live = any(hi >= mm[t, 0] and lo <= mm[t, 1] for t in range(cube[0], cube[1]))
                want = sort3(oc.search(*cube, lo, hi)) if live else np.zeros((0, 3), dtype=np.int64)
                got = trip[int(offs[q]):int(offs[q]) + int(counts[q])].astype(np.int64)
                assert np.array_equal(got, want), (tv, lo, hi, cube)
                unpruned = ptrip[int(poffs[q]):int(poffs[q]) + int(pcounts[q])].astype(np.int64)
                differs += not np.array_equal(got, unpruned)
        tiled.close()
        plain.close()
    assert differs > 0  # the pruning happens


def test_cpc_fixture_over_70_instants(ds):
    with open(os.path.join(HERE, "golden", "pydcdf_fixture.json")) as f:
        rw = json.load(f)["real_world"]
    day = np.load(os.path.join(HERE, "golden", rw["file"]))["precip"].reshape(rw["shape"]).astype(np.float32).reshape(-1, 360, 720)[0]
    scale = (2.0 ** (np.arange(70) % 5 - 2)).astype(np.float32)  # exact in float32: the stored values stay exact
    a = (day[None] * scale[:, None, None]).astype(np.float32)
    v = make_var(ds, a, [4, 6], 32, span_size=4)
    R = v.raster()
    assert sum(t.chunk is None for t in R.tiles) > 0
    rng = np.random.default_rng(70)
    cubes = rand_cubes(rng, a.shape, 300, (40, 120, 160))
    flat, off, _ = R.fill_windows_flat(cubes, dtype=np.float32)
    for q, c in enumerate(cubes):
        w = a[c[0]:c[1], c[2]:c[3], c[4]:c[5]]
        np.testing.assert_array_equal(flat[int(off[q]):int(off[q]) + w.size].reshape(w.shape), w)
    for lo, hi in [(10.0, 20.0), (0.0, 0.0), (50.0, INF), (-INF, INF)]:
        trip, offs, counts, _ = R.search_values_flat(cubes[:60], lo, hi)
        for q, c in enumerate(cubes[:60]):
            got = trip[int(offs[q]):int(offs[q]) + int(counts[q])].astype(np.int64)
            check_order(got, 32, R.tile)
            assert np.array_equal(sort3(got), oracle(a[c[0]:c[1], c[2]:c[3], c[4]:c[5]], lo, hi, (c[0], c[2], c[4]))), (lo, hi, c)


def test_plain_raster_get_and_fill_cell(ds):
    import dcdf_amd
    from dcdf_amd import synth
    from dcdf_amd.raster import EncodedRaster
    shape, tile, cs = (40, 300, 520), 256, 32
    a = synth.cells(0xDCDF0001, 0, shape[0], 0, shape[1], 0, shape[2], np.int32)
    chunks = [dcdf_amd.Chunk.build(np.ascontiguousarray(a[t0:t1, r0:r1, c0:c1])).data
              for (t0, t1, r0, r1, c0, c1) in EncodedRaster.chunk_grid(shape, tile, cs)]
    R = EncodedRaster(shape, chunks, tile, cs)
    rng = np.random.default_rng(0)
    pts = np.stack([rng.integers(0, s, 20000) for s in shape], axis=1).astype(np.uint32)
    want = a[pts[:, 0], pts[:, 1], pts[:, 2]].astype(np.int64)
    for dt in (np.int32, np.int64, np.float64):  # (float output of integer chunks: store_typed, as fill_window_batch_typed)
        vals, _ = R.get_flat(pts, dtype=dt)
        np.testing.assert_array_equal(vals, want.astype(dt) if dt != np.float64 else np.where(want == 0, np.nan, (want - 1) / 2.0))
    buf = device_buf(len(pts) * 4)
    R.get_flat(pts, dtype=np.int32, out_device_ptr=buf.ptr)
    np.testing.assert_array_equal(buf.read(0, len(pts) * 4, np.int32), want)
    buf.free()
    cells = np.stack([rng.integers(0, 41, 3000), rng.integers(0, 41, 3000), rng.integers(0, 300, 3000), rng.integers(0, 520, 3000)],
                     axis=1).astype(np.uint32)
    flat, off, _ = R.fill_cells_flat(cells, dtype=np.int32)
    for i, (x0, x1, r, c) in enumerate(cells.astype(int)):
        lo, hi = min(x0, x1), max(x0, x1)
        np.testing.assert_array_equal(flat[int(off[i]):int(off[i]) + hi - lo], a[lo:hi, r, c])
    R.close()


def test_errors(ds):
    import dcdf_amd
    from dcdf_amd import _lib as L
    from dcdf_amd.raster import EncodedRaster, RasterTile
    a = np.arange(4 * 16 * 16, dtype=np.int32).reshape(4, 16, 16)
    ch = dcdf_amd.Chunk.build(a).data
    mm = np.zeros((4, 2), dtype=np.int64)
    vals = np.arange(4, dtype=np.int64)
    good = [RasterTile(ch, 0, 0, None, mm, L.DCDF_I32, 0, True), RasterTile(None, 0, 0, vals, mm, L.DCDF_I32, 0, True)]

    def code(tiles, shape=(4, 16, 24), tile=16):
        with pytest.raises(L.DcdfError) as e:
            EncodedRaster.from_tiles(shape, tiles, tile, 4)
        return e.value.code

    with pytest.raises(ValueError):  # (the Python layer counts first)
        EncodedRaster.from_tiles((4, 16, 24), good[:1], 16, 4)
    desc, h = (L.RasterTile * 1)(), C.c_void_p()
    assert L.lib().dcdf_raster_create_tiles(desc, C.c_size_t(1), (C.c_uint32 * 3)(4, 16, 24), 16, 4, C.byref(h)) == -1  # wrong count
    assert code([RasterTile(ch, 0, 4, None, mm, L.DCDF_I32, 0, True), good[1]], (4, 16, 32)) == -1   # col0 + 16 > 16
    assert code([good[0], RasterTile(None, 0, 0, None, mm, L.DCDF_I32, 0, True)]) == -1                # elided without values
    assert code([good[0], RasterTile(None, 0, 0, vals, mm, 5, 0, True)]) == -1                          # bad encoding
    assert code([good[0], RasterTile(None, 0, 0, vals, mm, L.DCDF_F64, 63, True)]) == -1               # fractional_bits > 62
    assert code(good, (3, 16, 24)) == -1                                                                  # chunk has 4 instants, leaf 3
    R = EncodedRaster.from_tiles((4, 16, 24), good, 16, 4)
    flat, off, _ = R.fill_windows_flat([(0, 4, 0, 16, 0, 24)], dtype=np.int64)
    want = np.concatenate([a, np.broadcast_to(vals[:, None, None], (4, 16, 8))], axis=2)
    np.testing.assert_array_equal(flat.reshape(4, 16, 24), want)
    for bad in [(4, 0, 0), (0, 16, 0), (0, 0, 24)]:
        with pytest.raises(L.DcdfError) as e:
            R.get_flat([bad])
        assert e.value.code == -5
    with pytest.raises(L.DcdfError) as e:
        R.fill_cells_flat([(0, 5, 0, 0)])
    assert e.value.code == -5
    for f in (lambda: R.split([(0, 1, 0, 1, 0, 1)]), lambda: R.fill_windows([(0, 1, 0, 1, 0, 1)]),
              lambda: R.search([(0, 1, 0, 1, 0, 1)], [0], [1]), lambda: R.window_pieces([(0, 1, 0, 1, 0, 1)]),
              lambda: R.search_pieces([(0, 1, 0, 1, 0, 1)], [0], [1])):
        with pytest.raises(ValueError):
            f()
    # a raster with no chunk leaf at all is valid
    E = EncodedRaster.from_tiles((4, 16, 16), [good[1]], 16, 4)
    trip, offs, counts, _ = E.search_flat([(0, 4, 0, 16, 0, 16)], [2], [3])
    assert int(counts[0]) == 2 * 256
    np.testing.assert_array_equal(E.get_flat([(3, 5, 5)], dtype=np.int32)[0], [3])
    R.close()
    E.close()
    ch.close()


# ---- host output at scattered offsets, through the C ABI (the Python wrappers only pass dense offsets with host memory) ----
SCATTER_SHAPE, SCATTER_TILE, SCATTER_CS = (5, 40, 40), 32, 4  # 2 segments x 2 x 2 leaves: sidelen 32 (bulk units) and the 8 x 8 corner (wave walk)
SCATTER_CUBES = [
    (0, 5, 0, 40, 0, 40),     # the whole raster
    (2, 5, 20, 36, 28, 40),   # across a segment and a tile boundary
    (4, 5, 39, 40, 39, 40),   # one cell
    (3, 1, 5, 30, 10, 35),    # reversed bounds on the time axis
    (2, 2, 0, 40, 0, 40),     # zero volume
]
SCATTER_OFFS = [3000, 7, 12000, 1000, 650]  # elements: out of order, with gaps


@pytest.fixture(scope="module")
def scatter_rasters(ds):
    """The same int32 source as a plain raster and as a tiled one whose leaf (segment 0, rows 0:32, cols 32:40) is elided."""
    import dcdf_amd
    from dcdf_amd import synth, _lib as L
    from dcdf_amd.raster import EncodedRaster, RasterTile
    a = synth.cells(0xDCDF0007, 0, SCATTER_SHAPE[0], 0, SCATTER_SHAPE[1], 0, SCATTER_SHAPE[2], np.int32)
    a[0:4, 0:32, 32:40] = np.array([11, -7, 0, 123456], dtype=np.int32)[:, None, None]  # one value per instant: can be elided
    grid = EncodedRaster.chunk_grid(SCATTER_SHAPE, SCATTER_TILE, SCATTER_CS)
    chunks = [dcdf_amd.Chunk.build(np.ascontiguousarray(a[t0:t1, r0:r1, c0:c1])).data for (t0, t1, r0, r1, c0, c1) in grid]
    plain = EncodedRaster(SCATTER_SHAPE, chunks, SCATTER_TILE, SCATTER_CS)
    tiles = [RasterTile(c, 0, 0, None, None, L.DCDF_I32, 0, False) for c in chunks]
    tiles[1] = RasterTile(None, 0, 0, a[0:4, 0, 32].astype(np.int64), None, L.DCDF_I32, 0, False)
    tiled = EncodedRaster.from_tiles(SCATTER_SHAPE, tiles, SCATTER_TILE, SCATTER_CS)
    yield a, {"plain": plain, "tiled": tiled}
    plain.close()
    tiled.close()
    for c in chunks:
        c.close()


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("form", ["plain", "tiled"])
def test_host_output_at_scattered_offsets(scatter_rasters, form, dtype):
    """include/dcdf_k2r.h: cube q's window goes to out + out_offset[q] and nothing else is written -- dcdf_raster_fill_window_batch
    and dcdf_raster_decode_batch with host memory, offsets out of order and with gaps."""
    from dcdf_amd import _lib as L
    a, rasters = scatter_rasters
    R = rasters[form]
    enc = {np.int32: L.DCDF_I32, np.int64: L.DCDF_I64}[dtype]
    sent = {np.int32: -0x5a5a5a5b, np.int64: -0x5a5a5a5a5a5a5a5b}[dtype]
    nq = len(SCATTER_CUBES)
    cubes = (L.Cube * nq)(*[L.Cube(*c) for c in SCATTER_CUBES])
    offs = np.array(SCATTER_OFFS, dtype=np.uint64)
    norm = [(min(s, e), max(s, e), min(t, b), max(t, b), min(l, r), max(l, r)) for s, e, t, b, l, r in SCATTER_CUBES]

    def check(out):
        mask = np.zeros(out.size, dtype=bool)
        for (s, e, t, b, l, r), o in zip(norm, SCATTER_OFFS):
            v = (e - s) * (b - t) * (r - l)
            np.testing.assert_array_equal(out[o:o + v].reshape(e - s, b - t, r - l), a[s:e, t:b, l:r])
            assert not mask[o:o + v].any()
            mask[o:o + v] = True
        assert (out[~mask] == sent).all()

    ms = C.c_float()
    out = np.full(12010, sent, dtype=dtype)
    L.check(L.lib().dcdf_raster_fill_window_batch(R._handle(), cubes, C.c_size_t(nq), C.c_void_p(out.ctypes.data), enc, L.MEM_HOST,
                                                  C.c_void_p(offs.ctypes.data), C.byref(ms)), "raster_fill_window_batch")
    check(out)
    out = np.full(12010, sent, dtype=dtype)
    stats = np.zeros(3, dtype=np.uint64)
    L.check(L.lib().dcdf_raster_decode_batch(R._handle(), cubes, C.c_size_t(nq), C.c_void_p(out.ctypes.data), enc, L.MEM_HOST,
                                             C.c_void_p(offs.ctypes.data), C.c_void_p(stats.ctypes.data), C.byref(ms)), "raster_decode_batch")
    check(out)
    assert stats[0] > 0 and stats[1] > 0 and (stats[2] > 0) == (form == "tiled")  # bulk units, the wave walk, the elided fill
    assert int(stats.sum()) == sum((e - s) * (b - t) * (r - l) for s, e, t, b, l, r in norm)
