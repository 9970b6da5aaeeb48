"""Bulk decode (dcdf_raster_decode_batch, EncodedRaster.decode / decode_flat, Variable.decode) on the GPU: every comparison is
exact, float results as bit patterns (NaN positions count) -- against the source arrays, against fill_windows_flat on the same
cubes, and against the oracle's Chunk::fill_window for a chunk built to hold every leaf kind of the Log rule."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from bulk_model import leaf_kinds_array

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 0xDCDF0011
BITS = 3


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(bits_of(got), bits_of(want))


def source(kind, shape, seed=SEED):
    """The synthetic model as int32, as int64 (2 v + 1), as float32 / float64 with BITS fractional bits and NaN patches."""
    from dcdf_amd import synth
    T, R, Cc = shape
    if kind == "i32":
        return synth.cells(seed, 0, T, 0, R, 0, Cc, np.int32)
    if kind == "i64":
        return synth.cells(seed, 0, T, 0, R, 0, Cc, np.int64)
    v = synth.cells(seed, 0, T, 0, R, 0, Cc, np.int32)
    x = (v / 2.0 ** BITS).astype(np.float32 if kind == "f32" else np.float64)  # (exact: |v| < 2^13)
    x[3:9, 40:75, 100:180] = np.nan
    x[:, 300:316, 256:272] = np.nan  # a side-16 square that is NaN at every instant
    x[T - 1, R - 5:, :] = np.nan
    return x


def build_raster(dc, a, tile, cs, k=2):
    from dcdf_amd.raster import EncodedRaster
    grid = EncodedRaster.chunk_grid(a.shape, tile, cs)
    fb = BITS if a.dtype.kind == "f" else 0
    builds = dc.build_batch([np.ascontiguousarray(a[t0:t1, r0:r1, c0:c1]) for t0, t1, r0, r1, c0, c1 in grid], k=k, fractional_bits=fb)
    assert not any(isinstance(b, Exception) for b in builds)
    return EncodedRaster(a.shape, [b.data for b in builds], tile=tile, chunk_size=cs)


def sidelen(rows, cols, k=2):
    s = 1
    while s < max(rows, cols):
        s *= k
    return s


def bulk_cells(shape, tile, cs, cubes):
    """Requested cells that lie in chunk leaves of sidelen >= 32 (k = 2), from the grid."""
    from dcdf_amd.raster import EncodedRaster
    n = 0
    for q in np.asarray(cubes, dtype=np.int64).reshape(-1, 6):
        a0, a1, b0, b1, d0, d1 = min(q[0], q[1]), max(q[0], q[1]), min(q[2], q[3]), max(q[2], q[3]), min(q[4], q[5]), max(q[4], q[5])
        for t0, t1, r0, r1, c0, c1 in EncodedRaster.chunk_grid(shape, tile, cs):
            if 32 <= sidelen(r1 - r0, c1 - c0) <= 256:
                n += max(0, min(a1, t1) - max(a0, t0)) * max(0, min(b1, r1) - max(b0, r0)) * max(0, min(d1, c1) - max(d0, c0))
    return n


def volume(cubes):
    q = np.asarray(cubes, dtype=np.int64).reshape(-1, 6)
    return int(np.abs((q[:, 1] - q[:, 0]) * (q[:, 3] - q[:, 2]) * (q[:, 5] - q[:, 4])).sum())


# shape [70, 600, 520], tile 256, chunk_size 32: full chunks, padded chunks (88 rows in a sidelen-256 tree, 88 x 8 in a sidelen-128
# one), a short last segment.  Every chunk of it has sidelen >= 128, so a second, smaller raster adds what the first cannot: a
# corner chunk of 8 x 8 (sidelen 8: the fallback walk) beside bulk chunks in the same call.
RASTERS = {"wide": ((70, 600, 520), 256, 32), "mixed": ((20, 264, 264), 256, 8)}
DT = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def rasters(dc):
    made = {}

    def get(which, kind):
        if (which, kind) not in made:
            shape, tile, cs = RASTERS[which]
            a = source(kind, shape)
            made[(which, kind)] = (a, build_raster(dc, a, tile, cs))
        return made[(which, kind)]

    yield get
    for _, r in made.values():
        r.close()


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
@pytest.mark.parametrize("which", ["wide", "mixed"])
def test_whole_raster_every_dtype(rasters, which, kind):
    a, R = rasters(which, kind)
    shape, tile, cs = RASTERS[which]
    assert_same(R.decode(dtype=a.dtype), a)
    assert_same(R.decode(5, shape[0] - 3, dtype=a.dtype), a[5:shape[0] - 3])
    cube = [[0, shape[0], 0, shape[1], 0, shape[2]]]
    got, off, ms, stats = R.decode_flat(cube, dtype=a.dtype)
    want, woff, _ = R.fill_windows_flat(cube, dtype=a.dtype)
    assert_same(got, want)
    np.testing.assert_array_equal(off, woff)
    assert ms > 0
    # the bulk path is really taken: the cells in leaves with a side-16 table (a condition on the grid, not a measurement: the
    # model's values are far inside +-2^30, so every such chunk has a table)
    assert int(stats[0]) == bulk_cells(shape, tile, cs, cube)
    assert int(stats.sum()) == volume(cube)
    if which == "wide":
        assert int(stats[0]) == volume(cube)
    else:
        assert int(stats[1]) == shape[0] * 8 * 8 and int(stats[2]) == 0
    if kind in ("i32", "f32"):  # integer chunks through the float conversions and the other way round (store_typed)
        for dt in (np.int64, np.float64, np.float32, np.int32):
            g, _, _, _ = R.decode_flat(cube, dtype=dt)
            w, _, _ = R.fill_windows_flat(cube, dtype=dt)
            assert_same(g, w)


def random_cubes(rng, shape, n):
    T, Rr, Cc = shape
    t0, r0, c0 = rng.integers(0, T, n), rng.integers(0, Rr, n), rng.integers(0, Cc, n)
    t1 = np.minimum(T, t0 + rng.integers(1, T + 1, n))
    r1 = np.minimum(Rr, r0 + rng.integers(1, Rr + 1, n))
    c1 = np.minimum(Cc, c0 + rng.integers(1, Cc + 1, n))
    # most cubes small, some large: the whole raster 300 times over would only repeat test 1
    small = rng.random(n) < 0.85
    t1 = np.where(small, np.minimum(t1, t0 + rng.integers(1, 9, n)), t1)
    r1 = np.where(small, np.minimum(r1, r0 + rng.integers(1, 150, n)), r1)
    c1 = np.where(small, np.minimum(c1, c0 + rng.integers(1, 150, n)), c1)
    q = np.stack([t0, t1, r0, r1, c0, c1], axis=1).astype(np.uint32)
    for i in range(0, n, 7):  # some reversed
        ax = 2 * int(rng.integers(0, 3))
        q[i, ax], q[i, ax + 1] = q[i, ax + 1], q[i, ax]
    return q


@pytest.mark.parametrize("kind,which", [("i32", "wide"), ("f32", "wide"), ("i64", "mixed"), ("f64", "mixed")])
def test_unaligned_cubes(rasters, kind, which):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters(which, kind)
    shape = RASTERS[which][0]
    rng = np.random.default_rng(300 + len(kind) + len(which))
    cubes = random_cubes(rng, shape, 300)
    cubes[0] = [0, shape[0], 0, shape[1], 0, shape[2]]   # 1-70 instants, 1-600 x 1-520 cells: the extremes are in
    cubes[1] = [3, 4, 7, 8, 9, 10]
    dt = a.dtype
    got, off, _, stats = R.decode_flat(cubes, dtype=dt)
    want, woff, _ = R.fill_windows_flat(cubes, dtype=dt)
    np.testing.assert_array_equal(off, woff)
    assert_same(got, want)
    assert int(stats.sum()) == volume(cubes)
    for q in (0, 1, 7, 14, 100):  # (and fill_windows_flat itself is the source array)
        c = cubes[q].astype(int)
        w = a[min(c[0], c[1]):max(c[0], c[1]), min(c[2], c[3]):max(c[2], c[3]), min(c[4], c[5]):max(c[4], c[5])]
        assert_same(got[int(off[q]):int(off[q]) + w.size].reshape(w.shape), w)
    # device form, explicit offsets with gaps (odd ones: rows start at every alignment)
    vol = np.abs((cubes[:, 1].astype(np.int64) - cubes[:, 0]) * (cubes[:, 3].astype(np.int64) - cubes[:, 2]) *
                 (cubes[:, 5].astype(np.int64) - cubes[:, 4])).astype(np.uint64)
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1])
    buf, ref = DeviceBuffer(total * dt.itemsize), DeviceBuffer(total * dt.itemsize)
    fill = np.full(total, 77, dtype=dt)
    buf.write(0, fill)
    ref.write(0, fill)
    ms, dstats = R.decode_flat(cubes, dtype=dt, out_device_ptr=buf.ptr, out_offset=doff)
    R.fill_windows_flat(cubes, dtype=dt, out_device_ptr=ref.ptr, out_offset=doff)
    g, w = buf.read(0, total * dt.itemsize, dt), ref.read(0, total * dt.itemsize, dt)
    buf.free()
    ref.free()
    assert_same(g, w)  # (the gaps too: nothing is written outside a cube)
    np.testing.assert_array_equal(dstats, stats)
    for q in range(len(cubes)):
        assert_same(g[int(doff[q]):int(doff[q] + vol[q])], got[int(off[q]):int(off[q] + vol[q])])


@pytest.mark.parametrize("shape", [(40, 256, 256), (40, 200, 131)], ids=["full", "padded"])
def test_every_leaf_kind_against_the_oracle(dc, shape):
    from dcdf_amd.raster import EncodedRaster
    a = np.ascontiguousarray(leaf_kinds_array(np.random.default_rng(33))[:, :shape[1], :shape[2]])
    data = O.chunk_build_forced(a, 2, 8)
    oc = O.Chunk(data)
    assert oc.block_lengths() == [8] * 5
    ch = dc.Chunk(data)
    R = EncodedRaster(shape, [ch], tile=256, chunk_size=40)
    whole = [[0, 40, 0, shape[1], 0, shape[2]]]
    want = oc.fill_window(0, 40, 0, shape[1], 0, shape[2], dtype=np.int64)
    np.testing.assert_array_equal(want, a)
    got, _, _, stats = R.decode_flat(whole, dtype=np.int64)
    assert_same(got.reshape(shape), want)
    assert int(stats[0]) == a.size and int(stats[1]) == 0
    rng = np.random.default_rng(34)
    cubes = random_cubes(rng, shape, 60)
    got, off, _, stats = R.decode_flat(cubes, dtype=np.int32)
    assert int(stats[0]) == volume(cubes)
    for q, c in enumerate(cubes.astype(int)):
        w = oc.fill_window(min(c[0], c[1]), max(c[0], c[1]), min(c[2], c[3]), max(c[2], c[3]), min(c[4], c[5]), max(c[4], c[5]), dtype=np.int32)
        assert_same(got[int(off[q]):int(off[q]) + w.size].reshape(w.shape), w)
    R.close()
    # the same array through the library's own encoder and block policy
    b = dc.Chunk.build(a)
    R2 = EncodedRaster(shape, [b.data], tile=256, chunk_size=40)
    assert b.snapshots > 1 and b.logs > 1
    assert_same(R2.decode(dtype=np.int64), a)
    R2.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
@pytest.mark.parametrize("levels,shape", [([4, 8], (34, 300, 2060)), ([1, 6, 5], (40, 40, 2112))], ids=["4x8", "1x6x5_offset_leaves"])
def test_stored_variable(dtype, levels, shape):
    """Dataset.append of a raster with forced-uniform tiles (the construction of test_gpu_stored_raster): elided tiles, nested
    levels, a short last segment; k2_levels [1, 6, 5] adds a 40 x 64 chunk built at the top level that spans two leaves of 32."""
    import test_gpu_stored_raster as SR
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    rng = np.random.default_rng(sum(shape))
    a = SR.var_data(rng, shape, dtype, 1 << levels[-1])
    v = SR.make_var(dataset, a, levels, 32)
    R = v.raster()
    assert any(t.chunk is None for t in R.tiles) and any(t.chunk is not None for t in R.tiles)
    if len(levels) == 3:
        assert any(t.row0 or t.col0 for t in R.tiles)
    T, Rr, Cc = shape
    want = v.window(0, T, 0, Rr, 0, Cc)
    got = v.decode()
    assert_same(got, want)
    assert_same(got, a)
    assert_same(v.decode(7, T - 1), want[7:T - 1])
    assert v.decode(4, 4).shape == (0, Rr, Cc)
    _, _, _, stats = R.decode_flat([[0, T, 0, Rr, 0, Cc]], dtype=dtype)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    with pytest.raises(IndexError):
        v.decode(0, T + 1)


def test_fallbacks_k3_and_wide_values(dc):
    from dcdf_amd import synth
    a3 = synth.cells(SEED, 0, 10, 0, 100, 0, 90, np.int32)
    R3 = build_raster(dc, a3, 64, 8, k=3)
    wide = synth.cells(SEED, 0, 10, 0, 100, 0, 90, np.int64)
    for r, c in ((5, 7), (5, 80), (70, 7)):    # beyond 2^30 in every chunk of the grid (tile 64): the 64-bit walk
        wide[:, r, c] += 2 ** 30 + 12345
    wide[:, 70, 80] = -(2 ** 35)
    Rw = build_raster(dc, wide, 64, 8)
    rng = np.random.default_rng(5)
    for R, a in ((R3, a3), (Rw, wide)):
        cubes = np.concatenate([[[0, 10, 0, 100, 0, 90]], random_cubes(rng, a.shape, 40)]).astype(np.uint32)
        got, off, _, stats = R.decode_flat(cubes, dtype=a.dtype)
        want, woff, _ = R.fill_windows_flat(cubes, dtype=a.dtype)
        assert_same(got, want)
        np.testing.assert_array_equal(off, woff)
        assert int(stats[0]) == 0 and int(stats[1]) == volume(cubes)
        assert_same(R.decode(dtype=a.dtype), a)
        R.close()


CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import dcdf_amd
from dcdf_amd import synth
from dcdf_amd.raster import EncodedRaster
a = synth.cells(0xDCDF0011, 0, 12, 0, 300, 0, 200, np.int32)
grid = EncodedRaster.chunk_grid(a.shape, 256, 8)
R = EncodedRaster(a.shape, [b.data for b in dcdf_amd.build_batch([np.ascontiguousarray(a[t0:t1, r0:r1, c0:c1]) for t0, t1, r0, r1, c0, c1 in grid])], 256, 8)
cubes = [[0, 12, 0, 300, 0, 200], [3, 11, 17, 290, 5, 133]]
got, off, _, stats = R.decode_flat(cubes, dtype=np.int32)
want, woff, _ = R.fill_windows_flat(cubes, dtype=np.int32)
assert np.array_equal(got, want) and np.array_equal(off, woff)
assert np.array_equal(got[:a.size].reshape(a.shape), a)
print("STATS", int(stats[0]), int(stats[1]), int(stats[2]))
"""


def test_fallback_without_top_table_in_a_child_process():
    env = dict(os.environ, K2R_NO_TOP_TABLE="1")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    vol = 12 * 300 * 200 + 8 * 273 * 128
    assert "STATS 0 %d 0" % vol in out.stdout, out.stdout[-500:]


def test_errors(dc, rasters):
    from dcdf_amd import _lib as L
    a, R = rasters("mixed", "i32")
    shape = RASTERS["mixed"][0]
    lib = L.lib()
    out = np.zeros(64, dtype=np.int64)
    off = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()

    def call(h, cubes, nq, outp, dtype, offp, mem=L.MEM_HOST):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        return lib.dcdf_raster_decode_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), outp, dtype, mem, offp,
                                            C.c_void_p(stats.ctypes.data), C.byref(ms))

    o, f = C.c_void_p(out.ctypes.data), C.c_void_p(off.ctypes.data)
    small = [[0, 1, 0, 2, 0, 2]]
    assert call(R._handle(), small, 1, o, L.DCDF_I64, f) == 0 and int(stats.sum()) == 4
    np.testing.assert_array_equal(out[:4], a[0, :2, :2].ravel())
    for bad in ([[0, shape[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, shape[1] + 1, 0, 2]], [[0, 1, 0, 2, shape[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, o, L.DCDF_I64, f) == -5  # DCDF_ERR_BOUNDS
    assert call(R._handle(), small, 1, o, 5, f) == -1                # a bad dtype: DCDF_ERR_BAD_ARG
    assert call(R._handle(), small, 1, o, L.DCDF_I64, f, mem=7) == -1
    assert call(None, small, 1, o, L.DCDF_I64, f) == -1              # NULL arguments
    assert call(R._handle(), None, 1, o, L.DCDF_I64, f) == -1
    assert call(R._handle(), small, 1, None, L.DCDF_I64, f) == -1
    assert call(R._handle(), small, 1, o, L.DCDF_I64, None) == -1
    assert call(R._handle(), small, 0, o, L.DCDF_I64, f) == 0        # nq == 0 is fine
    # stats and kernel_ms may be NULL; an empty cube writes nothing
    q = np.array([[2, 2, 0, 5, 0, 5]], dtype=np.uint32)
    out[:] = -1
    assert lib.dcdf_raster_decode_batch(R._handle(), C.c_void_p(q.ctypes.data), C.c_size_t(1), o, L.DCDF_I64, L.MEM_HOST, f, None, None) == 0
    assert (out == -1).all()
    assert lib.dcdf_strerror(-5)


def test_full_size_segment(dc):
    """One segment of the 4096 x 4096 x 365 raster: [32, 4096, 4096] int32, encoded on the device, opened where it lies, decoded into
    a device buffer and compared band by band with the generator's integers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_query as BQ
    from dcdf_amd import _lib as L
    from dcdf_amd.encoder import DeviceBuffer, synth_fill
    from dcdf_amd.raster import EncodedRaster
    enc, grid, TT, raster = BQ.encode_raster(1)
    chunks = enc.open_chunks()
    raster.free()
    E = 4096
    R = EncodedRaster((TT, E, E), chunks)
    out = DeviceBuffer(TT * E * E * 4)
    cubes = [[0, TT, 0, E, 0, E]]
    ms, stats = R.decode_flat(cubes, dtype=np.int32, out_device_ptr=out.ptr, out_offset=[0])
    print("full-size segment: %.3f ms in-kernel, %.3e cells/s" % (ms, TT * E * E / (ms * 1e-3)))
    assert int(stats[0]) == TT * E * E and int(stats[1]) == 0 and int(stats[2]) == 0
    band = DeviceBuffer(E * E * 4)
    for t in range(TT):
        synth_fill(band.ptr, L.DCDF_I32, BQ.SEED, t, t + 1, 0, E, 0, E)
        want = band.read(0, E * E * 4, np.int32)
        got = out.read(t * E * E * 4, E * E * 4, np.int32)
        assert np.array_equal(got, want), "instant %d" % t
    band.free()
    out.free()
    R.close()
    for c in chunks:
        c.close()
    enc.close()
