"""Reduce over time (dcdf_raster_reduce_time_batch, EncodedRaster.reduce_time / reduce_time_flat, Variable.reduce_time) on the GPU.
Every comparison is on bit patterns against the NumPy model of reduce_model.py: the values widened to float64, fmin / fmax, the
sequential sum in instant order, the count and one division."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import reduce_model as M
import test_gpu_bulk_decode as BD
from bulk_model import leaf_kinds_array
from test_gpu_bulk_decode import assert_same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ALL = 31
SHAPE, TILE, CS = (20, 264, 264), 256, 8  # three segments, the last one short; bulk chunks and the 8 x 8 corner chunk (fallback walk)


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


def source(kind):
    a = BD.source(kind, SHAPE)
    if a.dtype.kind == "f":  # besides the NaN patches of the decode test: cells NaN at every instant, and at every instant but one
        a[:, 17, 23] = np.nan
        a[:6, 200, 5] = np.nan
        a[7:, 200, 5] = np.nan
        a[:, 258, 259] = np.nan  # (the same in the corner chunk)
        a[1:, 260, 261] = np.nan
    return a


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


def norm(c):
    c = [int(x) for x in c]
    return min(c[0], c[1]), max(c[0], c[1]), min(c[2], c[3]), max(c[2], c[3]), min(c[4], c[5]), max(c[4], c[5])


def check_cube(flat, off, q, mask, cube, a):
    """Cube q of a reduce_time_flat result equals the model on the array `a` the raster holds."""
    t0, t1, r0, r1, c0, c1 = norm(cube)
    if (t1 - t0) * (r1 - r0) * (c1 - c0) == 0:
        return
    want = M.reduce_time(a[t0:t1, r0:r1, c0:c1])
    got = M.planes(flat, off, q, mask, r1 - r0, c1 - c0)
    assert list(got) == M.names_of(mask)
    for n in got:
        assert_same(got[n], want[n])


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_segments_and_blocks(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    if kind[0] == "f":
        x = M.reduce_time(a)
        assert (x["count"] == 0).any() and (x["count"] == 1).any() and np.isnan(x["min"]).any()
    for t0, t1 in ((0, T), (5, 17), (3, 4)):  # whole; from the middle of a block across two segment boundaries; one instant
        cube = [[t0, t1, 0, Rr, 0, Cc]]
        flat, off, ms, stats = R.reduce_time_flat(cube, ALL)
        assert ms > 0 and flat.size == 5 * Rr * Cc and off.tolist() == [0]
        check_cube(flat, off, 0, ALL, cube[0], a)
        _, _, _, dstats = R.decode_flat(cube, dtype=a.dtype)
        np.testing.assert_array_equal(stats, dstats)
        assert int(stats[0]) > 0 and int(stats[1]) == (t1 - t0) * 8 * 8 and int(stats[2]) == 0
        for mask in (1, 16):  # MIN alone (one accumulator), MEAN alone (sum and count in scratch planes)
            f1, o1, _, s1 = R.reduce_time_flat(cube, mask)
            assert f1.size == Rr * Cc
            check_cube(f1, o1, 0, mask, cube[0], a)
            np.testing.assert_array_equal(s1, stats)
    d = R.reduce_time(("max", "count"), 2, 19, window=(250, 264, 3, 264))
    want = M.reduce_time(a[2:19, 250:264, 3:264])
    assert list(d) == ["max", "count"]
    assert_same(d["max"], want["max"])
    assert_same(d["count"], want["count"])


# 2 x 2 tiles -- 64 x 64, two strips of 6 and the 6 x 6 corner chunk (fallback walk) -- and three segments, the last one short.  The
# second cube is unaligned in every edge and its planes have an odd size (63 x 63), so a row's four cells are clipped, meet their
# plane at a misaligned address, and every piece after the first continues the state its cells' planes hold.
FOLD_SHAPE, FOLD_TILE, FOLD_CS = (20, 70, 70), 64, 8
FOLD_CUBES = [[0, 20, 0, 70, 0, 70], [3, 19, 3, 66, 5, 68]]


def fold_source(kind):
    a = BD.source(kind, FOLD_SHAPE)
    if a.dtype.kind == "f":
        a[:, 17, 23] = np.nan        # at every instant
        a[:6, 40, 5] = np.nan        # at every instant but one
        a[7:, 40, 5] = np.nan
        a[2:11, 10:30, 30:50] = np.nan  # a patch across the first segment boundary
        a[5:, 66, 67] = np.nan       # (in the corner chunk)
    return a


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_every_instantiation_of_the_shared_fold(dc, kind):
    """Every `ops` in 1 .. 31: k_bulk_reduce<LIVE> for LIVE 1 .. 15, with and without MEAN, and the per-cell fold kernel."""
    a = fold_source(kind)
    R = BD.build_raster(dc, a, FOLD_TILE, FOLD_CS)
    want = [M.reduce_time(a[t0:t1, r0:r1, c0:c1]) for t0, t1, r0, r1, c0, c1 in FOLD_CUBES]
    if kind == "f32":
        assert (want[0]["count"] == 0).any() and (want[0]["count"] == 1).any() and (want[1]["count"] < 16).any()
    for ops in range(1, 32):
        flat, off, _, stats = R.reduce_time_flat(FOLD_CUBES, ops)
        assert int(stats[0]) > 0 and int(stats[1]) > 0 and int(stats.sum()) == BD.volume(FOLD_CUBES)
        for q, (t0, t1, r0, r1, c0, c1) in enumerate(FOLD_CUBES):
            got = M.planes(flat, off, q, ops, r1 - r0, c1 - c0)
            assert list(got) == M.names_of(ops)
            for n in got:
                assert_same(got[n], want[q][n])
    R.close()


def order_raster(dc, dtype):
    """[24, 64, 64], tile 64, chunk_size 8: three segments built apart with 0, 25 and 12 fractional bits, values m / 2^bits with
    |m| < 2^28 -- stored integers 2 m + 1 inside +-2^30, so every chunk takes the bulk kernel -- whose sum depends on the order."""
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(2024)
    segs, chunks = [], []
    for fb in (0, 25, 12):
        m = rng.integers(-(2 ** 28) + 1, 2 ** 28, size=(8, 64, 64))
        x = (m / 2.0 ** fb).astype(dtype) if np.dtype(dtype).kind == "f" else m.astype(dtype)
        segs.append(x)
        (b,) = dc.build_batch([np.ascontiguousarray(x)], k=2, fractional_bits=fb if np.dtype(dtype).kind == "f" else 0)
        assert not isinstance(b, Exception)
        chunks.append(b.data)
    return np.concatenate(segs), chunks, EncodedRaster


def test_summation_order_is_observable(dc):
    a, chunks, EncodedRaster = order_raster(dc, np.float64)
    seq = M.reduce_time(a)["sum"]
    ones = np.ones((8, 64, 64), dtype=bool)
    parts = [M.sequential_sum(a[s:s + 8], ones) for s in (0, 8, 16)]
    assert ((parts[0] + parts[1]) + parts[2] != seq).any(), "per-segment partial sums equal the sequential sum: the input proves nothing"
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    cube = [[0, 24, 0, 64, 0, 64]]
    flat, off, _, stats = R.reduce_time_flat(cube, ("sum",))
    assert int(stats[0]) == a.size and int(stats[1]) == 0
    assert_same(flat.reshape(64, 64), seq)
    flat, off, _, _ = R.reduce_time_flat(cube, ALL)
    check_cube(flat, off, 0, ALL, cube[0], a)
    flat, off, _, _ = R.reduce_time_flat([[3, 21, 5, 64, 0, 59]], ("sum", "mean"))
    check_cube(flat, off, 0, 20, [3, 21, 5, 64, 0, 59], a)
    R.close()


def test_int64_beyond_2_53_rounds_to_nearest(dc):
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(7)
    a = rng.integers(-(2 ** 28) + 1, 2 ** 28, size=(24, 64, 64)).astype(np.int64)
    t = np.arange(24, dtype=np.int64)
    a[:, 3, 5] = 2 ** 53 + 1 + 2 * t           # odd beyond 2^53: every one rounds
    a[:, 10, 60] = -(2 ** 60) - 3 - 1024 * t
    a[:, 63, 0] = (2 ** 62 + 2 ** 9 + 1) * (1 - 2 * (t % 2))
    builds = dc.build_batch([np.ascontiguousarray(a[s:s + 8]) for s in (0, 8, 16)], k=2)
    assert not any(isinstance(b, Exception) for b in builds)
    R = EncodedRaster(a.shape, [b.data for b in builds], tile=64, chunk_size=8)
    assert (M.widen(a).astype(np.int64) != a).any()
    cube = [[0, 24, 0, 64, 0, 64]]
    flat, off, _, stats = R.reduce_time_flat(cube, ALL)
    assert int(stats[0]) == 0 and int(stats[1]) == a.size  # values beyond 2^30: the 64-bit walk
    check_cube(flat, off, 0, ALL, cube[0], a)
    R.close()


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_unaligned_batch(rasters, kind):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters(kind)
    rng = np.random.default_rng(500 + len(kind))
    cubes = BD.random_cubes(rng, SHAPE, 100)
    cubes[0] = [0, SHAPE[0], 0, SHAPE[1], 0, SHAPE[2]]
    cubes[1] = [3, 4, 7, 8, 9, 10]                 # one cell, one instant
    cubes[2] = [9, 10, 0, SHAPE[1], 0, SHAPE[2]]   # one instant
    cubes[3] = [0, SHAPE[0], 261, 262, 130, 131]   # one cell
    cubes[4] = [6, 6, 0, 30, 0, 30]                # no instants: writes nothing
    mask = 27  # min, max, count, mean: the sum lives in a scratch plane
    flat, off, _, stats = R.reduce_time_flat(cubes, mask)
    _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
    np.testing.assert_array_equal(stats, dstats)
    for q, c in enumerate(cubes):
        check_cube(flat, off, q, mask, c, a)
    # device form: odd gaps between the windows, a sentinel everywhere first
    nb = np.array([norm(c) for c in cubes], dtype=np.int64)
    vol = (4 * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64))
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1]) + 7
    buf = DeviceBuffer(total * 8)
    buf.write(0, np.full(total, -77.25, dtype=np.float64))
    ms, dvstats = R.reduce_time_flat(cubes, mask, out_device_ptr=buf.ptr, out_offset=doff)
    g = buf.read(0, total * 8, np.float64)
    buf.free()
    np.testing.assert_array_equal(dvstats, stats)
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        o, n = int(doff[q]), int(vol[q])
        inside[o:o + n] = True
        assert_same(g[o:o + n], flat[int(off[q]):int(off[q]) + n])
    assert (g[~inside] == -77.25).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's planes


@pytest.mark.parametrize("shape", [(40, 256, 256), (40, 200, 131)], ids=["full", "padded"])
def test_every_leaf_kind_against_the_oracle(dc, shape):
    from dcdf_amd.raster import EncodedRaster
    a = np.ascontiguousarray(leaf_kinds_array(np.random.default_rng(33))[:, :shape[1], :shape[2]])
    data = O.chunk_build_forced(a, 2, 8)
    oc = O.Chunk(data)
    assert oc.block_lengths() == [8] * 5
    R = EncodedRaster(shape, [dc.Chunk(data)], tile=256, chunk_size=40)
    cubes = np.array([[0, 40, 0, shape[1], 0, shape[2]], [5, 17, 0, shape[1], 0, shape[2]], [0, 40, 33, 170, 61, 131], [12, 13, 1, 2, 3, 130],
                      [7, 33, 63, 129, 1, 66]], dtype=np.uint32)
    flat, off, _, stats = R.reduce_time_flat(cubes, ALL)
    assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0
    for q, c in enumerate(cubes.astype(int)):
        want = M.reduce_time(oc.fill_window(*c, dtype=np.int64))
        got = M.planes(flat, off, q, ALL, c[3] - c[2], c[5] - c[4])
        for n in M.NAMES:
            assert_same(got[n], want[n])
    R.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
@pytest.mark.parametrize("levels,shape", [([4, 8], (34, 300, 2060)), ([1, 6, 5], (40, 40, 2112))], ids=["4x8", "1x6x5_offset_leaves"])
def test_stored_variable(dtype, levels, shape):
    """The two constructions of the decode test: elided tiles, nested levels, offset leaves, a short last segment."""
    import test_gpu_stored_raster as SR
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    rng = np.random.default_rng(sum(shape))
    a = SR.var_data(rng, shape, dtype, 1 << levels[-1])
    v = SR.make_var(dataset, a, levels, 32)
    T, Rr, Cc = shape
    got = v.reduce_time(M.NAMES)
    want = M.reduce_time(v.window(0, T, 0, Rr, 0, Cc))
    assert list(got) == list(M.NAMES)
    for n in M.NAMES:
        assert_same(got[n], want[n])
    win = (7, T - 1, 5, Rr - 3, 250, Cc - 9)
    got = v.reduce_time(("mean", "max"), *win)
    want = M.reduce_time(v.window(*win))
    assert list(got) == ["max", "mean"]
    assert_same(got["max"], want["max"])
    assert_same(got["mean"], want["mean"])
    assert list(v.reduce_time()) == ["mean"]
    _, _, _, stats = v.raster().reduce_time_flat([[0, T, 0, Rr, 0, Cc]], ALL)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    none = v.reduce_time(("count", "min"), 4, 4)
    assert none["count"].shape == (Rr, Cc) and (none["count"] == 0).all() and np.isnan(none["min"]).all()
    with pytest.raises(IndexError):
        v.reduce_time(stop=T + 1)
    with pytest.raises(IndexError):
        v.reduce_time(right=Cc + 1)


def test_fallbacks_k3_and_wide_values(dc):
    from dcdf_amd import synth
    a3 = synth.cells(BD.SEED, 0, 10, 0, 100, 0, 90, np.int32)
    R3 = BD.build_raster(dc, a3, 64, 8, k=3)
    wide = synth.cells(BD.SEED, 0, 10, 0, 100, 0, 90, np.int64)
    for r, c in ((5, 7), (5, 80), (70, 7)):    # beyond 2^30 in every chunk of the grid (tile 64): the 64-bit walk
        wide[:, r, c] += 2 ** 30 + 12345
    wide[:, 70, 80] = -(2 ** 35)
    Rw = BD.build_raster(dc, wide, 64, 8)
    rng = np.random.default_rng(5)
    for R, a in ((R3, a3), (Rw, wide)):
        cubes = np.concatenate([[[0, 10, 0, 100, 0, 90]], BD.random_cubes(rng, a.shape, 30)]).astype(np.uint32)
        flat, off, _, stats = R.reduce_time_flat(cubes, ALL)
        assert int(stats[0]) == 0 and int(stats[1]) == BD.volume(cubes)
        for q, c in enumerate(cubes):
            check_cube(flat, off, q, ALL, c, a)
        R.close()


CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import dcdf_amd
import reduce_model as M
from dcdf_amd import synth
from dcdf_amd.raster import EncodedRaster
a = synth.cells(0xDCDF0011, 0, 12, 0, 300, 0, 200, np.int32)
grid = EncodedRaster.chunk_grid(a.shape, 256, 8)
R = EncodedRaster(a.shape, [b.data for b in dcdf_amd.build_batch([np.ascontiguousarray(a[t0:t1, r0:r1, c0:c1]) for t0, t1, r0, r1, c0, c1 in grid])], 256, 8)
cubes = [[0, 12, 0, 300, 0, 200], [3, 11, 17, 290, 5, 133]]
flat, off, _, stats = R.reduce_time_flat(cubes, 31)
for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes):
    want = M.reduce_time(a[t0:t1, r0:r1, c0:c1])
    got = M.planes(flat, off, q, 31, r1 - r0, c1 - c0)
    for n in M.NAMES:
        assert np.array_equal(got[n].view(np.uint64), want[n].view(np.uint64)), (q, n)
print("STATS", int(stats[0]), int(stats[1]), int(stats[2]))
"""


@pytest.mark.parametrize("slab", [None, "150000"], ids=["default_slab", "pieces_cut_in_time"])
def test_fallback_without_top_table_in_a_child_process(slab):
    """No side-16 tables: every piece takes the window walk.  With a slab of 150 000 cells the 8 x 256 x 200 pieces of the first cube
    (409 600 cells) are cut in time, two instants a slab, and the smaller ones share slabs."""
    env = dict(os.environ, K2R_NO_TOP_TABLE="1")
    if slab:
        env["K2R_REDUCE_SLAB_CELLS"] = slab
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    vol = 12 * 300 * 200 + 8 * 273 * 128
    assert "STATS 0 %d 0" % vol in out.stdout, out.stdout[-500:]


def test_errors(dc, rasters):
    from dcdf_amd import _lib as L
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(64, dtype=np.float64)
    off = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()

    def call(h, cubes, nq, ops, outp, offp, mem=L.MEM_HOST):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        return lib.dcdf_raster_reduce_time_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops), outp, mem, offp,
                                                 C.c_void_p(stats.ctypes.data), C.byref(ms))

    o, f = C.c_void_p(out.ctypes.data), C.c_void_p(off.ctypes.data)
    small = [[0, 3, 0, 2, 0, 2]]
    assert call(R._handle(), small, 1, 4 | 8, o, f) == 0 and int(stats.sum()) == 12
    np.testing.assert_array_equal(out[:4], a[0:3, :2, :2].sum(0).ravel())
    np.testing.assert_array_equal(out[4:8], [3, 3, 3, 3])
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, 1, o, f) == -5  # DCDF_ERR_BOUNDS
    for ops in (0, 32, 33, 1 << 20):
        assert call(R._handle(), small, 1, ops, o, f) == -1          # no statistic, or a bit above 16: DCDF_ERR_BAD_ARG
    assert call(R._handle(), small, 1, 1, o, f, mem=7) == -1
    assert call(None, small, 1, 1, o, f) == -1                       # NULL arguments
    assert call(R._handle(), None, 1, 1, o, f) == -1
    assert call(R._handle(), small, 1, 1, None, f) == -1
    assert call(R._handle(), small, 1, 1, o, None) == -1
    assert call(R._handle(), small, 0, 1, o, f) == 0                 # nq == 0 is fine
    # stats and kernel_ms may be NULL; an empty cube writes nothing
    q = np.array([[2, 2, 0, 5, 0, 5]], dtype=np.uint32)
    out[:] = -1
    assert lib.dcdf_raster_reduce_time_batch(R._handle(), C.c_void_p(q.ctypes.data), C.c_size_t(1), C.c_uint32(31), o, L.MEM_HOST, f, None, None) == 0
    assert (out == -1).all()
    q = np.array([[0, 2, 0, 1, 0, 1]], dtype=np.uint32)
    assert lib.dcdf_raster_reduce_time_batch(R._handle(), C.c_void_p(q.ctypes.data), C.c_size_t(1), C.c_uint32(16), o, L.MEM_HOST, f, None, None) == 0
    assert out[0] == (float(a[0, 0, 0]) + float(a[1, 0, 0])) / 2 and (out[1:] == -1).all()


def test_unsupported_arity(dc):
    """A raster holding a k * k > 64 chunk: DCDF_ERR_UNSUPPORTED, as decode."""
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R = BD.build_raster(dc, a, 20, 4, k=9)
    with pytest.raises(L.DcdfError) as e:
        R.reduce_time_flat([[0, 4, 0, 20, 0, 20]], ALL)
    assert e.value.code == -8
    with pytest.raises(L.DcdfError) as e:
        R.decode_flat([[0, 4, 0, 20, 0, 20]], dtype=np.int32)
    assert e.value.code == -8
    R.close()
