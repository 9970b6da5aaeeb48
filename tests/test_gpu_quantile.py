"""Quantiles over time (dcdf_raster_quantile_time_batch, EncodedRaster.quantile_time / quantile_time_flat, Variable.quantile_time) on
the GPU.  The result is exact, so every comparison is on bit patterns (float64 viewed as uint64, NaN equal to NaN) against the
NumPy model of quantile_model.py applied to the array the raster holds (or to what the oracle / window() returns): one sort per
cell with NaN last, then the rank rule of the contract."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import quantile_model as M
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
from bulk_model import leaf_kinds_array

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPE, TILE, CS = RT.SHAPE, RT.TILE, RT.CS  # (20, 264, 264), 256, 8: three segments, bulk chunks and the 8 x 8 corner chunk
PROBS = [0, 0.1, 0.5, 0.9, 1]
METHODS = ("lower", "higher", "nearest", "linear")


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
            a = RT.source(kind)  # (float sources: cells with no value and with one, in bulk chunks and in the corner chunk)
            made[kind] = (a, BD.build_raster(dc, a, TILE, CS))
        return made[kind]

    yield get
    for _, r in made.values():
        r.close()


norm = RT.norm


def check_cube(flat, off, q, probs, method, cube, a):
    """Cube q of a quantile_time_flat result equals the model on the array `a` the raster holds."""
    t0, t1, r0, r1, c0, c1 = norm(cube)
    if (t1 - t0) * (r1 - r0) * (c1 - c0) == 0:
        return
    M.same_bits(M.planes(flat, off, q, len(probs), r1 - r0, c1 - c0), M.quantile_time(a[t0:t1, r0:r1, c0:c1], probs, method))


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_segments_and_methods(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    for t0, t1 in ((0, T), (5, 17), (3, 4)):  # whole; from the middle of a block across two segment boundaries; one instant
        cubes = [[t0, t1, 0, Rr, 0, Cc]] * 2
        _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
        v, n = M.sorted_values(a[t0:t1])  # one sort for the four methods
        rt, rto, _, _ = R.reduce_time_flat(cubes[:1], ("min", "max"))
        mn, mx = rt[:Rr * Cc].reshape(Rr, Cc), rt[Rr * Cc:2 * Rr * Cc].reshape(Rr, Cc)
        for method in METHODS:
            flat, off, ms, stats = R.quantile_time_flat(cubes, PROBS, method)
            assert ms > 0 and flat.dtype == np.float64 and flat.size == 2 * 5 * Rr * Cc and off.tolist() == [0, 5 * Rr * Cc]
            want = M.from_sorted(v, n, PROBS, method)
            for q in range(2):
                M.same_bits(M.planes(flat, off, q, 5, Rr, Cc), want)
            np.testing.assert_array_equal(stats, dstats)
            assert int(stats[0]) > 0 and int(stats[1]) == 2 * (t1 - t0) * 8 * 8 and int(stats[2]) == 0
            # p = 0 and p = 1 are reduce_time's MIN and MAX (==: apart from the sign of a zero; NaN where nothing was counted)
            got = M.planes(flat, off, 0, 5, Rr, Cc)
            np.testing.assert_array_equal(got[0], mn)
            np.testing.assert_array_equal(got[4], mx)
        if t1 - t0 > 1:
            assert (want[1] != want[3]).any() and (n == t1 - t0).any()
            if kind[0] == "f":
                assert np.isnan(want[2][17, 23]) and np.isnan(want[2][258, 259]) and (n < t1 - t0).any()
    d = R.quantile_time([0.25, 0.75], 2, 19, window=(250, 264, 3, 264), method="nearest")
    M.same_bits(d, M.quantile_time(a[2:19, 250:264, 3:264], [0.25, 0.75], "nearest"))
    d = R.quantile_time(0.5, 1, 20)
    assert d.shape == (Rr, Cc)
    M.same_bits(d, M.quantile_time(a[1:20], [0.5])[0])
    # sixteen probabilities, some repeated: the kernel's largest form
    many = list(np.linspace(0, 1, 13)) + [0.5, 0.5, 0.05]
    flat, off, _, _ = R.quantile_time_flat([[0, T, 200, 264, 190, 264]], many, "linear")
    check_cube(flat, off, 0, many, "linear", [0, T, 200, 264, 190, 264], a)


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_unaligned_batch(rasters, kind):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters(kind)
    rng = np.random.default_rng(500 + len(kind))  # (the cubes of the reduce_time test, reversed bounds among them)
    cubes = BD.random_cubes(rng, SHAPE, 100)
    cubes[0] = [0, SHAPE[0], 0, SHAPE[1], 0, SHAPE[2]]
    cubes[1] = [3, 4, 7, 8, 9, 10]                 # one cell, one instant
    cubes[2] = [9, 10, 0, SHAPE[1], 0, SHAPE[2]]   # one instant
    cubes[3] = [0, SHAPE[0], 261, 262, 130, 131]   # one cell
    cubes[4] = [6, 6, 0, 30, 0, 30]                # no instants: writes nothing
    probs = [0.9, 0.5, 0.02]                       # (planes in the order of probs, not sorted)
    flat, off, _, stats = R.quantile_time_flat(cubes, probs, "linear")
    _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
    np.testing.assert_array_equal(stats, dstats)
    for q, c in enumerate(cubes):
        check_cube(flat, off, q, probs, "linear", c, a)
    # device form: odd gaps between the windows, a sentinel everywhere first
    nb = np.array([norm(c) for c in cubes], dtype=np.int64)
    vol = (3 * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64))
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1]) + 7
    buf = DeviceBuffer(total * 8)
    buf.write(0, np.full(total, -77.25, dtype=np.float64))
    ms, dvstats = R.quantile_time_flat(cubes, probs, "linear", out_device_ptr=buf.ptr, out_offset=doff)
    g = buf.read(0, total * 8, np.float64)
    buf.free()
    np.testing.assert_array_equal(dvstats, stats)
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        o, m = int(doff[q]), int(vol[q])
        inside[o:o + m] = True
        M.same_bits(g[o:o + m], flat[int(off[q]):int(off[q]) + m])
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
    for method in ("linear", "nearest"):
        flat, off, _, stats = R.quantile_time_flat(cubes, PROBS, method)
        assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0
        for q, c in enumerate(cubes.astype(int)):
            M.same_bits(M.planes(flat, off, q, 5, c[3] - c[2], c[5] - c[4]), M.quantile_time(oc.fill_window(*c, dtype=np.int64), PROBS, method))
    R.close()


def test_62_fractional_bits(dc):
    """A float64 leaf with 62 fractional bits inside +-2^30 (the histogram test's chunk): the decoded value falls as the stored
    integer rises -- the keys are formed of the widened value, never of the stored integer."""
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(6262)
    m = rng.integers(-(2 ** 28), 2 ** 28, size=(8, 64, 64))  # (stored: 2 m + 1)
    m[:, 10:20, 30:50] = 12345
    m[2:5, 40:44, 3:9] = 0
    x = m / 2.0 ** 62
    (b,) = dc.build_batch([np.ascontiguousarray(x)], k=2, fractional_bits=62)
    assert not isinstance(b, Exception)
    R = EncodedRaster(x.shape, [b.data], tile=64, chunk_size=8)
    a = R.decode(dtype=np.float64)
    assert not np.isnan(a).any() and (a == -x).all()
    cubes = [[0, 8, 0, 64, 0, 64], [1, 7, 3, 53, 2, 63]]
    for method in METHODS:
        flat, off, _, stats = R.quantile_time_flat(cubes, PROBS, method)
        assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0 and int(stats[2]) == 0
        for q, c in enumerate(cubes):
            check_cube(flat, off, q, PROBS, method, c, a)
    R.close()


def test_fallbacks_k3_and_wide_values(dc):
    from dcdf_amd import synth
    a3 = synth.cells(BD.SEED, 0, 10, 0, 100, 0, 90, np.int32)
    R3 = BD.build_raster(dc, a3, 64, 8, k=3)
    wide = synth.cells(BD.SEED, 0, 10, 0, 100, 0, 90, np.int64)
    for r, c in ((5, 7), (5, 80), (70, 7)):    # beyond 2^30 in every chunk of the grid (tile 64): the 64-bit walk
        wide[:, r, c] += 2 ** 30 + 12345
    wide[:, 70, 80] = -(2 ** 35)
    wide[:, 71, 80] = 2 ** 53 + 1 + 2 * np.arange(10)  # odd beyond 2^53: every one rounds when widened
    Rw = BD.build_raster(dc, wide, 64, 8)
    rng = np.random.default_rng(5)
    for R, a in ((R3, a3), (Rw, wide)):
        cubes = np.concatenate([[[0, 10, 0, 100, 0, 90]], BD.random_cubes(rng, a.shape, 30)]).astype(np.uint32)
        for method in ("linear", "higher"):
            flat, off, _, stats = R.quantile_time_flat(cubes, PROBS, method)
            assert int(stats[0]) == 0 and int(stats[1]) == BD.volume(cubes)
            for q, c in enumerate(cubes):
                check_cube(flat, off, q, PROBS, method, c, a)
        R.close()


def test_segments_of_one_cell_with_different_fractional_bits(dc, dtype=np.float64):
    """Three segments built apart with 0, 25 and 12 fractional bits (the reduce_time test's raster): the same stored integer means
    another value in every segment, so the keys must be formed per segment."""
    a, chunks, EncodedRaster = RT.order_raster(dc, dtype)
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    got = R.decode(dtype=dtype)
    assert got.dtype == a.dtype and (got == a).all()
    # were the stored integers compared, the order would be another: some cell's median differs
    stored_order = np.concatenate([a[0:8], a[8:16] * 2.0 ** 25, a[16:24] * 2.0 ** 12]).astype(np.float64)
    pick = np.take_along_axis(M.widen(a), np.argsort(stored_order, axis=0, kind="stable")[11:12], 0)[0]
    assert (pick != M.quantile_time(a, [0.5], "lower")[0]).any(), "the order of the stored integers is the order of the values: the input proves nothing"
    cubes = [[0, 24, 0, 64, 0, 64], [3, 21, 5, 64, 0, 59], [8, 24, 0, 64, 0, 64]]
    for method in METHODS:
        flat, off, _, stats = R.quantile_time_flat(cubes, PROBS, method)
        assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0
        for q, c in enumerate(cubes):
            check_cube(flat, off, q, PROBS, method, c, a)
    R.close()


CHILD = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import dcdf_amd
import quantile_model as M
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
assert os.environ["K2R_QUANTILE_SLAB_BYTES"] == "400000"
a = RT.source("f32")
R = BD.build_raster(dcdf_amd, a, RT.TILE, RT.CS)
T, Rr, Cc = RT.SHAPE
cubes = [[0, T, 0, Rr, 0, Cc], [3, 19, 17, 260, 5, 133]]
probs = [0, 0.1, 0.5, 0.9, 1]
# 400 000 bytes: 2 500 cells of 20 instants.  The 256 x 256 columns are cut into 64 x 64 parts of 655 360 bytes, each over the cap
# and alone in its band; the 8-row and 8-column strips (2 048 cells) fit whole, one a band; the corner chunk shares one.
small = {m: R.quantile_time_flat(cubes, probs, m) for m in ("linear", "nearest")}
del os.environ["K2R_QUANTILE_SLAB_BYTES"]
for m, (flat, off, _, stats) in small.items():
    dflat, doff, _, dstats = R.quantile_time_flat(cubes, probs, m)
    assert np.array_equal(off, doff) and np.array_equal(stats, dstats)
    M.same_bits(flat, dflat)
    for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes):
        M.same_bits(M.planes(flat, off, q, 5, r1 - r0, c1 - c0), M.quantile_time(a[t0:t1, r0:r1, c0:c1], probs, m))
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
    got = v.quantile_time(PROBS)
    M.same_bits(got, M.quantile_time(v.window(0, T, 0, Rr, 0, Cc), PROBS))
    win = (7, T - 1, 5, Rr - 3, 250, Cc - 9)
    got = v.quantile_time([0.9, 0.1], *win, method="higher")
    M.same_bits(got, M.quantile_time(v.window(*win), [0.9, 0.1], "higher"))
    med = v.quantile_time(0.5, method="lower")
    assert med.shape == (Rr, Cc)
    M.same_bits(med, M.quantile_time(v.window(0, T, 0, Rr, 0, Cc), [0.5], "lower")[0])
    _, _, _, stats = v.raster().quantile_time_flat([[0, T, 0, Rr, 0, Cc]], [0.5])
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    none = v.quantile_time([0.1, 0.5], 4, 4)
    assert none.shape == (2, Rr, Cc) and np.isnan(none).all()
    with pytest.raises(IndexError):
        v.quantile_time(0.5, stop=T + 1)
    with pytest.raises(IndexError):
        v.quantile_time(0.5, right=Cc + 1)
    with pytest.raises(ValueError):
        v.quantile_time(1.5)


def test_errors(dc, rasters):
    from dcdf_amd import _lib as L
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(64, dtype=np.float64)
    off = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()
    half = np.array([0.5, 0.0])

    def call(h, cubes, nq, outp, offp, probs=half, n_probs=2, method=0, mem=L.MEM_HOST):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        p = None if probs is None else np.ascontiguousarray(np.asarray(probs, dtype=np.float64))
        return lib.dcdf_raster_quantile_time_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq),
                                                   None if p is None else C.c_void_p(p.ctypes.data), C.c_uint32(n_probs), C.c_int32(method), outp, mem,
                                                   offp, C.c_void_p(stats.ctypes.data), C.byref(ms))

    o, f = C.c_void_p(out.ctypes.data), C.c_void_p(off.ctypes.data)
    small = [[0, 3, 0, 2, 0, 2]]
    assert call(R._handle(), small, 1, o, f) == 0 and int(stats.sum()) == 12
    np.testing.assert_array_equal(out[:4], np.sort(a[0:3, :2, :2], axis=0)[1].ravel())  # LOWER at 0.5 of three: the middle one
    np.testing.assert_array_equal(out[4:8], a[0:3, :2, :2].min(0).ravel())
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, o, f) == -5  # DCDF_ERR_BOUNDS
    assert call(R._handle(), small, 1, o, f, probs=[0.5, np.nan]) == -1   # a NaN probability: DCDF_ERR_BAD_ARG
    assert call(R._handle(), small, 1, o, f, probs=[1.5, 0.5]) == -1      # outside [0, 1]
    assert call(R._handle(), small, 1, o, f, probs=[0.5, -0.25]) == -1
    assert call(R._handle(), small, 1, o, f, n_probs=0) == -1
    assert call(R._handle(), small, 1, o, f, probs=np.linspace(0, 1, 17), n_probs=17) == -1
    for method in (4, -1, 1 << 20):
        assert call(R._handle(), small, 1, o, f, method=method) == -1
    assert call(R._handle(), small, 1, o, f, mem=7) == -1
    assert call(None, small, 1, o, f) == -1                       # NULL arguments
    assert call(R._handle(), None, 1, o, f) == -1
    assert call(R._handle(), small, 1, o, f, probs=None) == -1
    assert call(R._handle(), small, 1, None, f) == -1
    assert call(R._handle(), small, 1, o, None) == -1
    assert call(R._handle(), small, 0, o, f) == 0                 # nq == 0 is fine
    # stats and kernel_ms may be NULL; an empty cube writes nothing
    q = np.array([[2, 2, 0, 5, 0, 5]], dtype=np.uint32)
    out[:] = -1
    assert lib.dcdf_raster_quantile_time_batch(R._handle(), C.c_void_p(q.ctypes.data), C.c_size_t(1), C.c_void_p(half.ctypes.data), C.c_uint32(2),
                                               C.c_int32(3), o, L.MEM_HOST, f, None, None) == 0
    assert (out == -1).all()
    q = np.array([[2, 0, 1, 0, 1, 0]], dtype=np.uint32)  # reversed bounds: the one cell's instants 0 and 1
    assert lib.dcdf_raster_quantile_time_batch(R._handle(), C.c_void_p(q.ctypes.data), C.c_size_t(1), C.c_void_p(half.ctypes.data), C.c_uint32(1),
                                               C.c_int32(3), o, L.MEM_HOST, f, None, None) == 0
    assert out[0] == (float(a[0, 0, 0]) + float(a[1, 0, 0])) / 2 and (out[1:] == -1).all()


def test_unsupported_arity(dc):
    """A raster holding a k * k > 64 chunk: DCDF_ERR_UNSUPPORTED, as decode."""
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R = BD.build_raster(dc, a, 20, 4, k=9)
    with pytest.raises(L.DcdfError) as e:
        R.quantile_time_flat([[0, 4, 0, 20, 0, 20]], PROBS)
    assert e.value.code == -8
    R.close()
