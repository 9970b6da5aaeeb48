"""Spell statistics (dcdf_raster_spells_batch, EncodedRaster.spells / spells_flat, Variable.spells) on the GPU.  Every result is an
integer and every comparison exact, against the NumPy model of spell_model.py applied to the array the raster holds (or to what
the oracle / window() returns): the hit rule of value search, then one sequential fold per cell."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import spell_model as M
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
from bulk_model import leaf_kinds_array

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ALL = 31
SHAPE, TILE, CS = RT.SHAPE, RT.TILE, RT.CS  # (20, 264, 264), 256, 8: three segments, bulk chunks and the 8 x 8 corner chunk
INF = float("inf")


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
            a = RT.source(kind)  # (float sources: the extra NaN cells of the reduce_time test)
            made[kind] = (a, BD.build_raster(dc, a, TILE, CS))
        return made[kind]

    yield get
    for _, r in made.values():
        r.close()


norm = RT.norm


def same(got, want):
    assert got.dtype == np.uint32 and want.dtype == np.uint32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def check_cube(flat, off, q, mask, cube, a, lower, upper):
    """Cube q of a spells_flat result equals the model on the array `a` the raster holds."""
    t0, t1, r0, r1, c0, c1 = norm(cube)
    if (t1 - t0) * (r1 - r0) * (c1 - c0) == 0:
        return None
    want = M.spells(M.hits(a[t0:t1, r0:r1, c0:c1], lower, upper))
    got = M.planes(flat, off, q, mask, r1 - r0, c1 - c0)
    assert list(got) == M.names_of(mask)
    for n in got:
        same(got[n], want[n])
    return want


def bound_pairs(a):
    """The one-sided bound of the host test, and a two-sided band between the quartiles."""
    q25, q50, q75 = (float(x) for x in np.nanpercentile(a, [25, 50, 75]))
    return [q50 + 0.5, q25 + 0.5], [INF, q75 + 0.5]


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_segments_and_blocks(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    lower, upper = bound_pairs(a)
    for t0, t1 in ((0, T), (5, 17), (3, 4)):  # whole; from the middle of a block across two segment boundaries; one instant
        cubes = [[t0, t1, 0, Rr, 0, Cc]] * 2
        _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
        # all five; COUNT alone; LONGEST_START alone (cur and LONGEST in scratch planes); FIRST | LAST
        for mask in (ALL, 1, 4, 24):
            flat, off, ms, stats = R.spells_flat(cubes, lower, upper, mask)
            n = bin(mask).count("1")
            assert ms > 0 and flat.dtype == np.uint32 and flat.size == 2 * n * Rr * Cc and off.tolist() == [0, n * Rr * Cc]
            for q in range(2):
                want = check_cube(flat, off, q, mask, cubes[q], a, lower[q], upper[q])
                if mask == ALL and t1 - t0 > 1:
                    assert 0 < want["count"].sum() < (t1 - t0) * Rr * Cc and (want["longest"] > 1).any()
            np.testing.assert_array_equal(stats, dstats)
            assert int(stats[0]) > 0 and int(stats[1]) == 2 * (t1 - t0) * 8 * 8 and int(stats[2]) == 0
    d = R.spells(lower[1], upper[1], ("last", "longest"), 2, 19, window=(250, 264, 3, 264))
    want = M.spells(M.hits(a[2:19, 250:264, 3:264], lower[1], upper[1]))
    assert list(d) == ["longest", "last"]
    same(d["longest"], want["longest"])
    same(d["last"], want["last"])


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_every_instantiation_of_the_shared_fold(dc, kind):
    """Every `ops` in 1 .. 31: k_bulk_spell<GROUPS> for GROUPS 1 .. 7 with every choice of scratch planes, and the per-cell fold kernel,
    on the small raster of the reduce_time test: a whole cube and one unaligned in every edge with planes of an odd size."""
    a = RT.fold_source(kind)
    R = BD.build_raster(dc, a, RT.FOLD_TILE, RT.FOLD_CS)
    cubes = RT.FOLD_CUBES
    lower, upper = bound_pairs(a)  # (one pair per cube)
    want = [M.spells(M.hits(a[t0:t1, r0:r1, c0:c1], lower[q], upper[q])) for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes)]
    for w, c in zip(want, cubes):
        assert 0 < w["count"].sum() < BD.volume([c]) and (w["longest"] > 1).any() and (w["longest"] < w["count"]).any()
    for ops in range(1, 32):
        flat, off, _, stats = R.spells_flat(cubes, lower, upper, ops)
        assert int(stats[0]) > 0 and int(stats[1]) > 0 and int(stats.sum()) == BD.volume(cubes)
        for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes):
            got = M.planes(flat, off, q, ops, r1 - r0, c1 - c0)
            assert list(got) == M.names_of(ops)
            for n in got:
                same(got[n], want[q][n])
    R.close()


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_cross_checks_with_search_values_and_reduce_time(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    lower, upper = bound_pairs(a)
    cube = [3, 18, 40, 264, 131, 264]  # bulk chunks, both strips and the corner chunk
    t0, t1, r0, r1, c0, c1 = cube
    for lo, hi in zip(lower, upper):
        flat, off, _, _ = R.spells_flat([cube], lo, hi, "count")
        trip, offs, counts, _ = R.search_values_flat([cube], lo, hi)
        tr = trip[:int(counts[0])].astype(np.int64)
        per_cell = np.bincount((tr[:, 1] - r0) * (c1 - c0) + (tr[:, 2] - c0), minlength=(r1 - r0) * (c1 - c0))
        assert int(counts[0]) > 0
        np.testing.assert_array_equal(flat, per_cell.astype(np.uint32))  # a hit is exactly a cell value search reports
    whole = [0, T, 0, Rr, 0, Cc]
    flat, off, _, _ = R.spells_flat([whole], -INF, INF, ("count", "longest"))
    got = M.planes(flat, off, 0, 3, Rr, Cc)
    rt = R.reduce_time("count")["count"]
    np.testing.assert_array_equal(got["count"], rt.astype(np.uint32))
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        assert (got["longest"][~nan.any(0)] == T).all()
        assert got["longest"][200, 5] == 1 and got["longest"][17, 23] == 0 and got["longest"][260, 261] == 1  # (a NaN instant breaks the run)
        broken = nan.any(0) & ~nan.all(0)
        assert (got["longest"][broken] < T).all() and broken.sum() > 100
    else:
        assert (got["longest"] == T).all()


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_unaligned_batch(rasters, kind):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters(kind)
    rng = np.random.default_rng(700 + len(kind))
    n = 100
    cubes = BD.random_cubes(rng, SHAPE, n)
    cubes[0] = [0, SHAPE[0], 0, SHAPE[1], 0, SHAPE[2]]
    cubes[1] = [3, 4, 7, 8, 9, 10]                 # one cell, one instant
    cubes[2] = [9, 10, 0, SHAPE[1], 0, SHAPE[2]]   # one instant
    cubes[3] = [0, SHAPE[0], 261, 262, 130, 131]   # one cell
    cubes[4] = [6, 6, 0, 30, 0, 30]                # no instants: writes nothing
    cubes[5] = [0, SHAPE[0], 100, 264, 200, 264]
    cubes[6] = [2, 19, 0, 264, 250, 264]
    # per-cube bounds around the data's quantiles, one-sided and two-sided, some reversed
    qs = np.nanpercentile(a, np.arange(5, 100, 5))
    lower = rng.choice(qs, n) + 0.5
    upper = np.where(rng.random(n) < 0.4, INF, lower + rng.choice(qs[10:] - qs[9], n))
    lower[rng.random(n) < 0.1] = -INF
    swap = rng.random(n) < 0.15
    lower[swap], upper[swap] = upper[swap], lower[swap]
    lower[5] = upper[5] = 0.5          # nothing hits on an integer raster
    lower[6], upper[6] = 2.0 ** 40, INF  # beyond int32 in stored integers
    mask = 29  # count, longest_start, first, last: LONGEST and cur live in scratch planes
    flat, off, _, stats = R.spells_flat(cubes, lower, upper, mask)
    _, _, _, dstats = R.decode_flat(cubes, dtype=a.dtype)
    np.testing.assert_array_equal(stats, dstats)
    some = 0
    for q, c in enumerate(cubes):
        want = check_cube(flat, off, q, mask, c, a, lower[q], upper[q])
        some += want is not None and 0 < int(want["count"].sum())
    assert some > 30
    got6 = M.planes(flat, off, 6, mask, 264, 14)
    assert (got6["count"] == 0).all() and all((got6[k] == M.NONE).all() for k in ("longest_start", "first", "last"))
    if kind == "i32":
        assert (M.planes(flat, off, 5, mask, 164, 64)["count"] == 0).all()
    # device form: odd gaps between the windows, a sentinel everywhere first
    nb = np.array([norm(c) for c in cubes], dtype=np.int64)
    vol = (4 * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64))
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1]) + 7
    SENT = 0x7e57ab1e
    buf = DeviceBuffer(total * 4)
    buf.write(0, np.full(total, SENT, dtype=np.uint32))
    ms, dvstats = R.spells_flat(cubes, lower, upper, mask, out_device_ptr=buf.ptr, out_offset=doff)
    g = buf.read(0, total * 4, np.uint32)
    buf.free()
    np.testing.assert_array_equal(dvstats, stats)
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        o, m = int(doff[q]), int(vol[q])
        inside[o:o + m] = True
        np.testing.assert_array_equal(g[o:o + m], flat[int(off[q]):int(off[q]) + m])
    assert (g[~inside] == SENT).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's planes


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
    med = float(np.median(a))
    for lo, hi in ((med, INF), (-INF, med), (med, med)):
        flat, off, _, stats = R.spells_flat(cubes, lo, hi, ALL)
        assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0
        for q, c in enumerate(cubes.astype(int)):
            want = M.spells(M.hits(oc.fill_window(*c, dtype=np.int64), lo, hi))
            got = M.planes(flat, off, q, ALL, c[3] - c[2], c[5] - c[4])
            for n in M.NAMES:
                same(got[n], want[n])
    R.close()


def test_62_fractional_bits_in_the_bulk_kernel(dc):
    """A float64 leaf with 62 fractional bits inside +-2^30 (the histogram test's chunk): the decoded value falls as the stored
    integer rises, and the band around zero holds the NaN code's place."""
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
    band = 2.0 ** -36
    cubes = [[0, 8, 0, 64, 0, 64], [1, 7, 3, 53, 2, 63], [0, 8, 0, 64, 0, 64], [0, 8, 0, 64, 0, 64]]
    lower, upper = [-band, -band, 0.0, -INF], [band, 3 * band, INF, -12345 / 2.0 ** 62]
    flat, off, _, stats = R.spells_flat(cubes, lower, upper, ALL)
    assert int(stats[0]) == BD.volume(cubes) and int(stats[1]) == 0 and int(stats[2]) == 0
    for q, c in enumerate(cubes):
        want = check_cube(flat, off, q, ALL, c, a, lower[q], upper[q])
        assert 0 < want["count"].sum() < BD.volume([c])
    R.close()


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
        med = float(np.median(a))
        for lo, hi in ((-(2.0 ** 34), 2.0 ** 30 + 0.5), (med + 0.5, INF)):
            flat, off, _, stats = R.spells_flat(cubes, lo, hi, ALL)
            assert int(stats[0]) == 0 and int(stats[1]) == BD.volume(cubes)
            for q, c in enumerate(cubes):
                check_cube(flat, off, q, ALL, c, a, lo, hi)
        if a is wide:
            got = M.planes(*R.spells_flat(cubes[:1], -(2.0 ** 34), 2.0 ** 30 + 0.5, 1)[:2], 0, 1, 100, 90)["count"]
            assert got[5, 7] == 0 and got[70, 80] == 0 and got[0, 0] == 10
        R.close()


CHILD = r"""
import itertools, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import dcdf_amd
import spell_model as M
from dcdf_amd import synth
from dcdf_amd.raster import EncodedRaster
a = synth.cells(0xDCDF0011, 0, 12, 0, 300, 0, 200, np.int32)
grid = EncodedRaster.chunk_grid(a.shape, 256, 8)
R = EncodedRaster(a.shape, [b.data for b in dcdf_amd.build_batch([np.ascontiguousarray(a[t0:t1, r0:r1, c0:c1]) for t0, t1, r0, r1, c0, c1 in grid])], 256, 8)
cubes = [[0, 12, 0, 300, 0, 200], [3, 11, 17, 290, 5, 133]]
lower = float(np.median(a)) + 0.5
h = M.hits(a, lower, np.inf)
w = M.spells(h)
s, n = w["longest_start"].astype(np.int64), w["longest"].astype(np.int64)
crosses = (n > 0) & np.any([(s < cut) & (s + n > cut) for cut in (2, 4, 6)], axis=0)
assert crosses.any(), "no longest run crosses a slab cut: the input proves nothing"
tied = 0
for r in range(0, 300, 7):
    for c in range(0, 200, 5):
        runs = [len(list(g)) for hit, g in itertools.groupby(h[:, r, c].tolist()) if hit]
        tied += bool(runs) and runs.count(max(runs)) > 1
assert tied > 0, "no cell with tied runs"
flat, off, _, stats = R.spells_flat(cubes, lower, np.inf, 31)
for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes):
    want = M.spells(h[t0:t1, r0:r1, c0:c1])
    got = M.planes(flat, off, q, 31, r1 - r0, c1 - c0)
    for n in M.NAMES:
        assert np.array_equal(got[n], want[n]), (q, n)
flat, off, _, _ = R.spells_flat(cubes, lower, np.inf, 4)
for q, (t0, t1, r0, r1, c0, c1) in enumerate(cubes):
    assert np.array_equal(M.planes(flat, off, q, 4, r1 - r0, c1 - c0)["longest_start"], M.spells(h[t0:t1, r0:r1, c0:c1])["longest_start"]), q
print("STATS", int(stats[0]), int(stats[1]), int(stats[2]))
"""


@pytest.mark.parametrize("slab", [None, "150000"], ids=["default_slab", "pieces_cut_in_time"])
def test_fallback_without_top_table_in_a_child_process(slab):
    """No side-16 tables: every piece takes the window walk and k_cell_fold.  With a slab of 150 000 cells the 8 x 256 x 200 pieces
    of the first cube are cut in time, two instants a slab: runs cross slab cuts inside a segment."""
    env = dict(os.environ, K2R_NO_TOP_TABLE="1")
    if slab:
        env["K2R_REDUCE_SLAB_CELLS"] = slab
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    vol = 12 * 300 * 200 + 8 * 273 * 128
    assert "STATS 0 %d 0" % vol in out.stdout, out.stdout[-500:]


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
    med = float(np.nanmedian(a))
    got = v.spells(med, INF, M.NAMES)
    want = M.spells(M.hits(v.window(0, T, 0, Rr, 0, Cc), med, INF))
    assert list(got) == list(M.NAMES) and 0 < want["count"].sum() < a.size
    for n in M.NAMES:
        same(got[n], want[n])
    win = (7, T - 1, 5, Rr - 3, 250, Cc - 9)
    got = v.spells(-INF, med, ("last", "longest_start"), *win)
    want = M.spells(M.hits(v.window(*win), -INF, med))
    assert list(got) == ["longest_start", "last"]
    same(got["longest_start"], want["longest_start"])
    same(got["last"], want["last"])
    assert list(v.spells(med, INF)) == ["count", "longest"]
    _, _, _, stats = v.raster().spells_flat([[0, T, 0, Rr, 0, Cc]], med, INF, ALL)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    none = v.spells(med, INF, ("count", "first"), 4, 4)
    assert none["count"].shape == (Rr, Cc) and (none["count"] == 0).all() and (none["first"] == M.NONE).all()
    with pytest.raises(IndexError):
        v.spells(med, INF, stop=T + 1)
    with pytest.raises(IndexError):
        v.spells(med, INF, right=Cc + 1)


def test_errors(dc, rasters):
    from dcdf_amd import _lib as L
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(64, dtype=np.uint32)
    off = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()
    lo1, hi1 = np.array([-INF]), np.array([INF])

    def call(h, cubes, nq, ops, outp, offp, mem=L.MEM_HOST, lo=lo1, hi=hi1):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        return lib.dcdf_raster_spells_batch(h, None if q is None else C.c_void_p(q.ctypes.data), None if lo is None else C.c_void_p(lo.ctypes.data),
                                            None if hi is None else C.c_void_p(hi.ctypes.data), C.c_size_t(nq), C.c_uint32(ops), outp, mem, offp,
                                            C.c_void_p(stats.ctypes.data), C.byref(ms))

    o, f = C.c_void_p(out.ctypes.data), C.c_void_p(off.ctypes.data)
    small = [[0, 3, 0, 2, 0, 2]]
    assert call(R._handle(), small, 1, 1 | 16, o, f) == 0 and int(stats.sum()) == 12
    np.testing.assert_array_equal(out[:8], [3, 3, 3, 3, 2, 2, 2, 2])
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, 1, o, f) == -5  # DCDF_ERR_BOUNDS
    for ops in (0, 32, 33, 1 << 20):
        assert call(R._handle(), small, 1, ops, o, f) == -1          # no statistic, or a bit above 16: DCDF_ERR_BAD_ARG
    nan = np.array([np.nan])
    assert call(R._handle(), small, 1, 1, o, f, lo=nan) == -1        # a NaN bound
    assert call(R._handle(), small, 1, 1, o, f, hi=nan) == -1
    assert call(R._handle(), small, 1, 1, o, f, mem=7) == -1
    assert call(None, small, 1, 1, o, f) == -1                       # NULL arguments
    assert call(R._handle(), None, 1, 1, o, f) == -1
    assert call(R._handle(), small, 1, 1, o, f, lo=None) == -1
    assert call(R._handle(), small, 1, 1, o, f, hi=None) == -1
    assert call(R._handle(), small, 1, 1, None, f) == -1
    assert call(R._handle(), small, 1, 1, o, None) == -1
    assert call(R._handle(), small, 0, 1, o, f) == 0                 # nq == 0 is fine
    # stats and kernel_ms may be NULL; an empty cube writes nothing; reversed value bounds are swapped
    q = np.array([[2, 2, 0, 5, 0, 5]], dtype=np.uint32)
    out[:] = 77
    assert lib.dcdf_raster_spells_batch(R._handle(), C.c_void_p(q.ctypes.data), C.c_void_p(lo1.ctypes.data), C.c_void_p(hi1.ctypes.data), C.c_size_t(1),
                                        C.c_uint32(31), o, L.MEM_HOST, f, None, None) == 0
    assert (out == 77).all()
    q = np.array([[0, 2, 0, 1, 0, 1]], dtype=np.uint32)
    v = float(a[1, 0, 0])
    lo, hi = np.array([v + 0.5]), np.array([v - 0.5])
    assert lib.dcdf_raster_spells_batch(R._handle(), C.c_void_p(q.ctypes.data), C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data), C.c_size_t(1),
                                        C.c_uint32(16), o, L.MEM_HOST, f, None, None) == 0
    assert out[0] == 1 and (out[1:] == 77).all()  # LAST of the one cell: instant 1 holds v


def test_unsupported_arity(dc):
    """A raster holding a k * k > 64 chunk: DCDF_ERR_UNSUPPORTED, as decode."""
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R = BD.build_raster(dc, a, 20, 4, k=9)
    with pytest.raises(L.DcdfError) as e:
        R.spells_flat([[0, 4, 0, 20, 0, 20]], 0.0, INF, ALL)
    assert e.value.code == -8
    R.close()
