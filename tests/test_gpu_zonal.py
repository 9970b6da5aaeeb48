"""Zonal statistics (dcdf_raster_zonal_batch, EncodedRaster.zonal / zonal_flat, Variable.zonal) on the GPU.  Every comparison is on
bit patterns against the model of zonal_model.py: zone z is space_model.reduce_space over the cells labelled z, with -0.0 below
+0.0 for the extremes."""
import ctypes as C
import math

import numpy as np
import pytest

import space_model as SM
import test_gpu_bulk_decode as BD
import zonal_model as ZM
from test_gpu_bulk_decode import assert_same
from test_gpu_reduce_space import exact_raster
from test_gpu_reduce_time import SHAPE, TILE, CS, norm, source

pytestmark = pytest.mark.gpu
ALL = 31
NONE = 0xFFFF
NAN_BITS = np.array(np.nan).view(np.uint64)


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


def check(flat, off, q, ops, want, n_zones, nt):
    """Cube q of a zonal_flat result equals the model's matrices `want` (all five; the call's are those of `ops`)."""
    got = ZM.matrices(flat, off, q, ops, n_zones, nt)
    assert list(got) == ZM.names_of(ops)
    for n in got:
        assert_same(np.ascontiguousarray(got[n]), want[n])


def label_sets(rng):
    """Over the whole raster: (labels, n_zones) -- one zone everywhere; the ids of 37 random rectangles, later ones on top, the
    rest NONE; every cell of the 64 x 64 region at (64, 128) -- one unit of the bulk kernel -- a zone of its own, 4096 labels in
    rounds of 16, the rest NONE but for a stripe of labels that name no zone."""
    _, Rr, Cc = SHAPE
    one = np.zeros((Rr, Cc), dtype=np.uint16)
    rects = np.full((Rr, Cc), NONE, dtype=np.uint16)
    for z in range(37):
        r0, c0 = int(rng.integers(0, Rr - 4)), int(rng.integers(0, Cc - 4))
        rects[r0:r0 + int(rng.integers(1, 120)), c0:c0 + int(rng.integers(1, 120))] = z
    own = np.full((Rr, Cc), NONE, dtype=np.uint16)
    own[64:128, 128:192] = np.arange(4096, dtype=np.uint16).reshape(64, 64)
    own[200:210, :] = 5000  # >= n_zones: ignored
    return [(one, 1), (rects, 37), (own, 4096)]


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_cubes_and_label_sets(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    rng = np.random.default_rng(53 + len(kind))
    #        whole raster         segments, the tile edge, 64-regions, odd columns   one instant             one cell
    cubes = [[0, T, 0, Rr, 0, Cc], [5, 17, 250, 264, 3, 264], [9, 10, 0, Rr, 0, Cc], [0, T, 261, 262, 130, 131]]
    for labels, nz in label_sets(rng):
        for cube in cubes:
            t0, t1, r0, r1, c0, c1 = norm(cube)
            if nz == 4096 and cube is cubes[0]:
                t0, t1 = 3, 12  # (the model's 4096 series: nine instants, two segments)
                cube = [t0, t1, r0, r1, c0, c1]
            lab = np.ascontiguousarray(labels[r0:r1, c0:c1])
            want = ZM.zonal(a[t0:t1, r0:r1, c0:c1], lab, nz)
            _, _, _, dstats = R.decode_flat([cube], dtype=a.dtype)
            for ops in (ALL, 1, 16):
                flat, off, ms, stats = R.zonal_flat([cube], ops, [lab], nz)
                assert ms > 0 and flat.size == bin(ops).count("1") * nz * (t1 - t0) and off.tolist() == [0]
                check(flat, off, 0, ops, want, nz, t1 - t0)
                np.testing.assert_array_equal(stats, dstats)  # (the labels do not change them)
    labels, nz = label_sets(rng)[1]
    d = R.zonal(("max", "count"), np.ascontiguousarray(labels[250:264, 3:264]), 2, 19, window=(250, 264, 3, 264))
    want = ZM.zonal(a[2:19, 250:264, 3:264], labels[250:264, 3:264], int(labels[250:264, 3:264][labels[250:264, 3:264] != NONE].max()) + 1)
    assert list(d) == ["max", "count"]
    assert_same(np.ascontiguousarray(d["max"]), want["max"])
    assert_same(np.ascontiguousarray(d["count"]), want["count"])


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_agrees_with_reduce_space(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    rng = np.random.default_rng(7)
    for cube in ([0, T, 0, Rr, 0, Cc], [5, 17, 250, 264, 3, 264]):
        t0, t1, r0, r1, c0, c1 = cube
        nt = t1 - t0
        mask = rng.random((r1 - r0, c1 - c0)) < 0.5
        space, _, _, sstats = R.reduce_space_flat([cube], ALL, [mask])
        flat, off, _, stats = R.zonal_flat([cube], ALL, [np.where(mask, 0, NONE).astype(np.uint16)], 1)
        assert_same(flat, space)  # [5][1][nt] is [5][nt]
        np.testing.assert_array_equal(stats, sstats)
        flat, off, _, _ = R.zonal_flat([cube], ALL, [np.where(mask, 3, 7).astype(np.uint16)], 5)
        m = flat.reshape(5, 5, nt)
        assert_same(np.ascontiguousarray(m[:, 3, :]).ravel(), space)
        for z in (0, 1, 2, 4):  # no cell carries them; label 7 names no zone
            assert (m[[0, 1, 4], z, :].view(np.uint64) == NAN_BITS).all()
            assert (m[[2, 3], z, :].view(np.uint64) == 0).all()  # sum +0.0, count 0


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_an_all_nan_zone(rasters, kind):
    a, R = rasters(kind)
    T, Rr, Cc = SHAPE
    labels = np.full((Rr, Cc), NONE, dtype=np.uint16)
    labels[17, 23] = labels[258, 259] = 0   # NaN at every instant, in a bulk chunk and in the corner chunk
    labels[40:75, 100:180] = 1              # NaN at the instants 3 .. 8 alone
    labels[17, 24:60] = 2
    assert np.isnan(a[:, labels == 0]).all() and np.isnan(a[3:9][:, labels == 1]).all() and not np.isnan(a[:, labels == 2]).any()
    flat, off, _, _ = R.zonal_flat([[0, T, 0, Rr, 0, Cc]], ALL, [labels], 3)
    m = ZM.matrices(flat, off, 0, ALL, 3, T)
    for z, ts in ((0, slice(0, T)), (1, slice(3, 9))):
        assert (m["count"][z, ts] == 0).all() and (m["sum"][z, ts].view(np.uint64) == 0).all()  # count 0, sum +0.0
        for n in ("min", "max", "mean"):
            assert (m[n][z, ts].view(np.uint64) == NAN_BITS).all()
    check(flat, off, 0, ALL, ZM.zonal(a, labels, 3), 3, T)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sum_is_exact_across_leaves(dc, dtype):
    """exact_raster: leaves of 0 and 25 fractional bits side by side; zones are vertical stripes of 24 columns, the one over columns
    48 .. 71 straddles both leaves: its sums mix the scales and equal math.fsum."""
    a, chunks, EncodedRaster = exact_raster(dc, dtype, 2025)
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    labels = np.ascontiguousarray(np.broadcast_to((np.arange(128) // 24).astype(np.uint16), (64, 128)))
    nz = int(labels.max()) + 1
    x = a.astype(np.float64)
    exact = np.array([[math.fsum(x[t][labels == z].tolist()) for t in range(8)] for z in range(nz)])
    seq = np.array([[np.add.reduce(x[t][labels == z]) for t in range(8)] for z in range(nz)])
    assert (seq[2] != exact[2]).any(), "np.sum equals the exact sum on the straddling zone: the input proves nothing"
    flat, off, _, stats = R.zonal_flat([[0, 8, 0, 64, 0, 128]], ("sum",), [labels], nz)
    assert int(stats[0]) == a.size and int(stats[1]) == 0
    assert_same(flat.reshape(nz, 8), exact)
    flat, off, _, _ = R.zonal_flat([[0, 8, 0, 64, 0, 128]], ALL, [labels], nz)
    check(flat, off, 0, ALL, ZM.zonal(a, labels, nz), nz, 8)
    sub = [2, 7, 5, 64, 9, 123]
    lab = np.ascontiguousarray(labels[5:64, 9:123])
    flat, off, _, _ = R.zonal_flat([sub], ("sum", "mean"), [lab], nz)
    check(flat, off, 0, 20, ZM.zonal(a[2:7, 5:64, 9:123], lab, nz), nz, 5)
    R.close()


def test_wide_values_take_the_walk(dc):
    """int64 near +-2^62 (128-bit sums: all six limbs) and float64 with 61 / 62 fractional bits: not narrow32, so the window walk
    and k_zonal_fold run.  The model is applied to what decode returns."""
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(62)
    wide = (rng.integers(2 ** 62 - 2 ** 20, 2 ** 62, size=(4, 32, 32)) * rng.choice([-1, 1], size=(4, 32, 32))).astype(np.int64)
    wide[:, :, :16] = np.abs(wide[:, :, :16])
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
    for R, dtype, cols in ((Ri, np.int64, 32), (Rf, np.float64, 64)):
        a = R.decode(dtype=dtype)
        labels = (rng.integers(0, 6, size=(32, cols)) + 2 * (np.arange(cols) // 24)).astype(np.uint16)  # zones 0 .. 9, some over both leaves
        labels[rng.random((32, cols)) < 0.1] = NONE
        for cube in ([0, 4, 0, 32, 0, cols], [1, 3, 7, 30, 5, cols - 3]):
            t0, t1, r0, r1, c0, c1 = cube
            lab = np.ascontiguousarray(labels[r0:r1, c0:c1])
            flat, off, _, stats = R.zonal_flat([cube], ALL, [lab], 10)
            assert int(stats[0]) == 0 and int(stats[1]) == (t1 - t0) * (r1 - r0) * (c1 - c0)
            check(flat, off, 0, ALL, ZM.zonal(a[t0:t1, r0:r1, c0:c1], lab, 10), 10, t1 - t0)
        R.close()


def test_minus_zero_is_the_minimum_and_plus_zero_the_maximum(dc):
    """A leaf with 62 fractional bits decodes a stored 1 to -0.0 (from_fixed's wrapped divisor); next to a leaf whose zeros are
    +0.0 a zone of zeros over both has the minimum -0.0 and the maximum +0.0."""
    from dcdf_amd.raster import EncodedRaster
    chunks = []
    for fb in (62, 0):
        (b,) = dc.build_batch([np.zeros((2, 32, 32), dtype=np.float64)], k=2, fractional_bits=fb)
        assert not isinstance(b, Exception)
        chunks.append(b.data)
    R = EncodedRaster((2, 32, 64), chunks, tile=32, chunk_size=2)
    a = R.decode(dtype=np.float64)
    assert np.signbit(a[:, :, :32]).all() and not np.signbit(a[:, :, 32:]).any() and (a == 0).all()
    labels = np.zeros((32, 64), dtype=np.uint16)
    labels[:, :8] = 1   # -0.0 alone
    labels[:, 56:] = 2  # +0.0 alone
    flat, off, _, _ = R.zonal_flat([[0, 2, 0, 32, 0, 64]], ALL, [labels], 3)
    want = ZM.zonal(a, labels, 3)
    check(flat, off, 0, ALL, want, 3, 2)
    assert np.signbit(want["min"][0]).all() and not np.signbit(want["max"][0]).any()
    assert np.signbit(want["max"][1]).all() and not np.signbit(want["min"][2]).any()
    R.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_stored_variable_with_elided_tiles(dtype):
    """A Dataset.append'ed variable as test_gpu_reduce_space builds it: uniform tiles elided, a nested level, offset leaves, a short
    last segment; zones cross the elided tile's edges; Variable.zonal takes arbitrary ids, negative = no zone."""
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
    ids_src = np.array([-7, 3, 40000, 2 ** 40, 17, 5], dtype=np.int64)
    zone = (np.arange(Rr)[:, None] // 24 * 3 + np.arange(Cc)[None, :] // 700) % 6  # blocks of 24 x 700 that cut every tile edge
    labels = ids_src[zone]
    labels[L + 3:2 * L - 3, L + 3:2 * L - 3] = 99  # a zone inside the elided tile alone
    ids, got = v.zonal(labels, SM.NAMES)
    np.testing.assert_array_equal(ids, np.unique(labels[labels >= 0]))
    dense = np.full(labels.shape, NONE, dtype=np.uint16)
    dense[labels >= 0] = np.searchsorted(ids, labels[labels >= 0])
    want = ZM.zonal(dec, dense, ids.size)
    assert list(got) == list(SM.NAMES)
    for n in SM.NAMES:
        assert_same(np.ascontiguousarray(got[n]), want[n])
    _, _, _, stats = R.zonal_flat([[0, T, 0, Rr, 0, Cc]], ALL, [dense], ids.size)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    # a window that cuts stored and elided tiles, one statistic
    win = (7, T - 1, 3, Rr - 3, 10, 900)
    ids2, got = v.zonal(labels[3:Rr - 3, 10:900], ("mean", "max"), *win)
    sub = labels[3:Rr - 3, 10:900]
    d2 = np.full(sub.shape, NONE, dtype=np.uint16)
    d2[sub >= 0] = np.searchsorted(ids2, sub[sub >= 0])
    want = ZM.zonal(dec[7:T - 1, 3:Rr - 3, 10:900], d2, ids2.size)
    assert list(got) == ["max", "mean"]
    for n in got:
        assert_same(np.ascontiguousarray(got[n]), want[n])
    ids0, none = v.zonal(labels, ("count", "min"), 4, 4)
    assert list(none) == ["min", "count"] and none["count"].shape == (ids.size, 0)
    with pytest.raises(ValueError):
        v.zonal(np.arange(Rr * Cc).reshape(Rr, Cc))  # more than 65535 distinct ids
    with pytest.raises(ValueError):
        v.zonal(labels[:, 1:])


def test_batches_give_identical_results(rasters, monkeypatch):
    """K2R_ZONAL_ACC_BYTES shrinks the accumulator scratch: with room for one instant of 37 zones every
    instant is a batch of its own, and the corner piece's walk one instant a slab: the same bits as with the defaults."""
    a, R = rasters("f32")
    T, Rr, Cc = SHAPE
    labels, nz = label_sets(np.random.default_rng(3))[1]
    cubes = [[0, T, 0, Rr, 0, Cc], [5, 17, 250, 264, 3, 264]]
    labs = [labels, np.ascontiguousarray(labels[250:264, 3:264])]
    base, boff, _, bstats = R.zonal_flat(cubes, ALL, labs, nz)
    for cap in (37 * 72, 1, 37 * 72 * 5 + 11):
        monkeypatch.setenv("K2R_ZONAL_ACC_BYTES", str(cap))
        monkeypatch.setenv("K2R_REDUCE_SLAB_CELLS", "100")
        flat, off, _, stats = R.zonal_flat(cubes, ALL, labs, nz)
        assert_same(flat, base)
        np.testing.assert_array_equal(off, boff)
        np.testing.assert_array_equal(stats, bstats)
    check(base, boff, 0, ALL, ZM.zonal(a, labels, nz), nz, T)
    check(base, boff, 1, ALL, ZM.zonal(a[5:17, 250:264, 3:264], labs[1], nz), nz, 12)


def test_time_split_parts(dc):
    """One 64 x 64 unit over a chunk of 64 instants: too few units for the device, so bulk_parts cuts it in time and every part
    adds to its own instants' entries."""
    from dcdf_amd import synth
    a = synth.cells(BD.SEED, 0, 64, 0, 64, 0, 64, np.int32)
    R = BD.build_raster(dc, a, 64, 64)
    labels = (np.arange(64)[:, None] // 16 * 4 + np.arange(64)[None, :] // 16).astype(np.uint16)  # 16 zones: one round exactly
    labels17 = labels.copy()
    labels17[63, 63] = 16  # 17: a second round of one zone
    for lab, nz in ((labels, 16), (labels17, 17), (np.zeros((64, 64), dtype=np.uint16), 1)):
        for cube in ([0, 64, 0, 64, 0, 64], [3, 61, 1, 64, 2, 63]):
            t0, t1, r0, r1, c0, c1 = cube
            sub = np.ascontiguousarray(lab[r0:r1, c0:c1])
            flat, off, _, stats = R.zonal_flat([cube], ALL, [sub], nz)
            assert int(stats[0]) == (t1 - t0) * (r1 - r0) * (c1 - c0)
            check(flat, off, 0, ALL, ZM.zonal(a[t0:t1, r0:r1, c0:c1], sub, nz), nz, t1 - t0)
    R.close()


def test_device_form_and_guard_words(rasters):
    """Labels and output on the device: two cubes with different label arrays at odd offsets, the matrices over a sentinel."""
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters("i32")
    T, Rr, Cc = SHAPE
    rng = np.random.default_rng(12)
    cubes = [[2, 11, 0, 130, 60, 264], [17, 5, 264, 250, 3, 264], [6, 6, 0, 30, 0, 30]]  # (one reversed, one without instants)
    nz, ops = 9, 27
    labs = [rng.integers(0, 12, size=(130, 204)).astype(np.uint16), rng.integers(0, 9, size=(14, 261)).astype(np.uint16),
            np.zeros((30, 30), dtype=np.uint16)]
    labs[0][rng.random(labs[0].shape) < 0.2] = NONE
    flat, off, _, stats = R.zonal_flat(cubes, ops, labs, nz)
    nts = [9, 12, 0]
    np.testing.assert_array_equal(off, [0, 4 * nz * 9, 4 * nz * 21])
    check(flat, off, 0, ops, ZM.zonal(a[2:11, 0:130, 60:264], labs[0], nz), nz, 9)
    check(flat, off, 1, ops, ZM.zonal(a[5:17, 250:264, 3:264], labs[1], nz), nz, 12)
    loff = np.array([7, 7 + labs[0].size + 5, 3], dtype=np.uint64)
    lbuf = DeviceBuffer(2 * (int(loff[1]) + labs[1].size + 16))
    lbuf.write(0, np.full(int(loff[1]) + labs[1].size + 16, 0, dtype=np.uint16))
    for p, o in zip(labs[:2], loff[:2]):
        lbuf.write(2 * int(o), np.ascontiguousarray(p).ravel())
    vol = 4 * nz * np.array(nts, dtype=np.uint64)
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1]) + 7
    buf = DeviceBuffer(total * 8)
    buf.write(0, np.full(total, -77.25, dtype=np.float64))
    ms, dvstats = R.zonal_flat(cubes, ops, (lbuf.ptr, loff), nz, out_device_ptr=buf.ptr, out_offset=doff)
    g = buf.read(0, total * 8, np.float64)
    buf.free()
    lbuf.free()
    np.testing.assert_array_equal(dvstats, stats)
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        o, n = int(doff[q]), int(vol[q])
        inside[o:o + n] = True
        assert_same(g[o:o + n], flat[int(off[q]):int(off[q]) + n])
    assert (g[~inside] == -77.25).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's matrices


def test_rejects_bad_input(dc, rasters):
    from dcdf_amd import _lib as L
    from dcdf_amd import synth
    a, R = rasters("i32")
    lib = L.lib()
    out = np.zeros(64, dtype=np.float64)
    off = np.zeros(1, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.uint64)
    ms = C.c_float()
    lab = np.array([0, 1, 0, 1], dtype=np.uint16)

    def call(h, cubes, nq, ops, outp, offp, mem=L.MEM_HOST, lp=lab.ctypes.data, lo=off.ctypes.data, lmem=L.MEM_HOST, nz=2):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        return lib.dcdf_raster_zonal_batch(h, None if q is None else q.ctypes.data, nq, ops, lp, lo, lmem, nz, outp, mem, offp, stats.ctypes.data, C.byref(ms))

    o, f = out.ctypes.data, off.ctypes.data
    small = [[0, 3, 0, 2, 0, 2]]
    assert call(R._handle(), small, 1, 4 | 8, o, f) == 0 and int(stats.sum()) == 12
    np.testing.assert_array_equal(out[:6].reshape(2, 3), np.stack([a[0:3, :2, 0].sum(1), a[0:3, :2, 1].sum(1)]))  # sum [zone][instant]
    np.testing.assert_array_equal(out[6:12], [2] * 6)
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, 1, o, f) == -5  # DCDF_ERR_BOUNDS
    for ops in (0, 32, 33, 1 << 20):
        assert call(R._handle(), small, 1, ops, o, f) == -1          # no statistic, or a bit above 16: DCDF_ERR_BAD_ARG
    for nz in (0, 65536, 1 << 31):
        assert call(R._handle(), small, 1, 1, o, f, nz=nz) == -1
    big = np.zeros(65535 * 3, dtype=np.float64)
    assert call(R._handle(), small, 1, 1, big.ctypes.data, f, nz=65535) == 0 and np.isnan(big[6:]).all()
    assert call(R._handle(), small, 1, 1, o, f, lp=None) == -1       # NULL labels or offsets
    assert call(R._handle(), small, 1, 1, o, f, lo=None) == -1
    assert call(R._handle(), small, 1, 1, o, f, lmem=7) == -1
    assert call(R._handle(), small, 1, 1, o, f, mem=7) == -1
    assert call(None, small, 1, 1, o, f) == -1
    assert call(R._handle(), None, 1, 1, o, f) == -1
    assert call(R._handle(), small, 1, 1, None, f) == -1
    assert call(R._handle(), small, 1, 1, o, None) == -1
    assert call(R._handle(), small, 0, 1, o, f) == 0                 # nq == 0 is fine
    # stats and kernel_ms may be NULL; a cube without instants writes nothing
    q = np.array([[2, 2, 0, 2, 0, 2]], dtype=np.uint32)
    out[:] = -1
    assert lib.dcdf_raster_zonal_batch(R._handle(), q.ctypes.data, 1, 31, lab.ctypes.data, f, 0, 2, o, L.MEM_HOST, f, None, None) == 0
    assert (out == -1).all()
    # instants but no rows: the "none" values for every zone
    flat, _, _, _ = R.zonal_flat([[2, 9, 40, 40, 0, 100]], ALL, [np.zeros((0, 100), dtype=np.uint16)], 3)
    m = flat.reshape(5, 3, 7)
    assert (m[[0, 1, 4]].view(np.uint64) == NAN_BITS).all() and (m[[2, 3]].view(np.uint64) == 0).all()
    with pytest.raises(ValueError):
        R.zonal_flat(small, 0, [lab.reshape(2, 2)], 2)
    with pytest.raises(ValueError):
        R.zonal_flat(small, 1, [lab.reshape(2, 2)], 0)
    with pytest.raises(ValueError):
        R.zonal_flat(small, 1, [lab.reshape(2, 2).astype(np.int32)], 2)
    # k = 3, side 27: k * k <= 64, the window walk serves it
    a3 = synth.cells(BD.SEED, 0, 4, 0, 27, 0, 27, np.int32)
    R3 = BD.build_raster(dc, a3, 27, 4, k=3)
    l3 = (np.arange(27)[:, None] // 9 * 3 + np.arange(27)[None, :] // 9).astype(np.uint16)
    flat, off3, _, st3 = R3.zonal_flat([[0, 4, 0, 27, 0, 27]], ALL, [l3], 9)
    assert int(st3[0]) == 0 and int(st3[1]) == 4 * 27 * 27
    check(flat, off3, 0, ALL, ZM.zonal(a3, l3, 9), 9, 4)
    R3.close()
    # k = 9: k * k = 81 > 64
    a9 = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R9 = BD.build_raster(dc, a9, 20, 4, k=9)
    with pytest.raises(L.DcdfError) as e:
        R9.zonal_flat([[0, 4, 0, 20, 0, 20]], ALL, [np.zeros((20, 20), dtype=np.uint16)], 1)
    assert e.value.code == -8
    R9.close()
