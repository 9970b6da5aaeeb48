"""Grouped reduce over time (dcdf_raster_reduce_time_groups_batch, EncodedRaster.reduce_time_groups / reduce_time_groups_flat,
Variable.reduce_time_groups) on the GPU.  Every comparison is on bit patterns against group_model.py: per group, reduce_model's
reduce_time of the instants that carry the group's label."""
import ctypes as C

import numpy as np
import pytest

import group_model as GM
import reduce_model as M
import test_gpu_bulk_decode as BD
import test_gpu_reduce_time as RT
from test_gpu_bulk_decode import assert_same

pytestmark = pytest.mark.gpu
ALL = 31
NONE = GM.NONE
SHAPE, TILE, CS, CUBES = RT.FOLD_SHAPE, RT.FOLD_TILE, RT.FOLD_CS, RT.FOLD_CUBES  # (20, 70, 70), 64, 8; the second cube unaligned in every edge
SMALL = [[0, 20, 30, 35, 60, 67]]  # 5 x 7 cells across the tile boundary at column 64


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


def label_sets(nt):
    """(name, labels of a cube of nt instants, n_groups)"""
    i = np.arange(nt)
    odd = np.where(i % 3 == 0, 0, 2)
    odd[i % 5 == 2] = 9      # a label >= n_groups
    odd[[0, 7]] = NONE       # the first instant is of no group; groups 1 and 3 never occur
    return [("one", np.zeros(nt), 1), ("mod3", i % 3, 3), ("div5", i // 5, 4), ("odd", odd, 4)]


def check(flat, off, q, ops, cube, a, labels, n_groups, want=None):
    t0, t1, r0, r1, c0, c1 = RT.norm(cube)
    want = GM.reduce_time_groups(a[t0:t1, r0:r1, c0:c1], labels, n_groups) if want is None else want
    got = GM.planes(flat, off, q, ops, n_groups, r1 - r0, c1 - c0)
    assert list(got) == M.names_of(ops)
    for n in got:
        assert_same(got[n], want[n])
    return want


@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64"])
def test_every_dtype_and_piece(rasters, kind):
    """Bulk chunks, two strips and the 6 x 6 corner chunk on the fallback walk, three segments with the last one short."""
    a, R = rasters(kind)
    _, _, _, dstats = R.decode_flat(CUBES, dtype=a.dtype)
    sets = [label_sets(c[1] - c[0]) for c in CUBES]
    for s in range(len(sets[0])):
        name, _, n_groups = sets[0][s]
        labels = [sets[q][s][1].astype(np.uint16) for q in range(len(CUBES))]
        flat, off, ms, stats = R.reduce_time_groups_flat(CUBES, ALL, labels, n_groups)
        assert ms > 0 and flat.size >= sum(5 * n_groups * (c[3] - c[2]) * (c[5] - c[4]) for c in CUBES)
        np.testing.assert_array_equal(stats, dstats)  # the labels do not change what is read
        assert int(stats[1]) > 0 and (kind[1:] == "64" or int(stats[0]) > 0)
        for q, c in enumerate(CUBES):
            want = check(flat, off, q, ALL, c, a, labels[q], n_groups)
            if name == "odd":
                for g in (1, 3):
                    assert np.isnan(want["min"][g]).all() and (want["count"][g] == 0).all()
        if name == "one":  # reduce_time of the same build, bit for bit
            f1, o1, _, s1 = R.reduce_time_flat(CUBES, ALL)
            np.testing.assert_array_equal(off, o1)
            np.testing.assert_array_equal(s1, stats)
            assert_same(flat, f1)
    lab = np.array([0, 150, 299], dtype=np.uint16)[np.arange(20) % 3]
    flat, off, _, stats = R.reduce_time_groups_flat(SMALL, ALL, [lab], 300)
    assert int(stats.sum()) == 20 * 5 * 7
    want = check(flat, off, 0, ALL, SMALL[0], a, lab, 300)
    assert (want["count"][[1, 149, 151, 298]] == 0).all()
    d = R.reduce_time_groups(("max", "mean"), (np.arange(17) % 2).astype(np.uint16), 2, 19, window=(60, 70, 3, 70))
    want = GM.reduce_time_groups(a[2:19, 60:70, 3:70], np.arange(17) % 2, 2)
    assert list(d) == ["max", "mean"]
    assert_same(d["max"], want["max"])
    assert_same(d["mean"], want["mean"])


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_every_instantiation(rasters, kind):
    """Every `ops` in 1 .. 31 with a change of group at every instant: k_bulk_group<LIVE> for LIVE 1 .. 15, MEAN from scratch planes,
    and the fold kernel."""
    a, R = rasters(kind)
    labels = [(np.arange(c[1] - c[0]) % 3).astype(np.uint16) for c in CUBES]
    want = [GM.reduce_time_groups(a[t0:t1, r0:r1, c0:c1], labels[q], 3) for q, (t0, t1, r0, r1, c0, c1) in enumerate(CUBES)]
    if kind == "f32":
        assert (want[0]["count"] == 0).any() and np.isnan(want[1]["mean"]).any() and (want[0]["count"] > 1).any()
    for ops in range(1, 32):
        flat, off, _, stats = R.reduce_time_groups_flat(CUBES, ops, labels, 3)
        assert int(stats[0]) > 0 and int(stats[1]) > 0 and int(stats.sum()) == BD.volume(CUBES)
        for q, c in enumerate(CUBES):
            check(flat, off, q, ops, c, a, labels[q], 3, want[q])


def test_summation_order_is_observable(dc):
    a, chunks, EncodedRaster = RT.order_raster(dc, np.float64)
    labels = (np.arange(24) % 2).astype(np.uint16)
    want = GM.reduce_time_groups(a, labels, 2)
    differs = False
    for g in (0, 1):  # per-segment partial sums of a group, then added: what a recombination on the host computes
        parts = []
        for s in (0, 8, 16):
            sub = a[s:s + 8][labels[s:s + 8] == g]
            parts.append(M.sequential_sum(sub, np.ones(sub.shape, dtype=bool)))
        differs = differs or ((parts[0] + parts[1]) + parts[2] != want["sum"][g]).any()
    assert differs, "per-segment partial sums equal the group's sequential sum: the input proves nothing"
    R = EncodedRaster(a.shape, chunks, tile=64, chunk_size=8)
    cube = [[0, 24, 0, 64, 0, 64]]
    flat, off, _, stats = R.reduce_time_groups_flat(cube, ("sum",), [labels], 2)
    assert int(stats[0]) == a.size and int(stats[1]) == 0
    assert_same(flat.reshape(2, 64, 64), want["sum"])
    flat, off, _, _ = R.reduce_time_groups_flat(cube, ALL, [labels], 2)
    check(flat, off, 0, ALL, cube[0], a, labels, 2, want)
    flat, off, _, _ = R.reduce_time_groups_flat([[3, 21, 5, 64, 0, 59]], ("sum", "mean"), [labels[:18]], 2)
    check(flat, off, 0, 20, [3, 21, 5, 64, 0, 59], a, labels[:18], 2)
    R.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
@pytest.mark.parametrize("levels,shape", [([4, 8], (34, 300, 2060)), ([1, 6, 5], (40, 40, 2112))], ids=["4x8", "1x6x5_offset_leaves"])
def test_stored_variable(dtype, levels, shape):
    """Elided tiles, nested levels, offset leaves, a short last segment; signed ids, negative = no group."""
    import test_gpu_stored_raster as SR
    from dcdf_amd import _lib, dataset
    assert _lib.lib().dcdf_device_name(), "no GPU"
    rng = np.random.default_rng(sum(shape))
    a = SR.var_data(rng, shape, dtype, 1 << levels[-1])
    v = SR.make_var(dataset, a, levels, 32)
    T, Rr, Cc = shape
    ids_in = rng.choice(np.array([-7, -1, 2, 40, 100000]), size=T)
    ids_in[:5] = [-1, 40, 2, 100000, 40]
    ids, got = v.reduce_time_groups(ids_in, M.NAMES)
    assert ids.tolist() == [2, 40, 100000] and list(got) == list(M.NAMES)
    dense = np.full(T, NONE)
    for i, g in enumerate(ids):
        dense[ids_in == g] = i
    want = GM.reduce_time_groups(v.decode(), dense, 3)
    for n in M.NAMES:
        assert_same(got[n], want[n])
    win = (7, T - 1, 5, Rr - 3, 250, Cc - 9)
    ids, got = v.reduce_time_groups(ids_in[7:T - 1], ("mean", "max"), *win)
    present = [g for g in (2, 40, 100000) if (ids_in[7:T - 1] == g).any()]
    assert ids.tolist() == present and list(got) == ["max", "mean"]
    dense = np.full(T - 8, NONE)
    for i, g in enumerate(ids):
        dense[ids_in[7:T - 1] == g] = i
    want = GM.reduce_time_groups(v.window(*win), dense, len(ids))
    assert_same(got["max"], want["max"])
    assert_same(got["mean"], want["mean"])
    labels = (np.arange(T) % 3).astype(np.uint16)
    _, _, _, stats = v.raster().reduce_time_groups_flat([[0, T, 0, Rr, 0, Cc]], 16, [labels], 3)
    assert int(stats.sum()) == a.size and int(stats[0]) > 0 and int(stats[2]) > 0
    with pytest.raises(ValueError):
        v.reduce_time_groups(ids_in.astype(np.float32))
    with pytest.raises(ValueError):
        v.reduce_time_groups(ids_in[1:])
    with pytest.raises(ValueError):
        v.reduce_time_groups(ids_in.reshape(T, 1))
    # (more than 65535 distinct ids need as many instants: tests/test_reduce_time_groups_host.py refuses them on a stand-in variable)
    none_ids, none = v.reduce_time_groups(np.full(T, -4), ("count", "min"))
    assert none_ids.size == 0 and none["count"].shape == (0, Rr, Cc)
    with pytest.raises(IndexError):
        v.reduce_time_groups(ids_in, stop=T + 1)


def test_both_output_forms(rasters):
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters("f32")
    cubes = CUBES + [[6, 6, 0, 30, 0, 30], [19, 2, 69, 50, 1, 0]]  # one without instants: writes nothing; one with reversed bounds
    labels = [(np.arange(abs(c[1] - c[0])) % 3).astype(np.uint16) for c in cubes]
    ops, n_groups = 27, 3  # min, max, count, mean: the sum lives in scratch
    flat, off, _, stats = R.reduce_time_groups_flat(cubes, ops, labels, n_groups)
    for q, c in enumerate(cubes):
        if q != 2:
            check(flat, off, q, ops, c, a, labels[q], n_groups)
    nb = np.array([RT.norm(c) for c in cubes], dtype=np.int64)
    vol = (4 * n_groups * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64))
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)  # odd gaps: the planes meet misaligned addresses
    total = int(doff[-1] + vol[-1]) + 7
    buf = DeviceBuffer(total * 8)
    buf.write(0, np.full(total, -77.25, dtype=np.float64))
    ms, dvstats = R.reduce_time_groups_flat(cubes, ops, labels, n_groups, out_device_ptr=buf.ptr, out_offset=doff)
    g = buf.read(0, total * 8, np.float64)
    buf.free()
    np.testing.assert_array_equal(dvstats, stats)
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        o, n = int(doff[q]), int(vol[q])
        inside[o:o + n] = True
        assert_same(g[o:o + n], flat[int(off[q]):int(off[q]) + n])
    assert (g[~inside] == -77.25).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's arrays


def test_batch_with_cubes_that_write_nothing(rasters):
    """[cube with cells, cube without instants, cube without cells, cube with cells], every cube with a label array of its own: the
    labels of the two that write nothing are the caller's alone, so the last cube's lie elsewhere on the device than on the host."""
    from dcdf_amd.encoder import DeviceBuffer
    a, R = rasters("f32")
    cubes = [CUBES[1], [6, 6, 0, 30, 0, 30], [2, 9, 40, 40, 3, 50], [19, 1, 66, 2, 69, 4]]
    i = np.arange(20)
    labels = [(i[:16] % 3).astype(np.uint16), np.zeros(0, dtype=np.uint16), np.full(7, 1, dtype=np.uint16), (2 - i[:18] // 7).astype(np.uint16)]
    labels[3][[0, 11]] = NONE
    ops, n_groups = ALL, 3
    flat, off, _, stats = R.reduce_time_groups_flat(cubes, ops, labels, n_groups)
    for q in (0, 3):
        check(flat, off, q, ops, cubes[q], a, labels[q], n_groups)
    nb = np.array([RT.norm(c) for c in cubes], dtype=np.int64)
    vol = (5 * n_groups * (nb[:, 3] - nb[:, 2]) * (nb[:, 5] - nb[:, 4]) * (nb[:, 1] > nb[:, 0])).astype(np.uint64)
    assert vol[1] == 0 and vol[2] == 0 and vol[0] and vol[3]
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64))
    doff = np.concatenate([[5], 5 + np.cumsum(vol + 3)[:-1]]).astype(np.uint64)
    total = int(doff[-1] + vol[-1]) + 7
    buf = DeviceBuffer(total * 8)
    buf.write(0, np.full(total, -77.25, dtype=np.float64))
    ms, dvstats = R.reduce_time_groups_flat(cubes, ops, labels, n_groups, out_device_ptr=buf.ptr, out_offset=doff)
    g = buf.read(0, total * 8, np.float64)
    buf.free()
    np.testing.assert_array_equal(dvstats, stats)
    inside = np.zeros(total, dtype=bool)
    for q in range(len(cubes)):
        o, n = int(doff[q]), int(vol[q])
        inside[o:o + n] = True
        assert_same(g[o:o + n], flat[int(off[q]):int(off[q]) + n])
    assert (g[~inside] == -77.25).all() and (~inside).sum() >= 3 * len(cubes)  # nothing is written outside a cube's arrays


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

    def call(h, cubes, nq, ops, labp, loffp, n_groups, outp, offp, mem=L.MEM_HOST, st=C.c_void_p(stats.ctypes.data), msp=C.byref(ms)):
        q = None if cubes is None else np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
        return lib.dcdf_raster_reduce_time_groups_batch(h, None if q is None else C.c_void_p(q.ctypes.data), C.c_size_t(nq), C.c_uint32(ops), labp, loffp,
                                                        C.c_uint32(n_groups), outp, mem, offp, st, msp)

    small = [[0, 3, 0, 2, 0, 2]]
    out[:] = -1
    assert call(R._handle(), small, 1, 4 | 8, lp, lo, 2, o, f) == 0 and int(stats.sum()) == 12
    x = a[0:3, :2, :2].astype(np.float64)
    np.testing.assert_array_equal(out[:8], np.concatenate([x[1].ravel(), (x[0] + x[2]).ravel()]))
    np.testing.assert_array_equal(out[8:16], [1, 1, 1, 1, 2, 2, 2, 2])
    assert (out[16:] == -1).all()
    for bad in ([[0, SHAPE[0] + 1, 0, 2, 0, 2]], [[0, 1, 0, SHAPE[1] + 1, 0, 2]], [[0, 1, 0, 2, SHAPE[2] + 1, 0]]):
        assert call(R._handle(), bad, 1, 1, lp, lo, 2, o, f) == -5  # DCDF_ERR_BOUNDS
    for ops in (0, 32, 33, 1 << 20):
        assert call(R._handle(), small, 1, ops, lp, lo, 2, o, f) == -1   # no statistic, or a bit above 16: DCDF_ERR_BAD_ARG
    for ng in (0, 65536, 1 << 31):
        assert call(R._handle(), small, 1, 1, lp, lo, ng, o, f) == -1
    assert call(R._handle(), small, 1, 1, lp, lo, 65535, o, f, mem=7) == -1
    assert call(None, small, 1, 1, lp, lo, 2, o, f) == -1                # NULL arguments
    assert call(R._handle(), None, 1, 1, lp, lo, 2, o, f) == -1
    assert call(R._handle(), small, 1, 1, None, lo, 2, o, f) == -1
    assert call(R._handle(), small, 1, 1, lp, None, 2, o, f) == -1
    assert call(R._handle(), small, 1, 1, lp, lo, 2, None, f) == -1
    assert call(R._handle(), small, 1, 1, lp, lo, 2, o, None) == -1
    assert call(R._handle(), small, 0, 1, None, None, 2, o, f) == 0      # nq == 0 is fine
    # stats and kernel_ms may be NULL; a cube without instants, rows or columns writes nothing
    out[:] = -1
    for empty in ([[2, 2, 0, 5, 0, 5]], [[0, 3, 4, 4, 0, 5]], [[0, 3, 0, 5, 7, 7]]):
        assert call(R._handle(), empty, 1, 31, lp, lo, 2, o, f, st=None, msp=None) == 0
    assert (out == -1).all()
    # every label NONE, or beyond n_groups: the none values everywhere, every element written
    none = np.array([NONE, 2, NONE, 5], dtype=np.uint16)
    assert call(R._handle(), [[0, 4, 3, 5, 60, 67]], 1, 31, C.c_void_p(none.ctypes.data), lo, 2, o, f, st=None, msp=None) == 0
    p = out[:5 * 2 * 14].reshape(5, 2 * 14)
    assert np.isnan(p[[0, 1, 4]]).all() and (p[[2, 3]] == 0).all() and not np.signbit(p[2]).any() and (out[140:] == -1).all()
    flat, _, _, _ = R.reduce_time_groups_flat([[0, 4, 3, 5, 60, 67]], 31, [np.full(4, NONE, dtype=np.uint16)], 1)
    assert_same(flat[:70], np.concatenate([np.full(28, np.nan), np.zeros(28), np.full(14, np.nan)]))
    # the wrappers' own refusals
    good = (np.arange(20) % 2).astype(np.uint16)
    for labels, ng in (([good.astype(np.int32)], 2), ([good[:19]], 2), ([good], 0), ([good], 65536), ([good, good], 2)):
        with pytest.raises(ValueError):
            R.reduce_time_groups_flat(CUBES[:1], 1, labels, ng)
    with pytest.raises(ValueError):
        R.reduce_time_groups("sum", good.astype(np.int64))
    with pytest.raises(ValueError):
        R.reduce_time_groups("sum", good, n_groups=65536)
    # a raster holding a k * k > 64 chunk: DCDF_ERR_UNSUPPORTED, as reduce_time
    a9 = synth.cells(BD.SEED, 0, 4, 0, 20, 0, 20, np.int32)
    R9 = BD.build_raster(dc, a9, 20, 4, k=9)
    with pytest.raises(L.DcdfError) as e:
        R9.reduce_time_groups_flat([[0, 4, 0, 20, 0, 20]], ALL, [np.zeros(4, dtype=np.uint16)], 1)
    assert e.value.code == -8
    R9.close()

