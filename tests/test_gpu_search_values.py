"""Value search (real-valued bounds) at every layer: Chunk.search_values, chunk.search_values_batch,
EncodedRaster.search_values_flat, dataset.Variable.search_values.  The oracle everywhere is the typed fill_window of the same
cells, cast to float64: np.argwhere((w64 >= lo) & (w64 <= hi)) (NaN compares false)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


def oracle(w, lo, hi, origin=(0, 0, 0)):
    a, b = min(lo, hi), max(lo, hi)
    w64 = np.asarray(w).astype(np.float64)
    return np.argwhere((w64 >= a) & (w64 <= b)).astype(np.int64) + np.array(origin, dtype=np.int64)


def sort3(t):
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def float_data(rng, shape, bits, dtype, nan_frac=0.05, span=3000):
    """Values exactly representable with `bits` fractional bits (to_fixed needs no rounding), negatives, NaNs, zeros and
    uniform 8 x 8 squares (the walks' whole-subtree paths)."""
    m = rng.integers(-span, span, size=shape)
    m[:, :8, :8] = 7                                   # a uniform square
    m[:, 8:16, 8:16] = rng.integers(-span, span)      # another one, the same at every instant
    x = (m / 2.0 ** bits).astype(dtype)
    x[rng.random(shape) < nan_frac] = np.nan
    x[:, 0, :4] = 0.0
    return x


def host_decode(x, bits, dtype):
    """to_fixed then from_fixed in the dtype (fixed.rs:31-86): the values fill_window must give, computed without the GPU."""
    n = np.where(np.isnan(x), 0, np.round(np.nan_to_num(x).astype(np.float64) * 2.0 ** bits).astype(np.int64) * 2 + 1)
    f = (n - 1).astype(dtype) / dtype(2.0 ** (bits + 1))
    return np.where(n == 0, np.nan, f).astype(dtype)


def bounds_for(x, bits):
    """Straddling 0, exactly representable values and their nextafter neighbours, +-0, +-inf, reversed, empty."""
    step = 2.0 ** -bits
    vals = x[np.isfinite(x)].astype(np.float64)
    v0 = float(np.median(vals))
    out = [(-500 * step, 700 * step), (-INF, INF), (v0, v0), (math.nextafter(v0, INF), v0 + 50 * step), (v0 - 50 * step, math.nextafter(v0, -INF)),
           (0.0, 0.0), (-0.0, 3 * step), (-INF, 0.0), (0.0, INF), (700 * step, -500 * step), (0.25 * step, 0.75 * step), (1e30, INF),
           (-INF, -1e30), (float(vals.min()), float(vals.min())), (float(vals.max()), INF)]
    return out


def check_chunk(ch, cube, lo, hi, w):
    got = ch.search_values(cube, lo, hi).astype(np.int64)
    want = oracle(w[cube.start:cube.end, cube.top:cube.bottom, cube.left:cube.right], lo, hi, (cube.start, cube.top, cube.left))
    assert np.array_equal(got, want), (cube.__dict__, lo, hi, len(got), len(want))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("bits", [0, 2, 8, 29])
@pytest.mark.parametrize("side,k", [(16, 2), (64, 2), (256, 2), (27, 3), (64, 4), (25, 5)])
def test_chunk_matches_typed_fill_window(dc, dtype, bits, side, k):
    rng = np.random.default_rng(side * 100 + bits + k)
    T = 6 if side == 256 else 12
    x = float_data(rng, (T, side, side), bits, dtype)
    for t in range(1, T):  # Log-heavy: each instant changes a few cells of the previous one
        x[t] = x[t - 1]
        idx = rng.integers(0, side, size=(2, 6))
        x[t, idx[0], idx[1]] = (rng.integers(-3000, 3000, size=6) / 2.0 ** bits).astype(dtype)
    ch = dc.Chunk.build(x, k=k, fractional_bits=bits).data
    w = ch.fill_window(dc.Cube(0, T, 0, side, 0, side))
    assert w.dtype == dtype
    np.testing.assert_array_equal(w, host_decode(x, bits, dtype))  # the oracle is not circular
    cubes = [dc.Cube(0, T, 0, side, 0, side), dc.Cube(1, T - 1, 3, side - 2, side // 3, side - 1)]
    for lo, hi in bounds_for(x, bits):
        for cube in cubes:
            check_chunk(ch, cube, lo, hi, w)


def test_chunk_wide_values_take_the_64_bit_walk(dc):
    # stored values beyond 2^30: no narrow walk, no side-16 table
    rng = np.random.default_rng(7)
    x = (rng.integers(-(1 << 20), 1 << 20, size=(5, 64, 64)) * 1024.0 + 0.5).astype(np.float64)
    x[rng.random(x.shape) < 0.03] = np.nan
    ch = dc.Chunk.build(x, fractional_bits=1).data
    w = ch.fill_window(dc.Cube(0, 5, 0, 64, 0, 64))
    np.testing.assert_array_equal(w, host_decode(x, 1, np.float64))
    for lo, hi in [(-1e8, 1e8), (-INF, 0.5), (0.5, 0.5), (-3e8, -1e8), (2e8, INF), (-1.0, 1.0)]:
        check_chunk(ch, dc.Cube(0, 5, 0, 64, 0, 64), lo, hi, w)
        check_chunk(ch, dc.Cube(1, 4, 9, 60, 2, 33), lo, hi, w)


def test_log_quirk_instants_give_true_values(dc):
    # the shape of test_gpu_query.py::test_log_search_reference_quirk_reproduced: iter_search reproduces the reference's
    # quirk there; value search returns the cells whose true value is in range
    a8 = (np.arange(64).reshape(8, 8) * 7 % 13).astype(np.int64)  # a multi-node snapshot
    rng = np.random.default_rng(64)
    s64 = rng.integers(0, 40, size=(64, 64)).astype(np.int64)
    cases = [(np.stack([a8, np.zeros((8, 8), dtype=np.int64) + tv]), 2) for tv in (21, 5)]
    cases += [(np.stack([s64, np.zeros((64, 64), dtype=np.int64) + tv, s64 + 1]), 3) for tv in (55, 17, -3)]
    seen_quirk = False
    for stored, blen in cases:
        data = bytearray(O.chunk_build_forced(stored * 2 + 1, 2, blen))  # odd stored integers: to_fixed's image of stored / 1
        for enc in (64, 32):
            data[0] = enc  # the same stored integers read as a float chunk with 0 fractional bits
            ch = dc.Chunk(bytes(data))
            T, R, Cc = stored.shape
            w = ch.fill_window(dc.Cube(0, T, 0, R, 0, Cc))
            np.testing.assert_array_equal(w, stored.astype(np.float64))
            for lo, hi in [(-10, 100), (0, 39), (10, 20), (5, 5), (16.5, 18), (39, 56), (-8, -1), (-0.5, 0.5)]:
                check_chunk(ch, dc.Cube(0, T, 0, R, 0, Cc), lo, hi, w)
                check_chunk(ch, dc.Cube(1, 2, 1, R - 1, 2, Cc), lo, hi, w)
        # the integer search on the same instant really differs somewhere (the quirk is real here)
        ich = dc.Chunk(bytes([8]) + bytes(data[1:]))
        for lo in range(-10, 60, 3):
            got = set(map(tuple, ich.iter_search(dc.Cube(1, 2, 0, stored.shape[1], 0, stored.shape[2]), 2 * lo + 1, 2 * lo + 41).tolist()))
            want = set(map(tuple, (np.argwhere((stored[1:2] >= lo) & (stored[1:2] <= lo + 20)) + [1, 0, 0]).tolist()))
            seen_quirk = seen_quirk or got != want
    assert seen_quirk


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_integer_chunks_equal_iter_search_on_rounded_bounds(dc, dtype):
    rng = np.random.default_rng(11)
    x = rng.integers(-50, 50, size=(9, 64, 64)).astype(dtype)
    x[:, :16, :16] = 3
    for t in range(1, 9):
        x[t, 20:30, 20:30] = x[t - 1, 20:30, 20:30] + 1
    ch = dc.Chunk.build(x).data
    cube = dc.Cube(0, 9, 2, 61, 5, 64)
    w = ch.fill_window(cube)
    for lo, hi in [(-3.5, 7.25), (0.0, 0.0), (-0.0, 0.0), (2.9, 3.1), (3.0, 3.0), (10.5, 10.9), (49.0, -49.0), (-INF, 0.5), (-1e20, 1e20)]:
        got = ch.search_values(cube, lo, hi)
        a, b = min(lo, hi), max(lo, hi)
        ia = -(1 << 62) if a == -INF else max(math.ceil(a), -(1 << 62))
        ib = 1 << 62 if b == INF else min(math.floor(b), 1 << 62)
        assert np.array_equal(got, ch.iter_search(cube, ia, ib)) if ia <= ib else len(got) == 0
        assert np.array_equal(got.astype(np.int64), oracle(w, lo, hi, (cube.start, cube.top, cube.left)))
    with pytest.raises(dc.DcdfError):
        ch.search_values(cube, float("nan"), 1.0)


@pytest.mark.parametrize("path", ["K2R_SEARCH_DFS", "K2R_SEARCH_CELLS"])
def test_chunk_other_walks(dc, monkeypatch, path):
    # the diagnostic switches route the same chunks through k_search_wave (k = 2 included) and the decode-and-test k_search_cells
    monkeypatch.setenv("K2R_SEARCH_DFS", "1")
    if path == "K2R_SEARCH_CELLS":
        monkeypatch.setenv("K2R_SEARCH_CELLS", "1")
    rng = np.random.default_rng(17)
    for side, k, bits in [(64, 2, 3), (27, 3, 0)]:
        x = float_data(rng, (7, side, side), bits, np.float32)
        ch = dc.Chunk.build(x, k=k, fractional_bits=bits).data
        w = ch.fill_window(dc.Cube(0, 7, 0, side, 0, side))
        for lo, hi in bounds_for(x, bits):
            check_chunk(ch, dc.Cube(0, 7, 0, side, 0, side), lo, hi, w)
            check_chunk(ch, dc.Cube(2, 6, 1, side - 3, 4, side), lo, hi, w)


def _device_triples(n):
    from dcdf_amd.encoder import DeviceBuffer
    return DeviceBuffer(max(12, 12 * n))


def test_batch_mixed_encodings_bits_and_empty_ranges(dc):
    from dcdf_amd import chunk as CH, _lib as L
    rng = np.random.default_rng(5)
    arrays = [rng.integers(-100, 100, size=(4, 32, 32)).astype(np.int32), float_data(rng, (5, 64, 64), 2, np.float32),
              float_data(rng, (3, 32, 48), 8, np.float64), float_data(rng, (6, 64, 64), 29, np.float32)]
    bits = [0, 2, 8, 29]
    chunks = [dc.Chunk.build(a, fractional_bits=b).data for a, b in zip(arrays, bits)]
    ws = [c.fill_window(dc.Cube(0, a.shape[0], 0, a.shape[1], 0, a.shape[2])) for c, a in zip(chunks, arrays)]
    qs, cs, lo, hi = [], [], [], []
    for q in range(40):
        i = q % 4
        T, R, Cc = arrays[i].shape
        t0 = int(rng.integers(T)); r0 = int(rng.integers(R)); c0 = int(rng.integers(Cc))
        cube = dc.Cube(t0, int(rng.integers(t0 + 1, T + 1)), r0, int(rng.integers(r0 + 1, R + 1)), c0, int(rng.integers(c0 + 1, Cc + 1)))
        step = 2.0 ** -bits[i]
        a, b = [(-40 * step, 60 * step), (0.25 * step, 0.75 * step), (-INF, INF), (30 * step, -10 * step), (1e9, 2e9)][q % 5]
        qs.append(i); cs.append(cube); lo.append(a); hi.append(b)
    trip, offs, counts, _ = CH.search_values_batch([chunks[i] for i in qs], cs, lo, hi)
    wants = []
    for q in range(len(qs)):
        c = cs[q]
        want = oracle(ws[qs[q]][c.start:c.end, c.top:c.bottom, c.left:c.right], lo[q], hi[q], (c.start, c.top, c.left))
        got = trip[int(offs[q]):int(offs[q]) + int(counts[q])].astype(np.int64)
        assert np.array_equal(got, want), q
        wants.append(want)
    total = int(counts.sum())
    assert total > 0 and any(len(w) == 0 for w in wants)
    # device output: the same triples, left in device memory
    dbuf = _device_triples(total)
    _, offs2, counts2, _ = CH.search_values_batch([chunks[i] for i in qs], cs, lo, hi, out_device_ptr=dbuf.ptr, cap=total)
    assert np.array_equal(counts2, counts) and np.array_equal(offs2, offs)
    assert np.array_equal(dbuf.read(0, total * 12, np.uint32).reshape(-1, 3), trip[:total])
    dbuf.free()
    # too small a result buffer: DCDF_ERR_CAPACITY, with the counts (and so the needed total) reported
    n = len(qs)
    cub = (L.Cube * n)(*[c._c() for c in cs])
    clo, chi = np.array(lo), np.array(hi)
    cnt, off = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    small = np.zeros((1, 3), dtype=np.uint32)
    rc = L.lib().dcdf_query_search_values_batch(CH._handles([chunks[i] for i in qs]), cub, C.c_void_p(clo.ctypes.data), C.c_void_p(chi.ctypes.data),
                                                C.c_size_t(n), C.c_void_p(small.ctypes.data), C.c_size_t(1), L.MEM_HOST,
                                                C.c_void_p(cnt.ctypes.data), C.c_void_p(off.ctypes.data), None)
    assert rc == -11 and int(cnt.sum()) == total


def test_raster_per_chunk_bits_translated_on_the_device(dc):
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(3)
    T, R, Cc, tile, cs = 10, 80, 96, 32, 4
    x = np.empty((T, R, Cc), dtype=np.float32)
    grid = EncodedRaster.chunk_grid((T, R, Cc), tile, cs)
    bits = [int(b) for b in rng.choice([0, 3, 8, 20], size=len(grid))]
    arrays = []
    for (t0, t1, r0, r1, c0, c1), b in zip(grid, bits):
        x[t0:t1, r0:r1, c0:c1] = float_data(rng, (t1 - t0, r1 - r0, c1 - c0), b, np.float32, span=200 * (1 << b) // 64 + 50)
        arrays.append(x[t0:t1, r0:r1, c0:c1])
    builds = dc.build_batch(arrays, k=2, fractional_bits=bits)
    ER = EncodedRaster((T, R, Cc), [bd.data for bd in builds], tile=tile, chunk_size=cs)
    flat, _, _ = ER.fill_windows_flat([[0, T, 0, R, 0, Cc]], dtype=np.float32)
    w = flat.reshape(T, R, Cc)
    np.testing.assert_array_equal(w, x)
    cubes = [[0, T, 0, R, 0, Cc], [1, 9, 20, 70, 10, 90], [3, 5, 31, 33, 63, 65], [0, 10, 0, 80, 40, 41], [7, 2, 60, 5, 90, 3]]
    for lo, hi in [(-1.0, 1.0), (-INF, INF), (0.0, 0.0), (2.0, 5.5), (-3.0, -0.125), (100.0, 1e9), (0.3, 0.31), (6.0, 2.0)]:
        trip, offs, counts, _ = ER.search_values_flat(cubes, [lo] * len(cubes), [hi] * len(cubes))
        total = int(counts.sum())
        dbuf = _device_triples(total)
        _, doffs, dcounts, _ = ER.search_values_flat(cubes, lo, hi, out_device_ptr=dbuf.ptr, cap=total)
        dtrip = dbuf.read(0, total * 12, np.uint32).reshape(-1, 3)
        dbuf.free()
        assert np.array_equal(dcounts, counts) and np.array_equal(doffs, offs)
        for q, c in enumerate(cubes):
            t0, t1 = sorted(c[:2]); r0, r1 = sorted(c[2:4]); c0, c1 = sorted(c[4:])
            want = oracle(w[t0:t1, r0:r1, c0:c1], lo, hi, (t0, r0, c0))
            got = sort3(trip[int(offs[q]):int(offs[q]) + int(counts[q])])
            assert np.array_equal(got, want), (q, lo, hi)
            assert np.array_equal(sort3(dtrip[int(offs[q]):int(offs[q]) + int(counts[q])]), want)
    with pytest.raises(dc.DcdfError):
        ER.search_values_flat(cubes[:1], float("nan"), 1.0)


# ---- Variable ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds():
    from dcdf_amd import dataset
    return dataset


def make_var(ds, data, k2_levels, chunk_size=5, span_size=2, round=False, fractional_bits=0):
    T, R, Cc = data.shape
    t = ds.Coordinate.time("t", 0, np.timedelta64(100, "s"))
    y = ds.Coordinate.range("y", 0, 1, R, np.float64)
    x = ds.Coordinate.range("x", 0, 1, Cc, np.float64)
    d = ds.Dataset.new([t, y, x], [R, Cc], ds.Resolver())
    d = d.add_variable("v", span_size, chunk_size, k2_levels, round, fractional_bits, dtype=data.dtype.type)
    d = d.append("v", data)
    return d.v, d


def var_data(rng, T, side, dtype, bits, nans=True):
    m = rng.integers(-400, 400, size=(T, side, side))
    m[:, :4, :4] = 9                    # uniform tiles (elided when k2_levels put a tile boundary there)
    m[:, 4:8, 12:16] = -2
    m[2:7, 8:12, 0:4] = 0
    m[:, 12:16, 4:8] = rng.integers(-400, 400, size=(T, 1, 1))  # uniform per instant
    if np.dtype(dtype).kind == "f":
        x = (m / 2.0 ** bits).astype(dtype)
        if nans:  # (a NaN reaching a tile's min / max reduction first makes it the NaN code: no bound to prune with)
            x[rng.random(x.shape) < 0.04] = np.nan
            x[:, 0:4, 8:12] = np.nan          # an all-NaN tile
        return x
    return m.astype(dtype)


def check_var(v, lo, hi, cube=None):
    T, R, Cc = v.shape
    t0, t1, r0, r1, c0, c1 = cube or (0, T, 0, R, 0, Cc)
    got = v.search_values(t0, t1, r0, r1, c0, c1, lo, hi)
    assert got.dtype == np.int64 and got.shape[1] == 3
    want = oracle(v.window(t0, t1, r0, r1, c0, c1), lo, hi, (t0, r0, c0))
    assert np.array_equal(got, want), (lo, hi, cube, len(got), len(want))


@pytest.mark.parametrize("dtype,bits", [(np.float32, 2), (np.float64, 5), (np.float32, 0)])
@pytest.mark.parametrize("levels", [[2, 2], [3, 1], [1, 1, 2]])  # external sub-chunks, 2 x 2 sub-chunks, nested superchunks
def test_variable_float(ds, dtype, bits, levels):
    rng = np.random.default_rng(bits * 10 + len(levels))
    x = var_data(rng, 23, 16, dtype, bits)
    v, _ = make_var(ds, x, levels)
    assert v.window(0, 23, 0, 16, 0, 16).dtype == dtype  # (the oracle is window() itself: the contract is agreement with it)
    s = 2.0 ** -bits
    for lo, hi in [(-INF, INF), (-50 * s, 70 * s), (9 * s, 9 * s), (-2 * s, -2 * s), (0.0, 0.0), (0.25 * s, 0.75 * s), (300 * s, -10 * s),
                   (1e6, INF), (-INF, -1e6)]:
        check_var(v, lo, hi)
        check_var(v, lo, hi, (3, 19, 2, 15, 1, 13))
        check_var(v, lo, hi, (4, 6, 0, 16, 7, 9))
    with pytest.raises(IndexError):
        v.search_values(0, 24, 0, 16, 0, 16, 0.0, 1.0)
    with pytest.raises(ValueError):
        v.search_values(0, 1, 0, 16, 0, 16, float("nan"), 1.0)


def test_variable_round(ds):
    rng = np.random.default_rng(21)
    x = (rng.random((12, 16, 16)) * 40 - 20).astype(np.float32)
    x[:, :4, :4] = 1.5
    x[:, 8:12, 8:12] = np.round(x[:, 8:12, 8:12])  # a tile that needs fewer bits than the node: stored with its own
    x[rng.random(x.shape) < 0.03] = np.nan
    v, _ = make_var(ds, x, [2, 2], round=True, fractional_bits=6)
    for lo, hi in [(-INF, INF), (-3.0, 4.0), (1.5, 1.5), (0.0, 0.0), (-20.0, -19.0), (7.0, 7.0), (30.0, 40.0)]:
        check_var(v, lo, hi)
        check_var(v, lo, hi, (2, 11, 3, 14, 0, 16))


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_variable_integer_equals_search(ds, dtype):
    rng = np.random.default_rng(2)
    x = var_data(rng, 17, 16, dtype, 0)
    v, _ = make_var(ds, x, [2, 2])
    for lo, hi in [(-3.5, 7.25), (9.0, 9.0), (-2.0, -2.0), (0.0, 0.0), (-400.0, 400.0), (8.1, 8.9), (50.0, -50.0)]:
        a, b = min(lo, hi), max(lo, hi)
        ia, ib = math.ceil(a), math.floor(b)
        got = v.search_values(0, 17, 0, 16, 0, 16, lo, hi)
        if ia <= ib:
            assert np.array_equal(got, v.search(0, 17, 0, 16, 0, 16, ia, ib))
        else:  # (no integer in range; the integer search would swap the bounds)
            assert len(got) == 0
        check_var(v, lo, hi, (1, 16, 1, 15, 2, 16))


def test_variable_one_launch_and_pruning(ds, monkeypatch):
    from dcdf_amd import chunk as CH
    from dcdf_amd.chunk import Chunk
    calls = []
    real = CH.search_values_batch

    def counting(*a, **k):
        calls.append(len(a[0]))
        return real(*a, **k)

    monkeypatch.setattr(CH, "search_values_batch", counting)
    rng = np.random.default_rng(9)
    x = var_data(rng, 23, 16, np.float32, 3, nans=False)
    v, d = make_var(ds, x, [2, 2])
    opened = lambda: sum(isinstance(n, Chunk) for n in d._resolver._nodes.values())  # noqa: E731
    before = opened()
    # outside every value: every referenced tile is pruned by the node's min / max, no chunk is opened, no launch
    assert len(v.search_values(0, 23, 0, 16, 0, 16, 1e6, 2e6)) == 0
    assert calls == [] and opened() == before
    check_var(v, -10.0, 10.0)
    assert len(calls) == 1 and calls[0] > 1  # every chunk piece of the call in one launch
    check_var(v, -INF, INF, (0, 23, 3, 13, 0, 16))
    assert len(calls) == 2


def test_cpc_precipitation_between_10_and_20_mm(ds):
    import json
    with open(os.path.join(HERE, "golden", "pydcdf_fixture.json")) as f:
        rw = json.load(f)["real_world"]
    testdata = np.load(os.path.join(HERE, "golden", rw["file"]))["precip"].reshape(rw["shape"]).astype(np.float32)
    t = ds.Coordinate.time("time", np.datetime64("1979-01-01"), np.timedelta64(1, "D"))
    lat = ds.Coordinate.range("latitude", -89.75, 0.5, 360, np.float32)
    lon = ds.Coordinate.range("longitude", -179.75, 0.5, 720, np.float32)
    d = ds.Dataset.new([t, lat, lon], (360, 720), ds.Resolver())
    d = d.add_variable("precip", rw["span_size"], rw["chunk_size"], rw["k2_levels"])
    v = d.append("precip", testdata).precip
    got = v.search_values(0, 1, 0, 360, 0, 720, 10.0, 20.0)
    want = oracle(testdata, 10.0, 20.0)
    assert len(want) > 0 and np.array_equal(got, want)
    for lo, hi in [(0.0, 0.0), (0.1, 0.2), (50.0, INF), (-INF, INF)]:
        check_var(v, lo, hi, (0, 1, 40, 300, 100, 650))


def test_62_fractional_bits_follow_the_decoders_wrapped_divisor(dc):
    """At 62 fractional bits from_fixed's divisor, 1 << 63 in i64, is -2^63 (fixed.rs:84): the decoded value is the negated input,
    falling as the stored integer rises.  A 16 x 16 float64 chunk of multiples of 2^-62 in (-1, 1): the typed fill_window equals
    the oracle's, and value search the brute force over what fill_window returned."""
    rng = np.random.default_rng(62)
    T, side = 3, 16
    m = rng.integers(-(1 << 62) + 1, 1 << 62, size=(T, side, side))
    x = m.astype(np.float64) / 2.0 ** 62
    x[0, 0, :6] = [0.25, -0.25, 0.5, -0.5, 0.0, 2.0 ** -62]
    x[1, 3, 3:6] = np.nan
    x[2] = x[1]
    x[2, 5, 5] = 0.25
    assert (np.abs(x[np.isfinite(x)]) < 1).all()
    b = dc.Chunk.build(x, fractional_bits=62)
    ref = O.chunk_build(x, fractional_bits=62)
    assert b.data.write_to() == ref
    ch = b.data
    w = ch.fill_window(dc.Cube(0, T, 0, side, 0, side))
    want = O.Chunk(ref).fill_window(0, T, 0, side, 0, side)
    assert w.dtype == np.float64
    np.testing.assert_array_equal(w, want)
    np.testing.assert_array_equal(w, -x)  # the reference's quirk, kept
    v0 = float(w[1, 7, 7])
    for lo, hi in [(0.1, 0.5), (-0.5, -0.1), (0.25, 0.25), (-0.25, -0.25), (-1.0, 1.0), (-INF, INF), (0.0, 0.0), (-INF, 0.0), (0.0, INF),
                   (v0, v0), (math.nextafter(v0, INF), INF), (-INF, math.nextafter(v0, -INF)), (0.5, 0.1), (2.0, 3.0)]:
        check_chunk(ch, dc.Cube(0, T, 0, side, 0, side), lo, hi, w)
        check_chunk(ch, dc.Cube(1, T, 2, side - 1, 1, side - 3), lo, hi, w)
    assert len(ch.search_values(dc.Cube(0, T, 0, side, 0, side), 0.1, 0.5)) == int(((w >= 0.1) & (w <= 0.5)).sum()) > 0
