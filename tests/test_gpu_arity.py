"""Every chunk arity and size the ABI accepts, against the oracle and the raw arrays: encode parity for k = 2..16 at every
depth up to sidelen 1024, the query entry points on each of those chunks, every search / window kernel at every arity it can
take (the diagnostic switches included), batches that mix arities, rasters of k = 9 / 16 tiles, and chunks only the oracle
can write (k = 17, 32, 255).  tests/test_oracle_arity.py pins the oracle itself across the same arities."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_search_values import host_decode, oracle as values_oracle
from test_oracle_arity import quirk_instants, ref_sidelen

pytestmark = pytest.mark.gpu
INF = float("inf")
BOUNDS, UNSUPPORTED, BAD_ARG = -5, -8, -1


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


# ---- which kernel a chunk reaches (k2r_query_host.h: wave_kernel_ok / node_kernel_ok) --------------------------------------
def window_kernel(k, sidelen):
    if k == 2 and sidelen >= 4:
        return "k_window_wave2"
    return "k_window_wave" if k * k <= 64 else "k_fill_window"


def search_kernel(k, sidelen):
    if k == 2 and sidelen >= 4:
        return "k_window_wave2<SEARCH>"
    return "k_search_wave" if k * k <= 64 else "k_search_cells"


# ---- the chunks ---------------------------------------------------------------------------------------------------------
def shapes_for(k):
    """(rows, cols) giving every depth with sidelen <= 1024, plus the first depth past it: exact powers, padded shapes, thin
    ones.  Sidelens of 512 and more get one thin or padded shape each (the universal kernel runs one workgroup per tile)."""
    out = []
    h = 1
    while True:
        s = k ** h
        if s > 1024:
            out.append((s // k + 1, 3))  # first shape past the limit: DCDF_ERR_UNSUPPORTED
            break
        if s <= 64:
            out += [(s, s), (s - 1, k ** (h - 1) + 1), (1, s - 1) if s > 2 else (1, s), (s, 2)]
        elif s < 512:
            out += [(s, s), (s - 1, k ** (h - 1) + 1)]
        else:
            out.append((s - 1, 37) if k != 10 else (1000, 999))
        h += 1
    return sorted(set((max(1, r), max(1, c)) for r, c in out))


ONE_BY_ONE = {2, 5, 12}  # a 1 x 1 chunk per query kernel class (k = 2 sidelen 1 takes k_window_wave, like 3..8)


def content(rng, T, R, Cc):
    """Log-heavy instants (each copies the previous one with a few cells changed), a region shifted by a constant ("equal"
    subtrees), a uniform instant, fresh noise that opens a new block."""
    a = np.empty((T, R, Cc), dtype=np.int64)
    a[0] = rng.integers(-300, 300, size=(R, Cc))
    for t in range(1, T):
        a[t] = a[t - 1]
        n = max(1, R * Cc // 200)
        a[t][rng.integers(0, R, size=n), rng.integers(0, Cc, size=n)] = rng.integers(-400, 400, size=n)
    if T > 2:
        a[2, : (R + 1) // 2] += 9
    if T > 3:
        a[3] = -27
    if T > 4:
        a[4] = rng.integers(-5000, 5000, size=(R, Cc))
    return a


def stored_of(x, bits):
    """to_fixed of values exact in `bits` fractional bits (fixed.rs:31-70): NaN -> 0, v -> 2 * v * 2^bits + 1."""
    return np.where(np.isnan(x), 0, np.round(np.nan_to_num(x).astype(np.float64) * 2.0 ** bits).astype(np.int64) * 2 + 1)


def expect_typed(stored, dtype, fbits):
    """MMBuffer3::set of the stored values (mmbuffer.rs:292-299, fixed.rs:81-86), as store_typed writes them."""
    dtype = np.dtype(dtype)
    if dtype == np.int64:
        return stored
    if dtype == np.int32:
        return stored.astype(np.int32)
    f = (stored - 1).astype(dtype) / dtype.type(2.0 ** (fbits + 1))
    return np.where(stored == 0, np.nan, f).astype(dtype)


def uniform_snapshot_logs(stored, snapshots):
    """Log instants whose block's snapshot is a single node: the reference's search seeds their root test with
    snapshot.min.get(0) = 0 (the min Dac of a single-node snapshot is empty) and may keep or drop the whole window; the library
    returns the cells in range."""
    out, snap = set(), 0
    for t in range(stored.shape[0]):
        if t in snapshots:
            snap = t
        elif (stored[snap] == stored[snap].flat[0]).all():
            out.add(t)
    return out


class Case:
    def __init__(self, k, a, fbits=0):
        self.k, self.a, self.fbits = k, a, fbits
        self.T, self.R, self.C = a.shape
        self.floating = a.dtype.kind == "f"
        self.stored = stored_of(a, fbits) if self.floating else a.astype(np.int64)
        self.typed = host_decode(a, fbits, a.dtype.type) if self.floating else a
        self.sidelen = O.sidelen(self.R, self.C, k)
        self.one = self.R * self.C == 1
        self.data, self.ns, self.nl, snaps = O.chunk_build(a, k=k, fractional_bits=fbits, want_snapshots=True)
        self.quirk = quirk_instants(self.stored, set(snaps))
        self.dev = uniform_snapshot_logs(self.stored, set(snaps))

    def __repr__(self):
        return "k=%d %s %s" % (self.k, (self.T, self.R, self.C), self.a.dtype)


def int_case(rng, k, T, R, Cc, dtype):
    a = content(rng, T, R, Cc)
    wide = [t for t in range(T) if t != 3]  # (instant 3 stays uniform)
    if dtype == np.int64:  # beyond 2^32 and into the eighth Dac plane
        a[wide, 0, 0] = 2 ** 33 + 5
        a[min(1, T - 1), R - 1, Cc - 1] = -(2 ** 60)
    else:
        a[wide, R // 2, 0] = 2 ** 30 + 77
        a[wide[-1], 0, Cc - 1] = -(2 ** 31)
    return Case(k, a.astype(dtype))


def float_case(rng, k, T, R, Cc, dtype, bits):
    a = (content(rng, T, R, Cc) / 2.0 ** bits).astype(dtype)
    nan = rng.random((R, Cc)) < 0.04
    for t in range(T):
        if t != 3:  # (instant 3 stays uniform)
            a[t, nan] = np.nan
    a[0, 0, 0] = np.nan
    return Case(k, a, bits)


def cases_for(k):
    """Every shape of shapes_for(k) within the limit, int32 / int64 alternating; float32 / float64 on two of them; a 1 x 1
    chunk for the arities of ONE_BY_ONE."""
    rng = np.random.default_rng(0xA417 + k)
    out, refused = [], []
    for i, (R, Cc) in enumerate(shapes_for(k)):
        if ref_sidelen(R, Cc, k) > 1024:
            refused.append((R, Cc))
            continue
        T = 4 if R * Cc > 100000 else 6
        out.append(int_case(rng, k, T, R, Cc, (np.int64, np.int32)[i % 2]))
    mid = [c for c in out if 8 <= c.R * c.C <= 20000]
    for c, dtype, bits in zip(mid[-2:], (np.float32, np.float64), (3, 20)):
        out.append(float_case(rng, k, 5, c.R, c.C, dtype, bits))
    if k in ONE_BY_ONE:
        out.append(int_case(rng, k, 4, 1, 1, np.int64))
    return out, refused


def test_dispatch_table_covers_every_kernel_class():
    windows, searches = set(), set()
    for k in range(2, 17):
        for R, Cc in shapes_for(k):
            s = O.sidelen(R, Cc, k)
            if s <= 1024:
                windows.add(window_kernel(k, s))
                searches.add(search_kernel(k, s))
        for k1 in ONE_BY_ONE:
            windows.add(window_kernel(k1, 1))
    assert windows == {"k_window_wave2", "k_window_wave", "k_fill_window"}
    assert searches == {"k_window_wave2<SEARCH>", "k_search_wave", "k_search_cells"}
    assert {window_kernel(k, 1) for k in ONE_BY_ONE} == {"k_window_wave", "k_fill_window"}
    assert any(O.sidelen(R, Cc, 2) in (1, 2) for R, Cc in shapes_for(2))
    assert {512, 1024} <= {O.sidelen(R, Cc, 2) for R, Cc in shapes_for(2)}
    assert all(ref_sidelen(R, Cc, k) == O.sidelen(R, Cc, k) for k in range(2, 17) for R, Cc in shapes_for(k))


# ---- queries on one chunk -----------------------------------------------------------------------------------------------
def brute(stored, s, e, t, b, l, r, lo, hi, skip=()):
    sub = stored[s:e, t:b, l:r]
    return set((int(i) + s, int(y) + t, int(x) + l) for i, y, x in zip(*np.nonzero((sub >= lo) & (sub <= hi)))
               if int(i) + s not in skip)


def windows_of(c):
    """Full chunk, a single cell / row / column, windows across the 32- and 64-cell piece edges and the k^j node edges, one
    ending on the last real row and column."""
    T, R, Cc = c.T, c.R, c.C
    ws = [(0, T, 0, R, 0, Cc), (T - 1, T, R - 1, R, Cc - 1, Cc), (1, min(T, 3), R // 2, R // 2 + 1, 0, Cc),
          (0, T, 0, R, Cc // 3, Cc // 3 + 1)]
    for e in (32, 64):
        if R > e - 2 or Cc > e - 2:
            ws.append((0, T, min(e - 3, R - 1), min(e + 2, R), min(e - 2, Cc - 1), min(e + 5, Cc)))
    j = c.k
    while j < max(R, Cc):
        ws.append((1, T, min(j - 1, R - 1), min(j + 1, R), min(max(0, j - 2), Cc - 1), min(j + 3, Cc)))
        j *= c.k
    ws.append((0, 2, max(0, R - 3), R, max(0, Cc - 5), Cc))
    return ws


def raw_fill_window(dc, ch, cube6, dtype):
    """dcdf_chunk_fill_window with the bounds as given (reversed ones included): the library reorders them."""
    from dcdf_amd import _lib as L
    from dcdf_amd.chunk import _ENC
    s, e, t, b, l, r = cube6
    out = np.zeros((abs(e - s), abs(b - t), abs(r - l)), dtype=dtype)
    st = [x // out.itemsize for x in out.strides]
    rc = L.lib().dcdf_chunk_fill_window(ch._h, C.byref(L.Cube(*cube6)), C.c_void_p(out.ctypes.data), _ENC[out.dtype],
                                        C.c_int64(st[0]), C.c_int64(st[1]), C.c_int64(st[2]))
    return rc, out


def search_bounds(c):
    v = c.stored[np.isfinite(c.typed) if c.floating else np.ones_like(c.stored, dtype=bool)]
    p = [int(x) for x in np.percentile(v, [10, 35, 50, 90])]
    return [(p[1], p[2]), (p[0], p[3]), (-27, -27), (p[2], p[2]), (int(v.max()) + 1, 2 ** 62), (-(2 ** 62), 2 ** 62)]


def value_bounds_of(c):
    v = c.typed[np.isfinite(c.typed)].astype(np.float64) if c.floating else c.typed.astype(np.float64).ravel()
    med, step = float(np.median(v)), 2.0 ** -c.fbits
    return [(-INF, INF), (med - 40 * step, med + 40 * step), (med, med), (0.0, 0.0), (float(v.max()), -INF)]


def check_search(dc, ch, c, cube, lo, hi, oc):
    got = ch.iter_search(dc.Cube(*cube), lo, hi)
    res = [tuple(x) for x in got.tolist()]
    assert res == sorted(res), (c, cube)
    got = set(res)
    assert set(x for x in got if x[0] not in c.quirk) == brute(c.stored, *cube, lo, hi, c.quirk), (c, cube, lo, hi)
    if oc is not None:
        want = set(map(tuple, oc.search(*cube, lo, hi).tolist()))
        assert set(x for x in got if x[0] not in c.dev) == set(x for x in want if x[0] not in c.dev), (c, cube, lo, hi)
    return got


def check_queries(dc, ch, c, full=True):
    """Item 2 of the suite: get, fill_cell, fill_window in every output type, search against brute force and the oracle,
    value search against the decoded values."""
    T, R, Cc = c.T, c.R, c.C
    assert ch.shape() == [T, R, Cc]
    oc = None if c.one else O.Chunk(c.data)
    rng = np.random.default_rng(c.k * 7919 + R * 31 + Cc)
    # get: every cell (one launch) for small chunks, a sample of large ones; single calls at the corners
    if T * R * Cc <= 40000:
        pts = np.argwhere(np.ones((T, R, Cc), dtype=bool))
    else:
        pts = np.stack([rng.integers(0, T, 3000), rng.integers(0, R, 3000), rng.integers(0, Cc, 3000)], axis=1)
    np.testing.assert_array_equal(dc.get_batch([ch] * len(pts), pts), c.stored[pts[:, 0], pts[:, 1], pts[:, 2]])
    for t, r, cc in [(0, 0, 0), (T - 1, R - 1, Cc - 1), (T // 2, R // 2, Cc // 2)]:
        assert ch.get(t, r, cc) == c.stored[t, r, cc], (c, t, r, cc)
    with pytest.raises(dc.DcdfError) as e:
        ch.get(0, R, 0)
    assert e.value.code == BOUNDS
    # fill_cell
    for r, cc in [(0, 0), (R - 1, Cc - 1), (R // 2, Cc // 3)]:
        np.testing.assert_array_equal(ch.fill_cell(0, T, r, cc), c.stored[:, r, cc])
        np.testing.assert_array_equal(ch.fill_cell(T - 1, 1, r, cc), c.stored[1:T - 1, r, cc])
    # fill_window
    own = c.a.dtype
    others = [np.int64] if c.floating else [np.int64 if own == np.int32 else np.int32]
    for i, (s, e, t, b, l, r) in enumerate(windows_of(c) if full else windows_of(c)[:1]):
        for dtype in [own] + (others if i == 0 else []):
            w = ch.fill_window(dc.Cube(s, e, t, b, l, r), dtype=dtype)
            np.testing.assert_array_equal(w, expect_typed(c.stored[s:e, t:b, l:r], dtype, c.fbits), err_msg=repr((c, s, e, t, b, l, r)))
            if dtype == own:
                np.testing.assert_array_equal(w, c.typed[s:e, t:b, l:r])
    rc, w = raw_fill_window(dc, ch, (T, 0, R, 0, Cc, 0), own)  # reversed on every axis
    assert rc == 0
    np.testing.assert_array_equal(w, c.typed)
    for cube in [(0, T, 0, R + 1, 0, Cc), (0, T, 0, R, 0, Cc + 1), (0, T + 1, 0, R, 0, Cc)]:
        assert raw_fill_window(dc, ch, cube, own)[0] == BOUNDS
        with pytest.raises(dc.DcdfError) as e:
            ch.iter_search(dc.Cube(*cube), 0, 1)
        assert e.value.code == BOUNDS
    # search
    cubes = [(0, T, 0, R, 0, Cc), windows_of(c)[-1], (1, T, R // 3, R, 0, max(1, Cc // 2))]
    for lo, hi in search_bounds(c) if full else search_bounds(c)[:2]:
        for cube in cubes:
            check_search(dc, ch, c, cube, lo, hi, oc)
    got = ch.iter_search(dc.Cube(T, 0, R, 0, Cc, 0), 50, -50)  # reversed bounds are swapped (chunk.rs:214)
    assert set(map(tuple, got.tolist())) == set(x for x in check_search(dc, ch, c, (0, T, 0, R, 0, Cc), -50, 50, oc))
    # value search: the true values, the reference quirk instants included
    for lo, hi in value_bounds_of(c) if full else value_bounds_of(c)[:2]:
        for cube in cubes[:2]:
            s, e, t, b, l, r = cube
            got = ch.search_values(dc.Cube(*cube), lo, hi).astype(np.int64)
            assert np.array_equal(got, values_oracle(c.typed[s:e, t:b, l:r], lo, hi, (s, t, l))), (c, cube, lo, hi)


def check_build(dc, cases, k):
    """build_batch == Chunk::build of the oracle: bytes, snapshot / log counts, per-instant stored (min, max)."""
    for floating in (False, True):
        group = [c for c in cases if c.floating == floating]
        if not group:
            continue
        res = dc.build_batch([c.a for c in group], k=k, fractional_bits=[c.fbits for c in group])
        for c, r in zip(group, res):
            assert not isinstance(r, Exception), (c, r)
            assert r.data.write_to() == c.data, c
            assert (r.snapshots, r.logs) == (c.ns, c.nl), c
            flat = c.stored.reshape(c.T, -1)
            np.testing.assert_array_equal(r.minmax, np.stack([flat.min(1), flat.max(1)], axis=1), err_msg=repr(c))
            c.built = r.data


_CASES = {}


def cases(k):
    if k not in _CASES:
        _CASES[k] = cases_for(k)
    return _CASES[k]


@pytest.mark.parametrize("k", range(2, 17))
def test_encode_and_query_every_depth(dc, k):
    cs, refused = cases(k)
    assert all((c.stored[3] == c.stored[3].flat[0]).all() for c in cs)  # every chunk has a uniform instant
    assert refused and {window_kernel(k, c.sidelen) for c in cs} >= {window_kernel(k, 1 << 20)}
    check_build(dc, cs, k)
    for R, Cc in refused:
        r = dc.build_batch([np.zeros((2, R, Cc), dtype=np.int32)], k=k)[0]
        assert isinstance(r, Exception) and r.code == UNSUPPORTED, (k, R, Cc)
    for c in cs:
        check_queries(dc, c.built, c, full=c.T * c.R * c.C <= 300000)
        if c.one:  # the oracle panics on every read of a 1 x 1 chunk (test_oracle_arity.py); the GPU returns the values
            with pytest.raises(O.OracleError) as e:
                O.Chunk(c.data).get(0, 0, 0)
            assert e.value.code == BOUNDS
            np.testing.assert_array_equal(c.built.fill_window(dc.Cube(0, c.T, 0, 1, 0, 1)), c.a)
            np.testing.assert_array_equal(c.built.fill_cell(0, c.T, 0, 0), c.a[:, 0, 0])
            assert [c.built.get(t, 0, 0) for t in range(c.T)] == c.a[:, 0, 0].tolist()


@pytest.mark.parametrize("k", [1, 17, 0, 32])
def test_arity_outside_2_to_16_is_a_bad_argument(dc, k):
    try:
        r = dc.build_batch([np.zeros((2, 4, 4), dtype=np.int32)], k=k)[0]
    except dc.DcdfError as e:
        r = e
    assert isinstance(r, Exception) and r.code == BAD_ARG


# ---- the quirk instants at higher arity ---------------------------------------------------------------------------------
def quirk_chunks():
    out = []
    for k in (4, 8, 9, 16):
        rng = np.random.default_rng(400 + k)
        side = {4: 64, 8: 64, 9: 81, 16: 40}[k]
        s = rng.integers(0, 40, size=(side, side)).astype(np.int64)
        for tv in (23, -3):
            out.append((k, np.stack([s, np.full((side, side), tv, dtype=np.int64), s + 1, np.full((side, side), 39, dtype=np.int64)])))
    return out


def test_quirk_instants_at_higher_arity(dc):
    seen = set()
    for k, stored in quirk_chunks():
        T, R, Cc = stored.shape
        data = O.chunk_build_forced(stored, k, 4)
        ch, oc = dc.Chunk(data), O.Chunk(data)
        np.testing.assert_array_equal(ch.fill_window(dc.Cube(0, T, 0, R, 0, Cc)), stored)
        for lo, hi in [(0, 39), (10, 20), (23, 23), (-20, 5), (-3, -3), (30, 45)]:
            for cube in [(0, T, 0, R, 0, Cc), (1, 2, 3, R - 1, 1, Cc - 5), (3, 4, 0, R, 0, Cc)]:
                got = set(map(tuple, ch.iter_search(dc.Cube(*cube), lo, hi).tolist()))
                assert got == set(map(tuple, oc.search(*cube, lo, hi).tolist())), (k, cube, lo, hi)
                if got != brute(stored, *cube, lo, hi):
                    seen.add(k)
        # value search gives the true values: the same stored integers read as a float chunk with 0 fractional bits
        fdata = bytearray(O.chunk_build_forced(stored * 2 + 1, k, 4))
        fdata[0] = 64
        fch = dc.Chunk(bytes(fdata))
        for lo, hi in [(0, 39), (10, 20), (23, 23), (-20, 5), (-3.5, -2.5)]:
            for cube in [(0, T, 0, R, 0, Cc), (1, 2, 3, R - 1, 1, Cc - 5)]:
                s, e, t, b, l, r = cube
                got = fch.search_values(dc.Cube(*cube), lo, hi).astype(np.int64)
                assert np.array_equal(got, values_oracle(stored[s:e, t:b, l:r], lo, hi, (s, t, l))), (k, cube, lo, hi)
    assert seen == {4, 8, 9, 16}  # the quirk is real at every one of these arities


def test_logs_over_a_uniform_snapshot_give_the_cells_in_range(dc):
    """Log::search_window (log.rs:519-551) seeds min_s with snapshot.min.get(0), which is 0 for a single-node snapshot
    (snapshot.rs:123-151 pushes no min for an elided root): the reference's root test is off by the snapshot's value.  Not
    reproduced: the GPU returns the cells in range, on every search kernel."""
    differs = set()
    for k in (2, 4, 9):
        rng = np.random.default_rng(900 + k)
        side = {2: 16, 4: 16, 9: 20}[k]
        logs = rng.integers(-200, 100, size=(2, side, side))
        for v in (-27, 40):
            stored = np.concatenate([np.full((1, side, side), v), logs]).astype(np.int64)
            data = O.chunk_build_forced(stored, k, 3)
            ch, oc = dc.Chunk(data), O.Chunk(data)
            m = int(logs.min())  # a negative snapshot value lifts the root's min: it keeps or drops everything near m
            for lo, hi in [(m + 5, 500), (m, m + 10), (-20, 60), (10, 10), (-250, 150)]:
                cube = (0, 3, 0, side, 0, side)
                got = set(map(tuple, ch.iter_search(dc.Cube(*cube), lo, hi).tolist()))
                assert got == brute(stored, *cube, lo, hi), (k, v, lo, hi)
                if set(map(tuple, oc.search(*cube, lo, hi).tolist())) != got:
                    differs.add(k)
    assert differs == {2, 4, 9}  # the reference really is the odd one out at each of these arities


# ---- each search kernel at every arity it can take ----------------------------------------------------------------------
def switch_cases():
    out = []
    for k in range(2, 17):
        cs, _ = cases(k)
        mid = [c for c in cs if not c.one and 16 <= c.R * c.C <= 20000]
        out += mid[-3:]
    return out


@pytest.mark.parametrize("switch", ["K2R_SEARCH_DFS", "K2R_SEARCH_CELLS"])
def test_search_switches_do_not_change_results(dc, monkeypatch, switch):
    cs = switch_cases()
    assert {search_kernel(c.k, c.sidelen) for c in cs} == {"k_window_wave2<SEARCH>", "k_search_wave", "k_search_cells"}
    chunks = [dc.Chunk(c.data) for c in cs]
    qs = [(c, (1, c.T, 0, c.R, c.C // 4, c.C), b) for c in cs for b in search_bounds(c)[:3]]
    vqs = [(c, (0, c.T - 1, c.R // 5, c.R, 0, c.C), b) for c in cs for b in value_bounds_of(c)[:3]]
    quirks = [(k, dc.Chunk(O.chunk_build_forced(s, k, 4)), s) for k, s in quirk_chunks()]

    def run():
        r = [ch.iter_search(dc.Cube(*cube), lo, hi).tolist() for ch, (c, cube, (lo, hi)) in zip([x for x in chunks for _ in range(3)], qs)]
        r += [ch.search_values(dc.Cube(*cube), lo, hi).tolist() for ch, (c, cube, (lo, hi)) in zip([x for x in chunks for _ in range(3)], vqs)]
        for k, ch, s in quirks:
            T, R, Cc = s.shape
            r += [ch.iter_search(dc.Cube(0, T, 1, R, 0, Cc - 1), lo, hi).tolist() for lo, hi in [(0, 39), (23, 23), (-20, 5)]]
        return r

    base = run()
    for (c, cube, (lo, hi)), got in zip(qs, base):  # the default dispatch is right to begin with
        assert set(x for x in map(tuple, got) if x[0] not in c.quirk) == brute(c.stored, *cube, lo, hi, c.quirk), (c, cube)
    monkeypatch.setenv("K2R_SEARCH_DFS", "1")  # k = 2 onto k_search_wave, the rest as before
    if switch == "K2R_SEARCH_CELLS":
        monkeypatch.setenv("K2R_SEARCH_CELLS", "1")  # every arity onto k_search_cells, integer and value instantiations
    alt = run()
    for i, (a, b) in enumerate(zip(base, alt)):
        assert a == b, (switch, i)


def test_no_top_table_windows(dc, monkeypatch):
    """k = 2 chunks of sidelen 32..256 start their walks from the per-instant top table; without it (read at open) the
    windows are the same."""
    cs = [c for c in cases(2)[0] if 32 <= c.sidelen <= 256]
    assert {c.sidelen for c in cs} == {32, 64, 128, 256}
    base = [[dc.Chunk(c.data).fill_window(dc.Cube(*w), dtype=c.a.dtype) for w in windows_of(c)] for c in cs]
    monkeypatch.setenv("K2R_NO_TOP_TABLE", "1")
    for c, ws in zip(cs, base):
        ch = dc.Chunk(c.data)
        for w, want in zip(windows_of(c), ws):
            got = ch.fill_window(dc.Cube(*w), dtype=c.a.dtype)
            np.testing.assert_array_equal(got, want)
            s, e, t, b, l, r = w
            np.testing.assert_array_equal(got, c.typed[s:e, t:b, l:r])


# ---- batches ------------------------------------------------------------------------------------------------------------
def batch_queries(rng, cs, n):
    which = [i % len(cs) for i in range(n)]
    rng.shuffle(which)
    cubes = []
    for i in which:
        c = cs[i]
        t0 = int(rng.integers(c.T)); r0 = int(rng.integers(c.R)); c0 = int(rng.integers(c.C))
        cubes.append((t0, int(rng.integers(t0 + 1, c.T + 1)), r0, int(rng.integers(r0 + 1, c.R + 1)), c0, int(rng.integers(c0 + 1, c.C + 1))))
    return which, cubes


def check_batches(dc, cs, chunks, seed, n=40):
    """get / fill_cell / fill_window (int64 and typed, host and device output) / search / value search of one batch over
    `chunks` (repeated handles), per query against the single-chunk entry points and the arrays."""
    from dcdf_amd import chunk as CH, _lib as L
    from dcdf_amd.encoder import DeviceBuffer
    rng = np.random.default_rng(seed)
    which, cubes = batch_queries(rng, cs, n)
    hs = [chunks[i] for i in which]
    # points and cell series
    pts = np.array([[int(rng.integers(cs[i].T)), int(rng.integers(cs[i].R)), int(rng.integers(cs[i].C))] for i in which])
    np.testing.assert_array_equal(dc.get_batch(hs, pts), [cs[i].stored[t, r, c] for i, (t, r, c) in zip(which, pts)])
    cells = [(cs[i].T, int(q % 2), int(p[1]), int(p[2])) for q, (i, p) in enumerate(zip(which, pts))]
    for i, (s, e, r, cc), sr in zip(which, cells, dc.fill_cell_batch(hs, cells)):
        np.testing.assert_array_equal(sr, cs[i].stored[min(s, e):max(s, e), r, cc])
    # windows: int64 (the entry point the raster routing uses) and typed, host and device output
    dcubes = [dc.Cube(*cu) for cu in cubes]
    dtypes = [np.int64, np.int32] + ([np.float32, np.float64] if any(c.floating for c in cs) else [])
    vol = [cu.instants() * cu.rows() * cu.cols() for cu in dcubes]
    for dtype in dtypes:
        flat, off = dc.fill_window_batch(hs, dcubes, dtype=dtype)
        for q, (i, cu) in enumerate(zip(which, cubes)):
            s, e, t, b, l, r = cu
            want = expect_typed(cs[i].stored[s:e, t:b, l:r], dtype, cs[i].fbits)
            got = flat[int(off[q]):int(off[q]) + vol[q]].reshape(want.shape)
            np.testing.assert_array_equal(got, want, err_msg=repr((dtype, cs[i], cu)))
            if q < 6:
                np.testing.assert_array_equal(got, hs[q].fill_window(dcubes[q], dtype=dtype))
        doff = np.cumsum([5] + [v + 3 for v in vol[:-1]]).astype(np.uint64)  # gaps between the windows stay untouched
        end = int(doff[-1]) + vol[-1]
        es = np.dtype(dtype).itemsize
        dev = DeviceBuffer(end * es + 64)
        sentinel = np.full(end, 77, dtype=dtype)
        dev.write(0, sentinel)
        dc.fill_window_batch(hs, dcubes, dtype=dtype, out_device_ptr=dev.ptr, out_offset=doff)
        back = dev.read(0, end * es, dtype)
        dev.free()
        mask = np.ones(end, dtype=bool)
        for q in range(n):
            np.testing.assert_array_equal(back[int(doff[q]):int(doff[q]) + vol[q]], flat[int(off[q]):int(off[q]) + vol[q]])
            mask[int(doff[q]):int(doff[q]) + vol[q]] = False
        assert (back[mask] == 77).all()
    # search: dcdf_query_search_batch against the single-chunk search
    lower = np.array([search_bounds(cs[i])[q % 3][0] for q, i in enumerate(which)], dtype=np.int64)
    upper = np.array([search_bounds(cs[i])[q % 3][1] for q, i in enumerate(which)], dtype=np.int64)
    cap = sum(vol)
    res = np.zeros((cap, 3), dtype=np.uint32)
    counts, soff = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    cub = (L.Cube * n)(*[cu._c() for cu in dcubes])
    ms = C.c_float()
    L.check(L.lib().dcdf_query_search_batch(CH._handles(hs), cub, C.c_void_p(lower.ctypes.data), C.c_void_p(upper.ctypes.data),
                                            C.c_size_t(n), C.c_void_p(res.ctypes.data), C.c_size_t(cap), C.c_void_p(counts.ctypes.data),
                                            C.c_void_p(soff.ctypes.data), C.byref(ms)), "search_batch")
    for q, i in enumerate(which):
        got = res[int(soff[q]):int(soff[q] + counts[q])].tolist()
        assert got == hs[q].iter_search(dcubes[q], int(lower[q]), int(upper[q])).tolist(), (q, cs[i])
        assert set(x for x in map(tuple, got) if x[0] not in cs[i].quirk) == brute(cs[i].stored, *cubes[q], lower[q], upper[q], cs[i].quirk)
    # value search
    vlo = [value_bounds_of(cs[i])[q % 4][0] for q, i in enumerate(which)]
    vhi = [value_bounds_of(cs[i])[q % 4][1] for q, i in enumerate(which)]
    trip, offs, cnts, _ = CH.search_values_batch(hs, dcubes, vlo, vhi)
    for q, i in enumerate(which):
        s, e, t, b, l, r = cubes[q]
        got = trip[int(offs[q]):int(offs[q]) + int(cnts[q])].astype(np.int64)
        assert np.array_equal(got, values_oracle(cs[i].typed[s:e, t:b, l:r], vlo[q], vhi[q], (s, t, l))), (q, cs[i])
        if q < 6:
            assert np.array_equal(got, hs[q].search_values(dcubes[q], vlo[q], vhi[q]).astype(np.int64))


@pytest.mark.parametrize("k", [2, 3, 8, 9, 16])
def test_single_arity_batches(dc, k):
    cs = [c for c in cases(k)[0] if c.T * c.R * c.C <= 60000]
    check_batches(dc, cs, [dc.Chunk(c.data) for c in cs], seed=k)


def test_mixed_arity_batch(dc):
    """k = 2, 3, 8, 9 and 16 chunks and a 1 x 1 chunk in one batch: the k = 9 / 16 chunks send every query of it to the
    per-cell kernels, whose typed output is the walks' (a typed batch with such a chunk was DCDF_ERR_UNSUPPORTED)."""
    cs = []
    for k in (2, 3, 8, 9, 16):
        pool = [c for c in cases(k)[0] if not c.one and 16 <= c.R * c.C <= 20000]
        cs += [pool[-1], next(c for c in pool if c.floating)]
    cs.append(next(c for c in cases(2)[0] if c.one))
    assert {window_kernel(c.k, c.sidelen) for c in cs} == {"k_window_wave2", "k_window_wave", "k_fill_window"}
    check_batches(dc, cs, [dc.Chunk(c.data) for c in cs], seed=99, n=60)


# ---- rasters of k = 9 and k = 16 tiles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,tile", [(9, 20), (16, 17)])
def test_raster_of_wide_arity_tiles(dc, k, tile):
    from dcdf_amd.raster import EncodedRaster
    rng = np.random.default_rng(k)
    T, R, Cc, cs = 7, 2 * tile + 1, 3 * tile - 4, 3  # ragged last tiles, a 1-row band, a short last segment
    a = np.empty((T, R, Cc), dtype=np.int64)
    a[0] = rng.integers(-200, 200, size=(R, Cc))
    for t in range(1, T):
        a[t] = a[t - 1] + (rng.random((R, Cc)) < 0.05) * rng.integers(-9, 9, size=(R, Cc))
    grid = EncodedRaster.chunk_grid(a.shape, tile, cs)
    builds = dc.build_batch([a[t0:t1, r0:r1, c0:c1] for t0, t1, r0, r1, c0, c1 in grid], k=k)
    for (t0, t1, r0, r1, c0, c1), bd in zip(grid, builds):
        assert bd.data.write_to() == O.chunk_build(a[t0:t1, r0:r1, c0:c1], k=k)
    ER = EncodedRaster(a.shape, [bd.data for bd in builds], tile=tile, chunk_size=cs)
    cubes = [[0, T, 0, R, 0, Cc], [1, 6, tile - 2, R, 3, Cc - 1], [2, 3, R - 1, R, 0, Cc], [6, 0, 30, 2, 40, 1]]
    for lo, hi in [(-50, 50), (0, 0), (-1000, 1000), (150, 400)]:
        trip, offs, counts, _ = ER.search_flat(cubes, [lo] * 4, [hi] * 4)
        for q, cu in enumerate(cubes):
            t0, t1 = sorted(cu[:2]); r0, r1 = sorted(cu[2:4]); c0, c1 = sorted(cu[4:])
            got = set(map(tuple, trip[int(offs[q]):int(offs[q] + counts[q])].tolist()))
            assert got == brute(a, t0, t1, r0, r1, c0, c1, lo, hi), (q, lo, hi)
    with pytest.raises(dc.DcdfError) as e:
        ER.fill_windows_flat(cubes[:1])
    assert e.value.code == UNSUPPORTED  # as the header documents for k * k > 64 rasters
    for cu, w in zip(cubes[:3], ER.fill_windows(cubes[:3])):
        np.testing.assert_array_equal(w, a[cu[0]:cu[1], cu[2]:cu[3], cu[4]:cu[5]])
    # value search on a float raster of the same tiles
    x = (a / 8.0).astype(np.float32)
    x[:, rng.random((R, Cc)) < 0.05] = np.nan
    fb = dc.build_batch([x[t0:t1, r0:r1, c0:c1] for t0, t1, r0, r1, c0, c1 in grid], k=k, fractional_bits=3)
    FR = EncodedRaster(x.shape, [bd.data for bd in fb], tile=tile, chunk_size=cs)
    for lo, hi in [(-5.0, 5.0), (-INF, INF), (0.125, 0.125), (20.0, -3.5)]:
        trip, offs, counts, _ = FR.search_values_flat(cubes, lo, hi)
        for q, cu in enumerate(cubes):
            t0, t1 = sorted(cu[:2]); r0, r1 = sorted(cu[2:4]); c0, c1 = sorted(cu[4:])
            t3 = trip[int(offs[q]):int(offs[q] + counts[q])].astype(np.int64)
            got = t3[np.lexsort((t3[:, 2], t3[:, 1], t3[:, 0]))]
            assert np.array_equal(got, values_oracle(x[t0:t1, r0:r1, c0:c1], lo, hi, (t0, r0, c0))), (q, lo, hi)


# ---- open paths ---------------------------------------------------------------------------------------------------------
def test_chunks_only_the_oracle_writes(dc):
    """k = 17, 32, 255 (dcdf_chunk_open takes k up to 255): opened one by one and as a host batch, queried as above."""
    from dcdf_amd import _lib as L
    rng = np.random.default_rng(255)
    cs = [int_case(rng, 17, 5, 17, 17, np.int64), int_case(rng, 17, 5, 20, 3, np.int32), int_case(rng, 32, 5, 31, 40, np.int64),
          int_case(rng, 255, 3, 255, 200, np.int32), float_case(rng, 32, 4, 32, 32, np.float64, 12)]
    for c in cs:
        check_queries(dc, dc.Chunk(c.data), c)
    n = len(cs)
    bufs = [C.create_string_buffer(c.data, len(c.data)) for c in cs]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint64 * n)(*[len(c.data) for c in cs])
    hs = (C.c_void_p * n)()
    st = (C.c_int32 * n)()
    L.check(L.lib().dcdf_chunk_open_batch(ptrs, lens, C.c_size_t(n), L.MEM_HOST, hs, st), "chunk_open_batch")
    assert list(st) == [0] * n
    opened = []
    for j in range(n):
        ch = dc.Chunk.__new__(dc.Chunk)
        ch._bytes, ch._handle, ch._shape = cs[j].data, C.c_void_p(hs[j]), None
        opened.append(ch)
    for ch, c in zip(opened, cs):
        check_queries(dc, ch, c, full=False)
    check_batches(dc, cs, opened, seed=255, n=20)


def test_gpu_built_chunks_opened_from_device_memory(dc):
    """Encoder sessions of k = 3, 8, 9, 16 leave the chunks in HBM; opened there (dcdf_chunk_open_batch, DCDF_MEM_DEVICE)
    they give the answers of the oracle's bytes."""
    from dcdf_amd import _lib as L
    from dcdf_amd.encoder import DeviceBuffer, Encoder
    for k in (3, 8, 9, 16):
        cs = [c for c in cases(k)[0] if c.T * c.R * c.C <= 60000]
        bufs, descs = [], []
        for c in cs:
            b = DeviceBuffer(c.a.nbytes)
            b.write(0, np.ascontiguousarray(c.a))
            bufs.append(b)
            code = {np.dtype(np.int32): L.DCDF_I32, np.dtype(np.int64): L.DCDF_I64, np.dtype(np.float32): L.DCDF_F32,
                    np.dtype(np.float64): L.DCDF_F64}[c.a.dtype]
            descs.append((b.ptr, code, (c.R * c.C, c.C, 1), c.a.shape, c.fbits))
        enc = Encoder(descs, k=k)
        enc.run()
        chunks = enc.open_chunks()
        for ch, c in zip(chunks, cs):
            assert ch.write_to() == c.data, c
            check_queries(dc, ch, c, full=False)
        check_batches(dc, cs, chunks, seed=k + 1000, n=20)
        for ch in chunks:
            ch.close()
        enc.close()
        for b in bufs:
            b.free()
