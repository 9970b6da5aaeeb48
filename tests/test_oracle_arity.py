"""The oracle across every arity the ABI takes (k = 2..16 to encode, up to 255 to open) against numpy on the raw arrays, so
that tests/test_gpu_arity.py can rely on it: get / fill_cell / fill_window / brute-force search on exact powers of k, padded,
1 x n, n x 1 and 1 x 1 shapes; the depth formula of snapshot.rs:118-119; the reference's panic on 1 x 1 chunks."""
import math

import numpy as np
import pytest

import oracle_lib as O

ARITIES = list(range(2, 17)) + [17, 32, 255]


def ref_sidelen(rows, cols, k):
    """snapshot.rs:118-119 in f64: k ^ ceil(ln(max) / ln(k))."""
    return k ** max(0, math.ceil(math.log(max(rows, cols)) / math.log(k)))


def shapes_for(k):
    """An exact power, a padded shape, a thin row, a thin column and a 1 x 1, kept small enough for a CPU decode."""
    h = 1
    while k ** (h + 1) <= 64:
        h += 1
    side = k ** h
    out = [(side, side), (side - 1, k ** (h - 1) + 1 if h > 1 else side - 1), (1, max(1, side - 1)), (side, 1), (1, 1)]
    return sorted(set((max(1, r), max(1, c)) for r, c in out))


def content(rng, T, R, Cc):
    """Log-friendly instants: noise, copies with a few changed cells, a region shifted by a constant, a uniform instant,
    fresh noise."""
    a = np.empty((T, R, Cc), dtype=np.int64)
    a[0] = rng.integers(-40, 40, size=(R, Cc))
    for t in range(1, T):
        a[t] = a[t - 1]
        idx = (rng.integers(0, R, size=3), rng.integers(0, Cc, size=3))
        a[t][idx] = rng.integers(-60, 60, size=3)
    if T > 3:
        a[2, : (R + 1) // 2] += 5
    if T > 4:
        a[4] = 17
    if T > 5:
        a[5] = rng.integers(-1000, 1000, size=(R, Cc))
    return a


def quirk_instants(a, snapshots):
    """Instants where the reference's search is not "the cells in range" (log.rs:527-548): a uniform
    log over a snapshot that is not uniform."""
    out = set()
    snap = 0
    for t in range(a.shape[0]):
        if t in snapshots:
            snap = t
            continue
        if (a[t] == a[t].flat[0]).all() and not (a[snap] == a[snap].flat[0]).all():
            out.add(t)
    return out


def brute(a, s, e, t, b, l, r, lo, hi, skip=()):
    sub = a[s:e, t:b, l:r]
    return set((int(i) + s, int(y) + t, int(x) + l) for i, y, x in zip(*np.nonzero((sub >= lo) & (sub <= hi)))
               if int(i) + s not in skip)


def windows(T, R, Cc, k):
    ws = [(0, T, 0, R, 0, Cc), (1, 2, R - 1, R, Cc - 1, Cc), (0, T, R // 2, R // 2 + 1, 0, Cc), (0, T, 0, R, Cc // 2, Cc // 2 + 1)]
    j = k
    while j < max(R, Cc):  # straddling the k^j node edges
        ws.append((0, T, min(max(0, j - 1), R - 1), min(R, j + 1), min(max(0, j - 2), Cc - 1), min(Cc, j + 1)))
        j *= k
    ws.append((T - 2, T, max(0, R - 3), R, max(0, Cc - 2), Cc))  # ending on the last real row / column
    return ws


@pytest.mark.parametrize("k", ARITIES)
def test_oracle_equals_numpy(k):
    rng = np.random.default_rng(1000 + k)
    T = 6
    for R, Cc in shapes_for(k):
        if R * Cc == 1:
            continue  # test_one_by_one_chunk_panics
        a = content(rng, T, R, Cc)
        data, ns, nl, snaps = O.chunk_build(a, k=k, want_snapshots=True)
        assert ns + nl == T and snaps[0] == 0
        c = O.Chunk(data)
        assert c.shape == (T, R, Cc) and c.serialize() == data
        for _ in range(60):
            i, r, cc = int(rng.integers(T)), int(rng.integers(R)), int(rng.integers(Cc))
            assert c.get(i, r, cc) == a[i, r, cc]
        for r, cc in [(0, 0), (R - 1, Cc - 1), (R // 2, Cc // 3)]:
            np.testing.assert_array_equal(c.fill_cell(0, T, r, cc), a[:, r, cc])
            np.testing.assert_array_equal(c.fill_cell(2, 5, r, cc), a[2:5, r, cc])
        quirk = quirk_instants(a, set(snaps))
        for s, e, t, b, l, r in windows(T, R, Cc, k):
            np.testing.assert_array_equal(c.fill_window(s, e, t, b, l, r), a[s:e, t:b, l:r])
            for lo, hi in [(-10, 10), (17, 17), (-1000, -41), (0, 0), (-5, 200)]:
                got = set(map(tuple, c.search(s, e, t, b, l, r, lo, hi).tolist()))
                assert set(x for x in got if x[0] not in quirk) == brute(a, s, e, t, b, l, r, lo, hi, quirk), (k, R, Cc, lo, hi)


@pytest.mark.parametrize("k", ARITIES)
def test_sidelen_follows_the_f64_depth_formula(k):
    dims = {1, 2, k - 1, k, k + 1, k * k - 1, k * k, k * k + 1, 125, 216, 1000}
    for n in sorted(d for d in dims if d >= 1):
        for rows, cols in [(n, 1), (1, n), (n, n)]:
            if ref_sidelen(rows, cols, k) > 1 << 20:
                continue
            assert O.sidelen(rows, cols, k) == ref_sidelen(rows, cols, k), (rows, cols, k)
    assert O.sidelen(125, 125, 5) == 625  # ln 125 / ln 5 = 3.0000000000000004: four levels, not three
    assert O.sidelen(216, 216, 6) == 1296  # the same: beyond what the universal encoder takes


def test_sidelen_in_the_encoded_bytes():
    """The first Snapshot's sidelen field (snapshot.rs:48-58) is the formula's, 1 for a 1 x 1 tile."""
    for k, (R, Cc) in [(5, (125, 125)), (2, (1, 1)), (9, (1, 1)), (3, (10, 1)), (10, (100, 100)), (11, (12, 3))]:
        data = O.chunk_build(np.zeros((1, R, Cc), dtype=np.int64), k=k)
        assert data[7] == k
        assert int.from_bytes(data[16:20], "big") == O.sidelen(R, Cc, k) == ref_sidelen(R, Cc, k)


@pytest.mark.parametrize("k", [2, 3, 8, 9, 16, 255])
def test_one_by_one_chunk_panics(k):
    """Snapshot::get on a 1 x 1 chunk reads nodemap.get(0) of an empty bitmap and panics (snapshot.rs:165-171,
    bitmap.rs:176-183); the oracle reports it as DCDF_ERR_BOUNDS.  The GPU returns the stored value instead (DESIGN.md
    section 6: tests/test_gpu_arity.py pins that side)."""
    a = np.arange(3, dtype=np.int64).reshape(3, 1, 1) * 7 - 4
    data, ns, nl, _ = O.chunk_build(a, k=k, want_snapshots=True)
    assert ns + nl == 3
    c = O.Chunk(data)
    assert c.shape == (3, 1, 1)
    for call in (lambda: c.get(0, 0, 0), lambda: c.get(2, 0, 0), lambda: c.fill_cell(0, 3, 0, 0),
                 lambda: c.fill_window(0, 3, 0, 1, 0, 1), lambda: c.search(0, 3, 0, 1, 0, 1, -100, 100)):
        with pytest.raises(O.OracleError) as e:
            call()
        assert e.value.code == -5


def test_forced_quirk_instants_at_higher_arity():
    """O.chunk_build_forced over a multi-node snapshot and a uniform instant (log.rs:527-548) at the arities
    test_gpu_arity.py uses: get / fill_window are exact, search equals brute force on the other instants and differs from it
    on the uniform one."""
    for k in (4, 8, 9, 16):
        side = k * k if k * k <= 64 else k + 3
        rng = np.random.default_rng(k)
        s = rng.integers(0, 40, size=(side, side)).astype(np.int64)
        a = np.stack([s, np.full((side, side), 23, dtype=np.int64), s + 1])
        c = O.Chunk(O.chunk_build_forced(a, k, 3))
        np.testing.assert_array_equal(c.fill_window(0, 3, 0, side, 0, side), a)
        assert c.get(1, side - 1, 0) == 23
        differs = False
        for lo, hi in [(0, 39), (10, 20), (23, 23), (-20, 5)]:
            got = set(map(tuple, c.search(0, 3, 0, side, 0, side, lo, hi).tolist()))
            assert set(x for x in got if x[0] != 1) == brute(a, 0, 3, 0, side, 0, side, lo, hi, {1})
            differs = differs or got != brute(a, 0, 3, 0, side, 0, side, lo, hi)
        assert differs


@pytest.mark.parametrize("k", [2, 4, 9])
def test_log_over_uniform_snapshot_root_test(k):
    """Log::search_window seeds min_s with snapshot.min.get(0) (log.rs:541-542), 0 for a single-node snapshot whose min Dac
    is empty (snapshot.rs:123-151): over a negative uniform snapshot the root's min is too high by its value, and the
    reference keeps or drops the whole window near the log's minimum.  The GPU returns the cells in range (DESIGN.md
    section 6, tests/test_gpu_arity.py)."""
    rng = np.random.default_rng(900 + k)
    side = 16
    logs = rng.integers(-200, 100, size=(2, side, side))
    a = np.concatenate([np.full((1, side, side), -27), logs]).astype(np.int64)
    c = O.Chunk(O.chunk_build_forced(a, k, 3))
    np.testing.assert_array_equal(c.fill_window(0, 3, 0, side, 0, side), a)
    m = int(logs.min())
    wrong = [(lo, hi) for lo, hi in [(m + 5, 500), (m, m + 10)]
             if set(map(tuple, c.search(0, 3, 0, side, 0, side, lo, hi).tolist())) != brute(a, 0, 3, 0, side, 0, side, lo, hi)]
    assert wrong
