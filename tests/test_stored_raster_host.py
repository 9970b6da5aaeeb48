"""leaf_grid on the CPU: stores written by the Superchunk oracle (tests/oracle_superchunk.py) are flattened into raster leaves, and
the source array is rebuilt from the records alone -- oracle Chunk.fill_window at (row0, col0) for chunk leaves, from_fixed of the
values for elided leaves.  Also checks each leaf's (min, max) against its holding tile and the `exact` rule."""
import numpy as np
import pytest

import oracle_lib as O
import oracle_superchunk as OS
from dcdf_amd.dataset import leaf_grid
from raster_rebuild import rebuild_from


def store_variable(a, levels, chunk_size, round_bits=None):
    """Superchunk::build of every chunk_size slice, as Variable.append does it: returns (store, segment cids)."""
    store, cids = OS.Store(), []
    round_ = round_bits is not None
    for t0 in range(0, a.shape[0], chunk_size):
        seg = np.ascontiguousarray(a[t0:t0 + chunk_size])
        fb = OS.compute_fractional_bits(seg, round_bits or 0, round_)
        obj, _ = OS.superchunk_build(seg, levels, 2, store, fb, round_)
        cids.append(store.save(obj))
    return store, cids


def rebuild(a, levels, chunk_size, round_bits=None):
    """The array rebuilt from leaf_grid's records, plus the records (with their raster positions) for further checks."""
    store, cids = store_variable(a, levels, chunk_size, round_bits)
    return rebuild_from(store, cids, a, levels, chunk_size, round_bits is not None)


def check_minmax_and_exact(a, recs, round_):
    """Chunk leaves: minmax is the (min, max) of the whole chunk's tile (integers: exactly), exact follows the rule; elided: min ==
    max == values."""
    for s, t0, nt, r0, c0, h, w, lf, obj in recs:
        if lf.cid is None:
            assert (lf.minmax[:, 0] == lf.values).all() and (lf.minmax[:, 1] == lf.values).all()
            continue
        ch = O.Chunk(obj[8:])
        _, rows, cols = ch.shape
        tile = a[t0:t0 + nt, r0 - lf.row0:r0 - lf.row0 + rows, c0 - lf.col0:c0 - lf.col0 + cols]
        if a.dtype.kind == "i":
            assert (lf.minmax[:, 0] == tile.min(axis=(1, 2))).all() and (lf.minmax[:, 1] == tile.max(axis=(1, 2))).all()
            assert lf.exact
        else:
            assert lf.exact == ((not round_) or obj[9] == lf.fractional_bits)


def test_uniform_blocks_16x16_levels_2_2():
    rng = np.random.default_rng(1)
    a = rng.integers(-50, 50, size=(40, 16, 16)).astype(np.int32)
    a[:, 4:8, 8:12] = 7                                    # uniform at every instant: elided
    a[:, 12:16, 0:4] = np.arange(40, dtype=np.int32)[:, None, None]  # uniform per instant, different values: elided too
    a[:20, 0:4, 0:4] = 3                                   # uniform in segment 0 only
    out, recs = rebuild(a, [2, 2], 16)
    np.testing.assert_array_equal(out, a)
    elided = [(s, r0, c0) for s, _, _, r0, c0, _, _, lf, _ in recs if lf.cid is None]
    assert (0, 4, 8) in elided and (2, 4, 8) in elided and (1, 12, 0) in elided and (0, 0, 0) in elided and (2, 0, 0) not in elided
    check_minmax_and_exact(a, recs, False)


def test_nested_fixture_shape_17x17_levels_1_2_2():
    rng = np.random.default_rng(2)
    a = rng.integers(-(1 << 40), 1 << 40, size=(21, 17, 17)).astype(np.int64)
    a[:, 0:8, 8:16] = -5  # one whole node of the middle level elided at the top
    out, recs = rebuild(a, [1, 2, 2], 8)
    np.testing.assert_array_equal(out, a)
    assert any(lf.cid is None and r0 < 8 and 8 <= c0 < 16 for _, _, _, r0, c0, _, _, lf, _ in recs)
    check_minmax_and_exact(a, recs, False)


def test_chunk_spanning_two_leaves_17x20_levels_1_3_1():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1000, size=(9, 17, 20)).astype(np.int32)
    out, recs = rebuild(a, [1, 3, 1], 4)
    np.testing.assert_array_equal(out, a)
    # the 1 x 4 top-level tile (row 16, cols 16..20) is one chunk built at the top level: two leaves of side 2 share it
    for s in range(3):
        pair = [lf for t, _, _, r0, c0, _, _, lf, _ in recs if t == s and r0 == 16 and c0 in (16, 18)]
        assert len(pair) == 2 and pair[0].cid == pair[1].cid is not None
        assert (pair[0].row0, pair[0].col0, pair[1].row0, pair[1].col0) == (0, 0, 0, 2)
    check_minmax_and_exact(a, recs, False)


def test_float_round_true():
    rng = np.random.default_rng(4)
    a = (rng.integers(-400, 400, size=(20, 16, 16)) / 8.0).astype(np.float32)  # needs 3 fractional bits
    a[:, 0:4, 4:8] = np.round(a[:, 0:4, 4:8])                                   # a tile that needs none
    a[:, 8:12, 8:12] = np.nan                                                     # all-NaN: elided, value 0
    a[:, 12:16, 12:16] = 2.5                                                      # constant: elided
    a[3, 4, 5] = np.nan
    out, recs = rebuild(a, [2, 2], 8, round_bits=3)
    np.testing.assert_array_equal(out, a)
    chunk_leaves = [lf for *_, lf, _ in recs if lf.cid is not None]
    assert any(lf.exact for lf in chunk_leaves) and not all(lf.exact for lf in chunk_leaves)
    nan_leaves = [lf for _, _, _, r0, c0, _, _, lf, _ in recs if (r0, c0) == (8, 8)]
    assert all(lf.cid is None and (lf.values == 0).all() for lf in nan_leaves)
    check_minmax_and_exact(a, recs, True)


def test_float64_not_rounded_is_exact():
    rng = np.random.default_rng(5)
    a = (rng.integers(-100, 100, size=(10, 8, 12)) / 4.0).astype(np.float64)
    a[:, 0:4, 0:4] = np.nan
    out, recs = rebuild(a, [2, 2], 5)
    np.testing.assert_array_equal(out, a)
    assert all(lf.exact for *_, lf, _ in recs)


def test_unrepresentable_tree_is_refused():
    a = np.arange(2 * 8 * 8, dtype=np.int32).reshape(2, 8, 8)
    store, cids = store_variable(a, [1, 2], 2)
    with pytest.raises(ValueError, match="not a Superchunk"):
        leaf_grid(store, [next(c for c, o in store.items() if o[6] == OS.NODE_LINKS)], [1, 2], False)
    b = np.arange(2 * 8 * 4, dtype=np.int32).reshape(2, 8, 4)
    store2, cids2 = store_variable(b, [1, 2], 2)
    store2.update(store)
    with pytest.raises(ValueError, match="shape"):
        leaf_grid(store2, cids + cids2, [1, 2], False)
