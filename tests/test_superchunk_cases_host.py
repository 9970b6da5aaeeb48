"""The case table of tests/superchunk_cases.py checked without a GPU: every case goes through the Superchunk oracle, and the
table keeps its promises there -- the elided / link / reference counts it names, tiles that end up with different fractional
bits, a stored minimum of 0 exactly where a NaN lies behind the first number, the stated panic of every error case -- and the
k = 2 stores rebuild the source raster from leaf_grid's records alone (a check that does not depend on the oracle's own build
side).  tests/test_gpu_superchunk_cases.py runs the same table on the card, from host and from device views."""
import struct

import numpy as np
import pytest

import encode_cases as E
import oracle_lib as O
import oracle_superchunk as OS
import superchunk_cases as SC
from raster_rebuild import rebuild_from


def oracle_of(case):
    """(code, store, root cid, node bytes, stats) of Superchunk::build on the case's view."""
    store = OS.Store()
    try:
        obj, st = OS.superchunk_build(case.view, list(case.levels), case.k, store, case.bits, case.round)
    except O.OracleError as e:
        return e.code, None, None, None, None
    except ValueError as e:
        assert "tree levels" in str(e)
        return SC.ERR_BAD_ARG, None, None, None, None
    return 0, store, store.save(obj), obj, st


RESULTS = {}


def result(case):
    if case.name not in RESULTS:
        RESULTS[case.name] = oracle_of(case)
    return RESULTS[case.name]


def is_chunk(obj):
    return obj[6] == OS.NODE_MMSTRUCT3 and obj[7] == OS.NODE_SUBCHUNK


def is_superchunk(obj):
    return obj[6] == OS.NODE_MMSTRUCT3 and obj[7] == OS.NODE_SUPERCHUNK


def test_table_is_what_the_issue_lists():
    cs = SC.cases()
    tags = {t for c in cs for t in c.tags}
    assert {"arity", "nan_order", "nan", "fractions", "wide", "dedup", "views", "banded", "error", "two_causes", "nested"} <= tags
    assert {c.k for c in cs} == {2, 3, 4, 5, 16}
    assert {(c.dtype.name, c.view_name) for c in cs if "views" in c.tags} == {(d, v) for d in ("int32", "float32") for v in SC.VIEW_NAMES}
    for c in cs:
        lo, hi = E.extent(c.byte_offset, c.strides, c.shape, c.dtype.itemsize)
        assert 0 <= lo and hi <= c.buffer.nbytes, c.name
        assert c.shape[0] <= 8, c.name
        side = c.k ** sum(c.levels) // c.k ** c.levels[0]
        assert side <= 125 and (side <= 64 or c.k == 5), c.name  # tiles of at most 64 a side (k = 5: the one 125-tile of [1, 3])
    # every view of a base raster holds the same cells, but for the broadcast one (its last instant, every time)
    for d in ("int32", "float32"):
        dense = SC.by_name("view-%s-dense" % d).view
        for v in SC.VIEW_NAMES[1:-1]:
            np.testing.assert_array_equal(SC.by_name("view-%s-%s" % (d, v)).view, dense)
        np.testing.assert_array_equal(SC.by_name("view-%s-broadcast_instants" % d).view, np.broadcast_to(dense[-1], dense.shape))
    # the banded case: a tile row of every instant is exactly the MiB K2R_SC_BAND_MB=1 asks a band to hold
    for c in cs:
        if "banded" in c.tags:
            T, R, Cc = c.shape
            assert len(c.levels) == 2 and T * (c.k ** c.levels[1]) * Cc * c.dtype.itemsize == 1 << 20 and c.tile_rows() == 3


@pytest.mark.parametrize("case", SC.cases(), ids=lambda c: c.name)
def test_oracle_result_is_as_promised(case):
    code, store, root, obj, st = result(case)
    assert code == case.code, case.hits
    if code != 0:
        return
    ex = case.expect
    refs = [r for r in st["references"] if r is not None]
    if "elided" in ex:
        assert st["elided"] == ex["elided"]
    if "references" in ex:
        assert len(refs) == ex["references"]
    if "links" in ex:
        assert len(st["links"]) == ex["links"] == len(set(refs))
    if "children" in ex:
        assert sum(is_superchunk(o) for c, o in store.items() if c != root) == ex["children"]
    if "sidelen" in ex:
        assert struct.unpack_from(">I", obj, 8 + 12)[0] == ex["sidelen"]
    if "chunk_bits" in ex:
        bits = sorted(o[9] for o in store.values() if is_chunk(o))  # Chunk::write_to: encoding u8, fractional_bits u8
        assert bits == ex["chunk_bits"]
        if "fractions" in case.name:
            assert len(set(bits)) >= 4  # tiles of one raster with different bits
    assert st["elided"] + len(refs) == len(st["references"])


def test_two_causes_panic_at_the_first_tile_in_the_reference():
    """The reference builds tile by tile: tile 0's Round verdict panics before tile 3's infinity is ever looked at.  Each cause
    alone gives its own code."""
    c = SC.by_name("error-two_causes")
    assert result(c)[0] == SC.ERR_PRECISION and c.expect["codes"] == [SC.ERR_PRECISION, SC.ERR_NONFINITE]
    a = np.array(c.view)
    only_inf = a.copy()
    only_inf[1, 3, 3] = 0.25
    with pytest.raises(O.OracleError) as e:
        OS.superchunk_build(only_inf, c.levels, 2, OS.Store(), c.bits, False)
    assert e.value.code == SC.ERR_NONFINITE
    only_round = a.copy()
    only_round[0, 31, 31] = 0.25
    with pytest.raises(O.OracleError) as e:
        OS.superchunk_build(only_round, c.levels, 2, OS.Store(), c.bits, False)
    assert e.value.code == SC.ERR_PRECISION
    # and the Round verdict is suggest_fraction's, not to_fixed's: every (min, max) of the raster converts at 2 bits
    assert O.suggest_fraction(only_round[:, :16, :16]) == (True, 55)
    OS.min_max(only_round, c.bits, False)


def test_error_cases_have_one_cause_in_the_last_tile():
    for c in SC.error_cases():
        if "two_causes" in c.tags or c.code == SC.ERR_BAD_ARG or c.name == "round_verdict-refused":
            continue
        side = c.k ** sum(c.levels) // c.k ** c.levels[0]
        tiles = SC.tiles_of(c.shape, side)
        codes = []
        for top, bottom, left, right in tiles:
            sub = np.ascontiguousarray(c.view[:, top:bottom, left:right])
            try:
                OS.min_max(sub, c.bits, c.round)
                OS.compute_fractional_bits(sub, c.bits, c.round)
                codes.append(0)
            except O.OracleError as e:
                codes.append(e.code)
        assert codes == [0] * (len(tiles) - 1) + [c.code], c.name


@pytest.mark.parametrize("case", [c for c in SC.cases() if "nan" in c.tags], ids=lambda c: c.name)
def test_nan_order_minimum_is_zero_exactly_behind_the_first_number(case):
    """min_max of every tile and instant: the stored minimum is 0 (NaN) where the tile is all NaN or a NaN lies behind its first
    number, the maximum only where it is all NaN; everywhere else both are the stored minimum / maximum of the numbers."""
    for top, bottom, left, right in SC.tiles_of(case.shape, 32):
        sub = case.view[:, top:bottom, left:right]
        got = OS.min_max(np.ascontiguousarray(sub), case.bits, case.round)
        for t in range(case.shape[0]):
            flat = sub[t].reshape(-1)
            all_nan, behind = SC.nan_behind(flat)
            assert (got[t][0] == 0) == (all_nan or behind), (case.name, t, top, left)
            assert (got[t][1] == 0) == all_nan
            if not all_nan:
                assert got[t][1] == int(np.nanmax(flat) * 16) + 1
                if not behind:
                    assert got[t][0] == int(np.nanmin(flat) * 16) + 1
    if "nan_order" in case.tags:
        # the layouts are where they say: instant t of every tile holds its NaNs at the named positions and nowhere else
        for t, name in enumerate(case.expect["layouts"]):
            for top, bottom, left, right in SC.tiles_of(case.shape, 32):
                flat = case.view[t, top:bottom, left:right].reshape(-1)
                want = SC.nan_layouts(flat.size)[SC.LAYOUT_NAMES.index(name)][1]  # (a small tile's layout of the same rank)
                assert np.flatnonzero(np.isnan(flat)).tolist() == want
    else:
        _, store, root, obj, st = result(case)
        assert st["references"][1] is None and st["references"][2] is not None  # all NaN for good: elided; all but one instant: built
        t0 = case.view[:, :32, :32]
        assert np.signbit(t0[0, 3, 4]) and not np.signbit(t0[0, 20, 9]) and np.signbit(t0[1, 20, 9]) and t0[:2].min() == 0
        assert OS.min_max(np.ascontiguousarray(t0), 3, False)[0][0] == OS.min_max(np.ascontiguousarray(t0), 3, False)[1][0] == 1


def test_nan_layouts_cover_what_they_are_named_for():
    for n in (1024, 40, 160, 256):
        lay = dict(SC.nan_layouts(n))
        lead = 300 if n == 1024 else 30
        assert lay["leading_nans_first_number_at_%d" % lead] == list(range(lead))
        assert lay["first_number_at_%d_nan_at_%d" % (lead, lead + 1)][-2:] == [lead - 1, lead + 1]
        assert all(0 <= p < n for ps in lay.values() for p in ps) and len(lay) == 9
        flags = []
        for name, ps in SC.nan_layouts(n):
            flat = np.ones(n)
            flat[ps] = np.nan
            flags.append(SC.nan_behind(flat))
        assert flags == [(False, False)] * 3 + [(False, True)] * 5 + [(True, False)]
    big = dict(SC.nan_layouts(1024))
    assert big["nan_at_255"] == [255] and big["nan_at_256"] == [256] and big["nan_at_last_cell"] == [1023]
    # first number and NaN held by different threads and strides of a 256-thread loop
    assert 300 % 256 != 301 % 256 and 300 // 256 == 1 and 255 // 256 != 256 // 256


def through_fixed(v, bits):
    """from_fixed(to_fixed(v, bits, round = true)) of float64 numbers, fixed.rs:31-86 restated: only a positive fractional part is
    rounded (half away from zero); a negative one survives to the doubling and is truncated toward zero by to_i64 -- so a value in
    (-2^-bits, -2^-(bits + 1)] is stored as 0, which reads back as NaN.  The fractions rasters hold such a cell."""
    s = v * 2.0 ** bits
    s = np.where(s - np.trunc(s) > 0, np.floor(s + 0.5), s)
    n = np.trunc(s * 2) + 1
    return np.where(n == 0, np.nan, (n - 1) / 2.0 ** (bits + 1))


@pytest.mark.parametrize("case", [c for c in SC.good_cases() if c.k == 2], ids=lambda c: c.name)
def test_k2_store_rebuilds_the_source(case):
    _, store, root, obj, st = result(case)
    a = np.array(case.view)
    out, recs = rebuild_from(store, [root], a, case.levels, case.shape[0], case.round)
    if case.exact:
        np.testing.assert_array_equal(out, a)  # (NaN compares equal to NaN)
        return
    # every cell went through to_fixed with the bits of the chunk that holds it (each tile has its own) and back
    for s, t0, nt, r0, c0, h, w, lf, o in recs:
        bits = lf.fractional_bits if o is None else o[9]
        np.testing.assert_array_equal(out[:, r0:r0 + h, c0:c0 + w], through_fixed(a[:, r0:r0 + h, c0:c0 + w], bits), err_msg="%s %d %d" % (case.name, r0, c0))
    assert (out != a).any()
