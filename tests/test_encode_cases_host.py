"""The case table of tests/encode_cases.py checked without a GPU: it covers every fused kernel class for every element
type, its contents have the properties they are named for, its error tiles fail in the oracle as announced, and the kernel
bodies (host simulator) agree with the oracle over the whole matrix up to sidelen 64.  tests/test_gpu_encode_classes.py
runs the same table from device views on the card."""
import numpy as np
import pytest

import encode_cases as E
import oracle_lib as O
import sim_lib as S


def oracle_of(view, bits, round_):
    """(code, bytes, snapshots, logs) of Chunk::build on the view."""
    try:
        data, ns, nl, _ = O.chunk_build(view, fractional_bits=bits, round_=round_, want_snapshots=True)
        return 0, data, ns, nl
    except O.OracleError as e:
        return e.code, None, 0, 0


def stored_of(data, shape):
    """The stored integers of an encoded chunk (fixed point for floats, 0 = NaN)."""
    T, R, Cc = shape
    return O.Chunk(data).fill_window(0, T, 0, R, 0, Cc, dtype=np.int64)


def test_table_covers_every_kernel_class_and_dtype():
    seen = set()
    for L in E.LEVELS:
        for dtype in E.DTYPES:
            names = []
            for name, expected, make in E.views(L, dtype):
                buf = E.aligned_buffer(make.nbytes, dtype)
                off, strides, shape = make(buf)
                assert buf.ctypes.data % 16 == 0
                got = E.classify(buf.ctypes.data + off, dtype, strides, shape)
                assert got == (L,) + tuple(expected), (L, np.dtype(dtype).name, name, got)
                seen.add((L, expected, np.dtype(dtype).name))
                names.append(name)
            assert len(set(names)) == len(names)
    want = set()
    for L in E.LEVELS:
        for dtype in E.DTYPES:
            dn = np.dtype(dtype).name
            want |= {(L, (0, 0), dn), (L, (1, 0), dn), (L, (0, E.LOADER[np.dtype(dtype)]), dn)}
    assert len(want) == 60 and seen == want  # 5 x (P0_V0, P1_V0) x 4 types + 5 x one row loader per type


@pytest.mark.parametrize("dtype", E.DTYPES, ids=lambda d: np.dtype(d).name)
def test_contents_have_the_property_they_are_named_for(dtype):
    L = 5
    Sd, T = 1 << L, E.instants(L)
    shape = (T, Sd, Sd)
    got = {}
    for kind in E.kinds(dtype):
        a, bits, rnd = E.contents(kind, shape, dtype, E.seeded("property", kind))
        assert a.dtype == np.dtype(dtype) and a.shape == shape
        code, data, ns, nl = oracle_of(a, bits, rnd)
        assert code == 0, kind
        got[kind] = (a, bits, rnd, data, ns, nl, stored_of(data, shape))

    def dac_bytes(kind):  # byte planes of the Dac of instant 0's Snapshot maxima (dac.rs:37-44)
        d = O.snapshot_dump(got[kind][6][0])
        return len(O.dac_dump(d["max"])["levels"])

    assert got["noise"][4:6] == (T, 0)                      # every instant a Snapshot
    assert got["sparse"][5] > 0 and got["sparse"][4] >= 1   # Logs
    assert dac_bytes("wide") >= 3 and dac_bytes("small") == 1
    assert len(got["const"][3]) < len(got["small"][3]) < len(got["wide"][3])
    assert got["const"][4] + got["const"][5] == T
    if not E.is_float(dtype):
        return
    assert got["small"][1] == 20 and got["wide"][1] == 3
    for kind in E.kinds(dtype):
        a, bits, rnd, _, _, _, stored = got[kind]
        scaled = a.astype(np.float64) * 2.0 ** bits
        frac = scaled - np.trunc(scaled)
        if kind == "nan_blocks":
            assert np.isnan(a[0, 4:8, 4:8]).all() and np.isnan(a[0, 8:16, 0:8]).all() and np.isnan(a[1]).all()
            assert np.isnan(a[2, 0]).all() and not np.isnan(a[2, 1]).any()
            assert np.isnan(a[3].reshape(-1)[::2]).all() and not np.isnan(a[3].reshape(-1)[1::2]).any()
            assert ((stored == 0) == np.isnan(a)).all()
        elif kind == "neg_fractions":
            share = ((frac != 0) & (scaled < 0)).mean()
            assert not rnd and 0.10 < share < 0.20 and not (frac > 0).any()
            groups = ((frac != 0).reshape(-1, 4)).any(axis=1)  # the 4-cell groups of the row loaders: some slow, some not
            assert 0.2 < groups.mean() < 0.8
        elif kind == "round_ties":
            ties = np.abs(frac) == 0.5
            assert rnd and 0.25 < ties.mean() < 0.35 and (ties & (scaled > 0)).any() and (ties & (scaled < 0)).any()
            assert (np.abs(frac)[~ties] == 0).all()
        elif kind == "subnormal":
            tiny = np.finfo(dtype).tiny
            sub = (a != 0) & (np.abs(a) < tiny)
            assert rnd and (sub & (a > 0)).any() and (sub & (a < 0)).any() and (np.signbit(a) & (a == 0)).any()
            assert (stored[sub] == 1).all()
        elif kind == "edge29":
            assert stored.max() == 2 * E.largest_below_2_29(dtype) + 1 < E.VALUE_LIMIT
            assert stored.min() == -E.VALUE_LIMIT + 1
        elif kind == "edge29_over":
            assert stored.max() == E.VALUE_LIMIT + 1  # outside the fused kernel's contract
    assert set(E.REROUTED_KINDS) == {"edge29_over"}


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("L", E.LEVELS)
def test_error_tiles_fail_in_the_oracle_as_expected(L, dtype):
    codes = []
    for name, x, bits, rnd, code in E.error_tiles(L, dtype):
        assert oracle_of(x, bits, rnd)[0] == code, name
        codes.append(code)
        # exactly one offending cell: the tile without it builds
        bad = ~np.isfinite(x) if code == E.ERR_NONFINITE else (np.abs(x) > 1e20) if code == E.ERR_OVERFLOW else \
            (x * 8 != np.trunc(x * 8))
        assert bad.sum() == 1
        y = x.copy()
        y[bad] = 0
        assert oracle_of(y, bits, rnd)[0] == 0
    assert sorted(codes) == [E.ERR_OVERFLOW, E.ERR_PRECISION, E.ERR_NONFINITE]


@pytest.mark.parametrize("dtype", E.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("L", [4, 5, 6])
def test_simulator_matches_the_oracle_over_the_matrix(L, dtype):
    """Every view x content kind through the kernel bodies: bytes, counters and status equal the oracle's.  The simulator
    chooses the loader by the library's rule from the view it is given; the generic-loader rows ask for it explicitly as well.
    A tile beyond the fused kernel's value contract is declined (-8) -- the library then hands it to the universal kernel."""
    for c in E.cases(L, dtype):
        novec = c.expected[1] == 0
        assert E.classify(c.view.ctypes.data, c.dtype, c.strides, c.shape) == (L,) + c.expected, c.name
        code, ref, rs, rl = oracle_of(c.view, c.bits, c.round)
        assert code == 0, c.name
        st, data, ns, nl, mm = S.encode(c.view, fractional_bits=c.bits, round_=c.round, force_novec=novec, want_minmax=True)
        if c.kind in E.REROUTED_KINDS:
            assert st == -8, c.name
            continue
        assert st == 0, (c.name, st)
        assert data == ref and (ns, nl) == (rs, rl), c.name
        stored = stored_of(ref, c.shape).reshape(c.shape[0], -1)
        assert (mm[:, 0] == stored.min(1)).all() and (mm[:, 1] == stored.max(1)).all(), c.name
    if E.is_float(dtype):
        for vname, expected, make in E.views(L, dtype):
            if vname not in ("dense", "base_plus_1", "padded_%dx%d_subtile" % ((1 << L) - 1, 1 << L)):
                continue
            buf = E.aligned_buffer(make.nbytes, dtype)
            off, strides, shape = make(buf)
            view = E.as_view(buf, off, strides, shape)
            for name, x, bits, rnd, code in E.error_tiles(L, dtype, shape=shape):
                view[...] = x
                assert oracle_of(view, bits, rnd)[0] == code
                assert S.encode(view, fractional_bits=bits, round_=rnd, force_novec=expected[1] == 0)[0] == code, (vname, name)
