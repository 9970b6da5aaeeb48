"""Reduce over time without a GPU: the entry point is declared and exported, the Python wrappers lay out planes and offsets (the
library call stubbed), and the NumPy model the GPU tests compare with is pinned against the oracle and against exact integers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reduce_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_and_exported():
    from dcdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    m = re.search(r"int dcdf_raster_reduce_time_batch\(([^;]*)\);", hdr)
    assert m, "dcdf_raster_reduce_time_batch is not declared"
    args = re.sub(r"\s+", " ", m.group(1))
    assert args == ("const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, double* out, int out_mem, "
                    "const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms")
    assert re.search(r"enum \{ DCDF_REDUCE_MIN = 1, DCDF_REDUCE_MAX = 2, DCDF_REDUCE_SUM = 4, DCDF_REDUCE_COUNT = 8, DCDF_REDUCE_MEAN = 16 \};", hdr)
    assert "dcdf_raster_reduce_time_batch" in _lib.SYMBOLS
    assert _lib.REDUCE_OPS == M.BIT and tuple(_lib.REDUCE_OPS) == M.NAMES
    so = _lib.LIB_PATH
    assert os.path.exists(so), "library not built"
    lib = C.CDLL(so)  # (loading needs no GPU)
    assert lib.dcdf_raster_reduce_time_batch
    assert lib.dcdf_abi_version() == 3  # an added entry point: the ABI version stays


class _Stub:
    """Stands in for the loaded library: records what the entry point is called with."""

    def __init__(self):
        self.calls = []

    def dcdf_raster_reduce_time_batch(self, h, cubes, nq, ops, out, mem, off, stats, ms):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        self.calls.append((q, o, ops.value, mem, out.value))
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0


def test_wrappers_lay_out_planes(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    R._native = C.c_void_p(1)  # (never dereferenced: the library is stubbed)
    try:
        #        5 x 7            reversed: 7 x 20      no instants      reversed rows: 50 x 60  no rows
        cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 5], [0, 10, 50, 0, 0, 60], [1, 2, 3, 3, 4, 9]]
        for ops, mask in ((31, 31), (("mean",), 16), ("min", 1), (["count", "min", "sum"], 13), (np.uint32(6), 6)):
            stub.calls.clear()
            n = bin(mask).count("1")
            flat, off, ms, stats = R.reduce_time_flat(cubes, ops)
            q, o, got_mask, mem, _ = stub.calls[0]
            assert got_mask == mask and mem == _lib.MEM_HOST
            np.testing.assert_array_equal(q, cubes)  # (the library normalises reversed bounds itself)
            np.testing.assert_array_equal(off, [0, 35 * n, 175 * n, 175 * n, 3175 * n])
            np.testing.assert_array_equal(o, off)
            assert flat.dtype == np.float64 and flat.size == 3175 * n and stats.tolist() == [5, 6, 7]
        assert EncodedRaster.reduce_ops(["mean", "min", "count"]) == (25, ["min", "count", "mean"])  # plane order = bit order
        assert EncodedRaster.reduce_ops(31)[1] == list(M.NAMES)
        for bad in (0, 32, [], ["median"], "avg"):
            with pytest.raises(ValueError):
                EncodedRaster.reduce_ops(bad)
        # device form: the caller's offsets go through untouched
        stub.calls.clear()
        ms, stats = R.reduce_time_flat(cubes, ("sum", "max"), out_device_ptr=4096, out_offset=[9, 200, 700, 701, 40000])
        q, o, got_mask, mem, ptr = stub.calls[0]
        assert (got_mask, mem, ptr) == (6, _lib.MEM_DEVICE, 4096) and o.tolist() == [9, 200, 700, 701, 40000]
        # reduce_time(): one cube, a dict of planes in bit order
        stub.calls.clear()
        d = R.reduce_time(("mean", "min"), 2, 7)
        assert list(d) == ["min", "mean"] and all(v.shape == (50, 60) and v.dtype == np.float64 for v in d.values())
        assert stub.calls[0][0].tolist() == [[2, 7, 0, 50, 0, 60]] and stub.calls[0][2] == 17
        d = R.reduce_time(8, window=(3, 10, 20, 60))
        assert d["count"].shape == (7, 40) and stub.calls[1][0].tolist() == [[0, 10, 3, 10, 20, 60]]
        d = R.reduce_time(31, 3, 3)  # no instants: nothing to read
        assert len(stub.calls) == 2 and np.isnan(d["min"]).all() and np.isnan(d["mean"]).all() and (d["count"] == 0).all() and (d["sum"] == 0).all()
        for bad in (dict(start=5, stop=4), dict(stop=11), dict(start=-1, stop=3), dict(window=(0, 51, 0, 60)), dict(window=(4, 3, 0, 60))):
            with pytest.raises(ValueError):
                R.reduce_time("mean", **bad)
    finally:
        R._native = None


def test_model_against_the_oracle_and_exact_integers():
    """The model applied to the oracle's Chunk::fill_window of a forced-block chunk: for integers below 2^53 every statistic has
    an exact integer form to compare with, whatever way the model is written."""
    import oracle_lib as O
    from bulk_model import leaf_kinds_array
    a = np.ascontiguousarray(leaf_kinds_array(np.random.default_rng(33))[:, :200, :131])
    oc = O.Chunk(O.chunk_build_forced(a, 2, 8))
    w = oc.fill_window(0, 40, 0, 200, 0, 131, dtype=np.int64)
    np.testing.assert_array_equal(w, a)
    got = M.reduce_time(w)
    np.testing.assert_array_equal(got["min"], a.min(0).astype(np.float64))
    np.testing.assert_array_equal(got["max"], a.max(0).astype(np.float64))
    np.testing.assert_array_equal(got["sum"], a.sum(0).astype(np.float64))  # (|sum| < 2^53: exact in every order)
    np.testing.assert_array_equal(got["count"], np.full((200, 131), 40.0))
    np.testing.assert_array_equal(got["mean"], a.sum(0).astype(np.float64) / 40.0)
    part = M.reduce_time(oc.fill_window(5, 17, 3, 90, 7, 100, dtype=np.int32))
    np.testing.assert_array_equal(part["sum"], a[5:17, 3:90, 7:100].sum(0).astype(np.float64))


def test_model_skips_nan_rounds_and_keeps_the_order():
    x = np.array([1e16, 1.0, np.nan, -1e16, 1.0], dtype=np.float64).reshape(5, 1, 1)
    got = M.reduce_time(x)
    assert got["sum"][0, 0] == 1.0  # ((1e16 + 1) - 1e16) + 1 in order: the first 1 is absorbed; pairwise or sorted sums give 2 or 0
    assert got["count"][0, 0] == 4 and got["min"][0, 0] == -1e16 and got["max"][0, 0] == 1e16 and got["mean"][0, 0] == 0.25
    nan = M.reduce_time(np.full((3, 2, 2), np.nan, dtype=np.float32))
    for n in ("min", "max", "mean"):
        assert (nan[n].view(np.uint64) == np.array(np.nan).view(np.uint64)).all()
    assert (nan["sum"] == 0).all() and (nan["count"] == 0).all()
    big = np.array([2 ** 53 + 1, -(2 ** 62) - 1], dtype=np.int64).reshape(2, 1, 1)  # (double)n rounds to nearest even
    assert M.widen(big)[0, 0, 0] == float(2 ** 53) and M.widen(big)[1, 0, 0] == -float(2 ** 62)
    f = np.array([0.1], dtype=np.float32).reshape(1, 1, 1)  # float32 widens exactly
    assert M.reduce_time(f)["sum"][0, 0] == float(np.float32(0.1))
