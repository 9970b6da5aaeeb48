"""Bulk decode without a GPU: the entry point is declared and exported, and the Python wrappers lay out volumes and offsets for
reversed and empty cubes as fill_windows_flat does (the library call stubbed)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_and_exported():
    from dcdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    m = re.search(r"int dcdf_raster_decode_batch\(([^;]*)\);", hdr)
    assert m, "dcdf_raster_decode_batch is not declared"
    args = re.sub(r"\s+", " ", m.group(1))
    assert args == ("const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, void* out, int32_t out_dtype, int out_mem, "
                    "const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms")
    assert "dcdf_raster_decode_batch" in _lib.SYMBOLS
    so = _lib.LIB_PATH
    assert os.path.exists(so), "library not built"
    lib = C.CDLL(so)  # (loading needs no GPU)
    assert lib.dcdf_raster_decode_batch
    assert lib.dcdf_abi_version() == 3  # an added entry point: the ABI version stays


class _Stub:
    """Stands in for the loaded library: records what the two raster entry points are called with."""

    def __init__(self):
        self.calls = []

    def _record(self, name, h, cubes, nq, out, dtype, mem, off, *rest):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        self.calls.append((name, q, o, dtype, mem, out.value))
        return rest

    def dcdf_raster_fill_window_batch(self, *a):
        self._record("fill", *a)
        return 0

    def dcdf_raster_decode_batch(self, *a):
        stats, ms = self._record("decode", *a)
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0


def test_wrappers_lay_out_cubes_like_fill_windows_flat(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    R._native = C.c_void_p(1)  # (never dereferenced: the library is stubbed)
    try:
        cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 5], [0, 10, 50, 0, 0, 60], [1, 2, 3, 3, 4, 9]]
        for dt in (np.int32, np.float64):
            stub.calls.clear()
            fo, foff, _ = R.fill_windows_flat(cubes, dtype=dt)
            do, doff, ms, stats = R.decode_flat(cubes, dtype=dt)
            (fname, fq, fo2, fdt, fmem, _), (dname, dq, do2, ddt, dmem, _) = stub.calls
            assert (fname, dname) == ("fill", "decode")
            np.testing.assert_array_equal(fq, dq)
            np.testing.assert_array_equal(fo2, do2)
            np.testing.assert_array_equal(foff, doff)
            np.testing.assert_array_equal(doff, [0, 105, 105 + 420, 105 + 420, 105 + 420 + 30000])
            assert (fdt, fmem) == (ddt, dmem) and fo.shape == do.shape and fo.dtype == do.dtype == np.dtype(dt)
            assert stats.tolist() == [5, 6, 7]
        # device form: the caller's offsets go through untouched
        stub.calls.clear()
        ms, stats = R.decode_flat(cubes, dtype=np.int32, out_device_ptr=4096, out_offset=[9, 200, 700, 701, 40000])
        name, q, o, dt, mem, ptr = stub.calls[0]
        assert (name, mem, ptr) == ("decode", _lib.MEM_DEVICE, 4096) and o.tolist() == [9, 200, 700, 701, 40000]
        # decode(): one cube over the whole extent
        stub.calls.clear()
        a = R.decode(2, 7, dtype=np.float32)
        assert a.shape == (5, 50, 60) and a.dtype == np.float32
        assert stub.calls[0][1].tolist() == [[2, 7, 0, 50, 0, 60]]
        assert R.decode(3, 3).shape == (0, 50, 60) and len(stub.calls) == 1
        for bad in ((5, 4), (0, 11), (-1, 3)):
            try:
                R.decode(*bad)
            except ValueError:
                continue
            raise AssertionError("decode%r did not raise" % (bad,))
    finally:
        R._native = None


def test_split_rule_is_a_closed_form():
    """bulk_parts / bulk_part of k2r_bulk.h, restated: enough pieces for the device, none shorter than four instants, and the
    pieces tile [t0, t0 + nt) exactly."""
    def parts(n_units, nt, wanted):
        if n_units == 0 or n_units >= wanted:
            return 1
        return max(1, min(-(-wanted // n_units), nt // 4))

    for n_units, nt, wanted in [(1, 32, 1024), (16, 32, 1024), (600, 32, 1024), (2000, 32, 1024), (3, 5, 1024), (1, 3, 1024)]:
        p = parts(n_units, nt, wanted)
        edges = [7 + nt * j // p for j in range(p + 1)]
        assert edges[0] == 7 and edges[-1] == 7 + nt and all(b > a for a, b in zip(edges, edges[1:]))
        assert p == 1 or min(b - a for a, b in zip(edges, edges[1:])) >= 4


def test_numpy_model_of_the_rule_equals_the_oracle():
    """The identity the kernel is built on, pinned on the CPU: Snapshot pyramid once per block + each Log's own tree alone ==
    Chunk::fill_window of the oracle, on the chunks of the GPU leaf-kind test (full and padded) and on natural block policies."""
    import oracle_lib as O
    from bulk_model import decode_chunk, leaf_kinds_array
    a = leaf_kinds_array(np.random.default_rng(33))
    for shape in [(40, 256, 256), (40, 200, 131)]:
        x = np.ascontiguousarray(a[:, :shape[1], :shape[2]])
        data = O.chunk_build_forced(x, 2, 8)
        oc = O.Chunk(data)
        want = oc.fill_window(0, 40, 0, shape[1], 0, shape[2], dtype=np.int64)
        np.testing.assert_array_equal(want, x)
        np.testing.assert_array_equal(decode_chunk(data), want)
    for x in (np.ascontiguousarray(a[:24, :100, :77]), np.ascontiguousarray(a[:, :64, :64].astype(np.int32)), a[3:5, :9, :9].copy()):
        data = O.chunk_build(x)
        np.testing.assert_array_equal(decode_chunk(data), x)
