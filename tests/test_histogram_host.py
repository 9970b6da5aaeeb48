"""Value histograms without a GPU: both entry points are declared and exported, the translation of bin edges into intervals of
stored integers (dcdf_histogram_bounds) agrees with the model the GPU tests compare with -- every encoding, the fractional bits
where the decoder rounds or its divisor wraps, ties on edges --, the Python wrappers lay out counts, offsets, masks and edges (the
library call stubbed), and the K2R_HD helpers of k2r_hist.h -- intervals, the bulk kernel's int32 threshold table and its
branch-free search, the fold's binning -- run in a stand-alone program built with AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hist_model as HM
from test_reduce_space_host import widen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
I32, I64, F32, F64 = 4, 8, 32, 64
FBITS = [0, 1, 25, 30, 61, 62]
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


def test_symbols_declared_and_exported():
    from dcdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    m = re.search(r"int dcdf_raster_histogram_batch\(([^;]*)\);", hdr)
    assert m, "dcdf_raster_histogram_batch is not declared"
    assert re.sub(r"\s+", " ", m.group(1)) == (
        "const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, const double* edges, uint32_t n_bins, const uint8_t* mask, "
        "const uint64_t* mask_offset, int mask_mem, uint64_t* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], "
        "float* kernel_ms")
    m = re.search(r"int dcdf_histogram_bounds\(([^;]*)\);", hdr)
    assert m, "dcdf_histogram_bounds is not declared"
    assert re.sub(r"\s+", " ", m.group(1)) == ("int32_t encoding, uint32_t fractional_bits, const double* edges, uint32_t n_bins, "
                                                "int64_t* lo, int64_t* hi")
    assert re.search(r"#define DCDF_HIST_MAX_BINS 256\b", hdr) and _lib.HIST_MAX_BINS == 256
    assert "dcdf_raster_histogram_batch" in _lib.SYMBOLS and "dcdf_histogram_bounds" in _lib.SYMBOLS
    so = _lib.LIB_PATH
    assert os.path.exists(so), "library not built"
    lib = C.CDLL(so)  # (loading needs no GPU)
    assert lib.dcdf_raster_histogram_batch and lib.dcdf_histogram_bounds
    assert lib.dcdf_abi_version() == 3  # added entry points: the ABI version stays


# ---- the translation against the model ----------------------------------------------------------------------------------------
def stored_integers(enc, rng):
    """A few thousand stored integers of a leaf: small ones, around +-2^24 / +-2^53 / +-2^62, the ends of the range."""
    near = np.arange(-40, 41, dtype=np.int64)
    parts = [rng.integers(-4096, 4096, 1500), rng.integers(-(1 << 30), 1 << 30, 300), rng.integers(-(1 << 62), 1 << 62, 300)]
    for p in (24, 53, 62):
        parts += [(1 << p) + near, -(1 << p) + near, (1 << p) + rng.integers(-(1 << (p - 3)), 1 << (p - 3), 150),
                  -(1 << p) + rng.integers(-(1 << (p - 3)), 1 << (p - 3), 150)]
    parts.append(np.array([INT64_MAX, INT64_MAX - 1, INT64_MIN + 1, INT64_MIN + 2, 1, 2, -1, 3, (1 << 53) + 3], dtype=np.int64))
    n = np.unique(np.concatenate([np.asarray(p, dtype=np.int64) for p in parts]))
    if enc == I32:
        n = np.unique(np.concatenate([n.astype(np.int32).astype(np.int64), np.array([-(1 << 31), (1 << 31) - 1], dtype=np.int64)]))
    if enc in (F32, F64):
        n = n[n != 0]  # (the NaN code)
    return n


def edge_sets(x, rng):
    """Edges among the decoded values themselves (ties on an edge certainly occur), with and without infinite ends."""
    u = np.unique(x)
    out = []
    for bins in (1, 2, 16, 40):
        pick = np.unique(rng.choice(u, size=min(bins + 1, u.size), replace=False))
        if pick.size >= 2:
            out.append(pick)
            out.append(np.concatenate([[-np.inf], pick, [np.inf]]))
    out.append(np.array([u[0], u[-1]]))            # one bin for everything: both ends closed
    out.append(np.array([-np.inf, np.inf]))
    mid = np.unique((u[:-1] + u[1:]) / 2)
    mid = mid[np.isfinite(mid)]
    if mid.size >= 2:
        out.append(np.unique(rng.choice(mid, size=min(9, mid.size), replace=False)))  # edges that are no decoded value
    return [e for e in out if e.size >= 2]


def check_bounds(enc, fb, n, edges):
    from dcdf_amd import _lib
    x = widen(enc, fb, n)
    lo, hi = _lib.histogram_bounds(enc, fb, edges)
    bins = edges.size - 1
    assert lo.shape == hi.shape == (bins,)
    want = HM.bin_index(edges, x)
    got = np.full(n.shape, -1, dtype=np.int64)
    hits = np.zeros(n.shape, dtype=np.int64)
    for b in range(bins):
        inside = (n >= lo[b]) & (n <= hi[b])
        got[inside] = b
        hits += inside
    assert (hits <= 1).all(), (enc, fb, "an integer in two bins")
    np.testing.assert_array_equal(got, want, err_msg="encoding %d, %d fractional bits, edges %r" % (enc, fb, edges[:4]))
    # the intervals are disjoint, and stored 0 of a float encoding ends none of them
    live = [(int(lo[b]), int(hi[b])) for b in range(bins) if lo[b] <= hi[b]]
    live.sort()
    for (l0, h0), (l1, h1) in zip(live, live[1:]):
        assert h0 < l1, (enc, fb, live)
    if enc in (F32, F64):
        assert all(l != 0 and h != 0 for l, h in live)


def test_histogram_bounds_agree_with_the_model():
    rng = np.random.default_rng(4242)
    for enc, bits in ((I32, [0]), (I64, [0]), (F32, FBITS), (F64, FBITS)):
        for fb in bits:
            n = stored_integers(enc, rng)
            x = widen(enc, fb, n)
            assert not np.isnan(x).any()
            if fb == 62:
                assert (np.diff(x) <= 0).all()  # the wrapped divisor: non-increasing in n
            else:
                assert (np.diff(x) >= 0).all()
            for edges in edge_sets(x, rng):
                check_bounds(enc, fb, n, edges)


def test_i64_rounds_beyond_2_pow_53():
    """n = 2^53 + 3 decodes to 2^53 + 4 as a double: it is binned as that value, although n itself is below the edge."""
    from dcdf_amd import _lib
    n = np.array([(1 << 53) + 1, (1 << 53) + 2, (1 << 53) + 3, (1 << 53) + 4, (1 << 53) + 5], dtype=np.int64)
    edges = np.array([0.0, float((1 << 53) + 4), float(1 << 54)])
    assert float((1 << 53) + 3) == float((1 << 53) + 4)
    lo, hi = _lib.histogram_bounds(I64, 0, edges)
    assert lo[1] == (1 << 53) + 3 and hi[0] == (1 << 53) + 2
    check_bounds(I64, 0, n, edges)
    # value search compares n itself here: the two calls differ on purpose
    vlo, vhi, _ = _lib.value_bounds(I64, 0, float((1 << 53) + 4), float(1 << 54))
    assert vlo == (1 << 53) + 4


def test_f32_collapses_beyond_2_pow_24_and_62_bits_reverse():
    from dcdf_amd import _lib
    n = np.arange((1 << 25) - 20, (1 << 25) + 40, dtype=np.int64)
    x = widen(F32, 3, n)
    assert np.unique(x).size < n.size  # many n, one value
    edges = np.unique(x)[::3]
    check_bounds(F32, 3, n, edges)
    lo, hi = _lib.histogram_bounds(F64, 62, np.array([-0.5, -0.25, 0.0, 0.25, 0.5]))
    live = [(int(a), int(b)) for a, b in zip(lo, hi)]
    assert all(a <= b for a, b in live) and all(live[b][0] > live[b + 1][1] for b in range(3)), live  # bins run against n


def test_histogram_bounds_error_codes():
    from dcdf_amd import _lib
    lib = _lib.lib()
    lo, hi = (C.c_int64 * 300)(), (C.c_int64 * 300)()

    def call(enc, fb, edges, bins=None, lo_=lo, hi_=hi):
        e = np.asarray(edges, dtype=np.float64)
        return lib.dcdf_histogram_bounds(enc, fb, e.ctypes.data if e.size else None, len(e) - 1 if bins is None else bins, lo_, hi_)

    assert call(F32, 3, [0.0, 1.0, 2.0]) == 0
    assert call(F32, 3, [0.0, np.nan, 2.0]) == -1
    assert call(F32, 3, [np.nan, 1.0]) == -1
    assert call(I32, 0, [0.0, 1.0, 1.0]) == -1          # equal
    assert call(I32, 0, [0.0, 2.0, 1.0]) == -1          # decreasing
    assert call(I32, 0, [np.inf, np.inf]) == -1
    assert call(I32, 0, [0.0, 1.0], bins=0) == -1
    assert call(I64, 0, np.arange(258.0)) == -1         # 257 bins
    assert call(I64, 0, np.arange(257.0)) == 0          # 256 bins
    assert call(F32, 63, [0.0, 1.0]) == -1 and call(F64, 63, [0.0, 1.0]) == -1
    assert call(F64, 62, [0.0, 1.0]) == 0
    assert call(I32, 63, [0.0, 1.0]) == 0               # (integers have no fractional bits to refuse)
    assert call(5, 0, [0.0, 1.0]) == -1 and call(0, 0, [0.0, 1.0]) == -1
    assert lib.dcdf_histogram_bounds(I32, 0, None, 1, lo, hi) == -1
    assert call(I32, 0, [0.0, 1.0], lo_=None) == -1 and call(I32, 0, [0.0, 1.0], hi_=None) == -1
    with pytest.raises(_lib.DcdfError):
        _lib.histogram_bounds(F32, 3, [1.0, 1.0])


# ---- the wrappers, the library call stubbed -----------------------------------------------------------------------------------
class _Stub:
    """Stands in for the loaded library: records what the entry point is called with."""

    def __init__(self):
        self.calls = []

    def dcdf_raster_histogram_batch(self, h, cubes, nq, edges, bins, mask, moff, mmem, out, mem, off, stats, ms):
        nq, bins = nq.value, bins.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        e = np.ctypeslib.as_array(C.cast(edges, C.POINTER(C.c_double)), shape=(bins + 1,)).copy()
        mo, mb = None, None
        if mask is not None:
            mo = np.ctypeslib.as_array(C.cast(moff, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
            if mmem == 0:
                n = np.abs((q[:, 3].astype(np.int64) - q[:, 2]) * (q[:, 5].astype(np.int64) - q[:, 4]))
                mb = [np.ctypeslib.as_array(C.cast(mask, C.POINTER(C.c_uint8)), shape=(int(mo[i] + n[i]) + 1,))[int(mo[i]):int(mo[i] + n[i])].copy()
                      for i in range(nq)]
        self.calls.append(dict(q=q, off=o, edges=e, bins=bins, mem=mem, out=out.value, mask=None if mask is None else mask.value, moff=mo,
                               mmem=mmem, mbytes=mb))
        if mem == 0:  # the host form's own array: a recognisable count per cube
            total = int(o[-1] + abs(int(q[-1, 1]) - int(q[-1, 0])) * bins) if nq else 0
            a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(max(total, 1),))
            for i in range(nq):
                a[int(o[i]):int(o[i]) + abs(int(q[i, 1]) - int(q[i, 0])) * bins] = i + 1
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0


def test_wrappers_lay_out_counts_masks_and_edges(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    R._native = C.c_void_p(1)  # (never dereferenced: the library is stubbed)
    try:
        #        3 instants         reversed: 3         none             10, reversed rows       1 instant, no rows
        cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 5], [0, 10, 50, 0, 0, 60], [1, 2, 3, 3, 4, 9]]
        for edges in ([0, 1], [-np.inf, 0, 2.5, np.inf], np.arange(257, dtype=np.int32), np.linspace(0, 1, 8, dtype=np.float32)):
            stub.calls.clear()
            bins = len(edges) - 1
            flat, off, ms, stats = R.histogram_flat(cubes, edges)
            c = stub.calls[0]
            assert c["bins"] == bins and c["mem"] == _lib.MEM_HOST and c["mask"] is None
            assert c["edges"].dtype == np.float64
            np.testing.assert_array_equal(c["edges"], np.asarray(edges, dtype=np.float64))  # edges go as float64
            np.testing.assert_array_equal(c["q"], cubes)  # (the library normalises reversed bounds itself)
            np.testing.assert_array_equal(off, [0, 3 * bins, 6 * bins, 6 * bins, 16 * bins])  # instants x bins; none: no space
            np.testing.assert_array_equal(c["off"], off)
            assert flat.dtype == np.uint64 and flat.size == 17 * bins and stats.tolist() == [5, 6, 7]
            assert (HM.cube(flat, off, 3, 10, bins) == 4).all() and HM.cube(flat, off, 1, 3, bins).shape == (3, bins)
        # masks: one per cube, None entries become all-ones, bool and uint8 alike, flattened to bytes
        stub.calls.clear()
        rng = np.random.default_rng(1)
        m0 = rng.random((5, 7)) < 0.5
        m3 = (rng.random((50, 60)) < 0.5).astype(np.uint8) * 200
        R.histogram_flat(cubes, [0, 1, 2], masks=[m0, None, None, m3, np.zeros((0, 5), dtype=bool)])
        c = stub.calls[0]
        assert c["mmem"] == _lib.MEM_HOST and c["moff"].tolist() == [0, 35, 175, 200, 3200]
        np.testing.assert_array_equal(c["mbytes"][0], m0.ravel().astype(np.uint8))
        assert (c["mbytes"][1] == 1).all() and c["mbytes"][1].size == 140
        np.testing.assert_array_equal(c["mbytes"][3], (m3 != 0).ravel().astype(np.uint8))
        stub.calls.clear()
        R.histogram_flat(cubes, [0, 1], masks=[None] * 5)  # nothing given: no mask at all
        assert stub.calls[0]["mask"] is None
        for bad in ([m0], [m0.T, None, None, None, None]):
            with pytest.raises(ValueError):
                R.histogram_flat(cubes, [0, 1], masks=bad)
        for bad in ([0.0], [], [0, 0], [1, 0], [0, np.nan, 1], np.arange(258), [[0, 1], [2, 3]]):
            with pytest.raises(ValueError):
                R.histogram_flat(cubes, bad)
        # device forms: the caller's offsets and mask pointer go through untouched
        stub.calls.clear()
        ms, stats = R.histogram_flat(cubes, [0, 1, 2, 3], masks=(8192, [0, 64, 128, 192, 4096]), out_device_ptr=4096, out_offset=[9, 20, 70, 71, 400])
        c = stub.calls[0]
        assert (c["bins"], c["mem"], c["out"], c["mask"], c["mmem"]) == (3, _lib.MEM_DEVICE, 4096, 8192, _lib.MEM_DEVICE)
        assert c["off"].tolist() == [9, 20, 70, 71, 400] and c["moff"].tolist() == [0, 64, 128, 192, 4096]
        # histogram(): one cube, [instants, bins]
        stub.calls.clear()
        h = R.histogram([0, 1, 2, 3, 4], 2, 7)
        assert h.shape == (5, 4) and h.dtype == np.uint64 and (h == 1).all()
        assert stub.calls[0]["q"].tolist() == [[2, 7, 0, 50, 0, 60]]
        h = R.histogram([0.5, 1.5], window=(3, 10, 20, 60), mask=np.ones((7, 40), dtype=bool))
        assert h.shape == (10, 1) and stub.calls[1]["q"].tolist() == [[0, 10, 3, 10, 20, 60]] and stub.calls[1]["mbytes"][0].size == 280
        h = R.histogram([0, 1, 2], 3, 3)  # no instants: nothing to read
        assert len(stub.calls) == 2 and h.shape == (0, 2) and h.dtype == np.uint64
        for bad in (dict(start=5, stop=4), dict(stop=11), dict(start=-1, stop=3), dict(window=(0, 51, 0, 60)), dict(window=(4, 3, 0, 60)),
                    dict(mask=np.ones((50, 61), dtype=bool)), dict(window=(0, 5, 0, 5), mask=np.ones((50, 60), dtype=bool))):
            with pytest.raises(ValueError):
                R.histogram([0, 1], **bad)
    finally:
        R._native = None


# ---- the helpers of k2r_hist.h on the CPU -------------------------------------------------------------------------------------
def test_helpers_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/sim/hist_check.cpp over k2r_hist.h, host code only, with AddressSanitizer and UBSan: the intervals, the bulk kernel's
    int32 threshold table with its branch-free search, and the fold's binning of the decoded value -- all three against the model."""
    exe = str(tmp_path / "hist_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", exe, os.path.join(HERE, "sim", "hist_check.cpp")])
    rng = np.random.default_rng(99)
    lines, want = [], []

    def add(enc, fb, edges, n):
        e = np.asarray(edges, dtype=np.float64)
        lines.append("L %d %d %d %s %d %s" % (enc, fb, e.size - 1, " ".join("%x" % int(v) for v in e.view(np.uint64)), n.size,
                                              " ".join(str(int(v)) for v in n)))
        want.append((enc, fb, e, n))

    for enc, bits in ((I32, [0]), (I64, [0]), (F32, FBITS), (F64, FBITS)):
        for fb in bits:
            n = stored_integers(enc, rng)
            narrow = n[np.abs(n) <= (1 << 30)]
            x = widen(enc, fb, n)
            for edges in edge_sets(x, rng)[:6] + edge_sets(widen(enc, fb, narrow), rng)[:6]:
                add(enc, fb, edges, np.concatenate([n, [0]]) if enc in (F32, F64) else n)
    big = np.sort(rng.choice(np.arange(-3000, 3000), 257, replace=False)).astype(np.float64)  # 256 bins: the largest table
    add(I32, 0, big, np.arange(-3100, 3100, dtype=np.int64))
    add(F32, 3, big / 16, np.arange(-3100, 3100, dtype=np.int64))
    add(F64, 62, np.sort(-(big[:66] - 1) / 2.0 ** 63), np.arange(-3100, 3100, dtype=np.int64))  # 65 bins, reversed
    add(I32, 0, [0.0, np.nan], np.array([1], dtype=np.int64))      # refused, not read
    add(F32, 63, [0.0, 1.0], np.array([1], dtype=np.int64))
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    assert got[-1] == "bad" and got[-2] == "bad"
    for line, (enc, fb, e, n) in zip(got[:-2], want[:-2]):
        words = line.split()
        assert words[-1] == "ok"
        a, b32, c = (np.array(words[k:-1:3], dtype=np.int64) for k in range(3))
        nan = (n == 0) if enc in (F32, F64) else np.zeros(n.shape, dtype=bool)
        model = np.full(n.shape, -1, dtype=np.int64)
        model[~nan] = HM.bin_index(e, widen(enc, fb, n[~nan]))
        np.testing.assert_array_equal(c, model)             # the fold's binning, NaN code included
        np.testing.assert_array_equal(a[~nan], model[~nan])  # the intervals
        narrow = (np.abs(n) <= (1 << 30)) & ~nan
        np.testing.assert_array_equal(b32[narrow], model[narrow])  # the bulk kernel's table and search
        assert (b32[~narrow] == -2).all()
