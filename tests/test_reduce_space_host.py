"""Reduce over space without a GPU: the entry point is declared and exported, the Python wrappers lay out series, offsets and masks
(the library call stubbed), the model the GPU tests compare with is pinned on the oracle's decode, the identity the kernels rest on
is checked in exact integers, and the K2R_HD helpers of k2r_space.h -- scale and add in 192 bits, round once -- run on the CPU:
through the pure-host export and in a stand-alone program built with AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import space_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
I32, I64, F32, F64 = 4, 8, 32, 64
ONE = 1 << 63


def test_symbol_declared_and_exported():
    from dcdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    m = re.search(r"int dcdf_raster_reduce_space_batch\(([^;]*)\);", hdr)
    assert m, "dcdf_raster_reduce_space_batch is not declared"
    args = re.sub(r"\s+", " ", m.group(1))
    assert args == ("const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint8_t* mask, "
                    "const uint64_t* mask_offset, int mask_mem, double* out, int out_mem, const uint64_t* out_offset, "
                    "uint64_t stats[3], float* kernel_ms")
    assert "dcdf_raster_reduce_space_batch" in _lib.SYMBOLS and "dcdf_space_fold_records" in _lib.SYMBOLS
    so = _lib.LIB_PATH
    assert os.path.exists(so), "library not built"
    lib = C.CDLL(so)  # (loading needs no GPU)
    assert lib.dcdf_raster_reduce_space_batch and lib.dcdf_space_fold_records
    assert lib.dcdf_abi_version() == 3  # added entry points: the ABI version stays


class _Stub:
    """Stands in for the loaded library: records what the entry point is called with."""

    def __init__(self):
        self.calls = []

    def dcdf_raster_reduce_space_batch(self, h, cubes, nq, ops, mask, moff, mmem, out, mem, off, stats, ms):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        mo, mb = None, None
        if mask is not None:
            mo = np.ctypeslib.as_array(C.cast(moff, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
            if mmem == 0:
                n = np.abs((q[:, 3].astype(np.int64) - q[:, 2]) * (q[:, 5].astype(np.int64) - q[:, 4]))
                mb = [np.ctypeslib.as_array(C.cast(mask, C.POINTER(C.c_uint8)), shape=(int(mo[i] + n[i]) + 1,))[int(mo[i]):int(mo[i] + n[i])].copy()
                      for i in range(nq)]
        self.calls.append(dict(q=q, off=o, ops=ops.value, mem=mem, out=out.value, mask=None if mask is None else mask.value, moff=mo, mmem=mmem,
                               mbytes=mb))
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0


def test_wrappers_lay_out_series_and_masks(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    R._native = C.c_void_p(1)  # (never dereferenced: the library is stubbed)
    try:
        #        3 instants         reversed: 3         none             10, reversed rows       1 instant, no rows
        cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 5], [0, 10, 50, 0, 0, 60], [1, 2, 3, 3, 4, 9]]
        for ops, bits in ((31, 31), (("mean",), 16), ("min", 1), (["count", "min", "sum"], 13), (np.uint32(6), 6)):
            stub.calls.clear()
            n = bin(bits).count("1")
            flat, off, ms, stats = R.reduce_space_flat(cubes, ops)
            c = stub.calls[0]
            assert c["ops"] == bits and c["mem"] == _lib.MEM_HOST and c["mask"] is None
            np.testing.assert_array_equal(c["q"], cubes)  # (the library normalises reversed bounds itself)
            np.testing.assert_array_equal(off, [0, 3 * n, 6 * n, 6 * n, 16 * n])
            np.testing.assert_array_equal(c["off"], off)
            assert flat.dtype == np.float64 and flat.size == 17 * n and stats.tolist() == [5, 6, 7]
        # masks: one per cube, None entries become all-ones, bool and uint8 alike, shapes against the normalised cube
        stub.calls.clear()
        rng = np.random.default_rng(1)
        m0 = rng.random((5, 7)) < 0.5
        m3 = (rng.random((50, 60)) < 0.5).astype(np.uint8) * 200
        R.reduce_space_flat(cubes, 16, masks=[m0, None, None, m3, np.zeros((0, 5), dtype=bool)])
        c = stub.calls[0]
        assert c["mmem"] == _lib.MEM_HOST and c["moff"].tolist() == [0, 35, 175, 200, 3200]
        np.testing.assert_array_equal(c["mbytes"][0], m0.ravel().astype(np.uint8))
        assert (c["mbytes"][1] == 1).all() and c["mbytes"][1].size == 140
        np.testing.assert_array_equal(c["mbytes"][3], (m3 != 0).ravel().astype(np.uint8))
        stub.calls.clear()
        R.reduce_space_flat(cubes, 16, masks=[None] * 5)  # nothing given: no mask at all
        assert stub.calls[0]["mask"] is None
        for bad in ([m0], [m0.T, None, None, None, None], [None, np.ones((20, 7), dtype=bool), None, None, None]):
            with pytest.raises(ValueError):
                R.reduce_space_flat(cubes, 16, masks=bad)
        # device forms: the caller's offsets and mask pointer go through untouched
        stub.calls.clear()
        ms, stats = R.reduce_space_flat(cubes, ("sum", "max"), masks=(8192, [0, 64, 128, 192, 4096]), out_device_ptr=4096, out_offset=[9, 20, 70, 71, 400])
        c = stub.calls[0]
        assert (c["ops"], c["mem"], c["out"], c["mask"], c["mmem"]) == (6, _lib.MEM_DEVICE, 4096, 8192, _lib.MEM_DEVICE)
        assert c["off"].tolist() == [9, 20, 70, 71, 400] and c["moff"].tolist() == [0, 64, 128, 192, 4096]
        # reduce_space(): one cube, a dict of series in bit order
        stub.calls.clear()
        d = R.reduce_space(("mean", "min"), 2, 7)
        assert list(d) == ["min", "mean"] and all(v.shape == (5,) and v.dtype == np.float64 for v in d.values())
        assert stub.calls[0]["q"].tolist() == [[2, 7, 0, 50, 0, 60]] and stub.calls[0]["ops"] == 17
        d = R.reduce_space(8, window=(3, 10, 20, 60), mask=np.ones((7, 40), dtype=bool))
        assert d["count"].shape == (10,) and stub.calls[1]["q"].tolist() == [[0, 10, 3, 10, 20, 60]] and stub.calls[1]["mbytes"][0].size == 280
        d = R.reduce_space(31, 3, 3)  # no instants: nothing to read
        assert len(stub.calls) == 2 and list(d) == list(SM.NAMES) and all(v.shape == (0,) for v in d.values())
        for bad in (dict(start=5, stop=4), dict(stop=11), dict(start=-1, stop=3), dict(window=(0, 51, 0, 60)), dict(window=(4, 3, 0, 60)),
                    dict(mask=np.ones((50, 61), dtype=bool)), dict(window=(0, 5, 0, 5), mask=np.ones((50, 60), dtype=bool))):
            with pytest.raises(ValueError):
                R.reduce_space("mean", **bad)
        with pytest.raises(ValueError):
            R.reduce_space("median")
    finally:
        R._native = None


def test_model_on_the_oracles_decode_with_elided_tiles():
    """The model applied to what the oracle decodes from stored Superchunks with elided tiles: where every statistic has an exact
    integer or rational form, that form, whatever way the model is written."""
    import test_stored_raster_host as SH
    rng = np.random.default_rng(11)
    a = rng.integers(-5000, 5000, size=(12, 16, 16)).astype(np.int32)
    a[:, 4:8, 8:12] = 7                                              # elided: constant
    a[:, 12:16, 0:4] = np.arange(12, dtype=np.int32)[:, None, None]  # elided: one value per instant
    w, recs = SH.rebuild(a, [2, 2], 5)
    assert any(lf.cid is None for *_, lf, _ in recs)
    np.testing.assert_array_equal(w, a)
    mask = rng.random((16, 16)) < 0.5
    mask[4:6, 8:12] = True   # (straddles the elided tile's edge)
    mask[6:8, 8:12] = False
    for m in (None, mask):
        got = SM.reduce_space(w, m)
        sel = a.reshape(12, -1) if m is None else a.reshape(12, -1)[:, m.ravel()]
        np.testing.assert_array_equal(got["sum"], sel.sum(1).astype(np.float64))  # (|sum| < 2^53: exact)
        np.testing.assert_array_equal(got["min"], sel.min(1).astype(np.float64))
        np.testing.assert_array_equal(got["max"], sel.max(1).astype(np.float64))
        np.testing.assert_array_equal(got["count"], np.full(12, float(sel.shape[1])))
        np.testing.assert_array_equal(got["mean"], sel.sum(1).astype(np.float64) / sel.shape[1])
    f = (rng.integers(-400, 400, size=(10, 16, 16)) / 8.0).astype(np.float32)
    f[:, 8:12, 8:12] = np.nan   # elided, NaN at every instant
    f[:, 12:16, 12:16] = 2.5    # elided, constant
    f[3, 4, 5] = np.nan
    w, recs = SH.rebuild(f, [2, 2], 4, round_bits=3)
    assert sum(lf.cid is None for *_, lf, _ in recs) >= 6
    got = SM.reduce_space(w, mask)
    for t in range(10):
        v = [Fraction(float(x)) for x in w[t][mask] if not np.isnan(x)]
        assert got["sum"][t] == float(sum(v)) and got["count"][t] == len(v) and got["min"][t] == float(min(v)) and got["max"][t] == float(max(v))
        assert got["mean"][t] == got["sum"][t] / len(v)
    none = SM.reduce_space(w, np.zeros((16, 16), dtype=bool))
    only_nan = np.zeros((16, 16), dtype=bool)
    only_nan[8:12, 8:12] = True
    for g in (none, SM.reduce_space(w, only_nan)):
        for n in ("min", "max", "mean"):
            assert (g[n].view(np.uint64) == np.array(np.nan).view(np.uint64)).all()
        assert (g["sum"].view(np.uint64) == 0).all() and (g["count"] == 0).all()
    flat = np.arange(40, dtype=np.float64)
    s = SM.series(flat, [0, 7], 1, 1 | 4 | 16, 5)
    assert list(s) == ["min", "sum", "mean"] and s["sum"].tolist() == [12, 13, 14, 15, 16]


# ---- the identity the kernels rest on ---------------------------------------------------------------------------------------
def widen(enc, fbits, n):
    """reduce_widen (k2r_reduce.h) in NumPy: the typed value of the stored integer n (n != 0 for floats), widened to float64."""
    n = np.asarray(n, dtype=np.int64)
    if enc == I32:
        return n.astype(np.int32).astype(np.float64)
    if enc == I64:
        return n.astype(np.float64)
    div = -(2.0 ** 63) if fbits == 62 else 2.0 ** (fbits + 1)  # ((int64_t)1 << 63 is negative: the wrapped divisor)
    if enc == F32:
        return ((n - 1).astype(np.float32) / np.float32(div)).astype(np.float64)
    return (n - 1).astype(np.float64) / div


EXTREMES = [-(1 << 63) + 1, (1 << 63) - 1, 1 << 30, -(1 << 30), 1, 2, (1 << 24) + 2, (1 << 24) + 4, -(1 << 24) - 1, (1 << 53) + 2, (1 << 53) + 4,
            -(1 << 53) - 2, (1 << 62) + 12345, -(1 << 62) - 54321, 3, -7]
FBITS = [0, 1, 23, 25, 52, 61, 62]


def leaf_cases():
    rng = np.random.default_rng(2025)
    out = []
    for enc, bits in ((I32, [0]), (I64, [0]), (F32, FBITS), (F64, FBITS)):
        for fb in bits:
            n = np.concatenate([rng.integers(-(1 << 62), 1 << 62, 200), rng.integers(-(1 << 30), 1 << 30, 200), rng.integers(-(1 << 12), 1 << 12, 100),
                                np.array(EXTREMES, dtype=np.int64)])
            if enc == I32:
                n = n.astype(np.int32).astype(np.int64)
            if enc in (F32, F64):
                n = n[n != 0]
            out.append((enc, fb, n))
    return out


def test_every_value_is_an_integer_multiple_of_2_pow_minus_63_and_integer_sums_are_fsum():
    scaled_all, x_all = [], []
    for enc, fb, n in leaf_cases():
        x = widen(enc, fb, n)
        assert not np.isnan(x).any() and (np.abs(x) <= 2.0 ** 63).all()
        scaled = [Fraction(float(v)) * ONE for v in x]
        assert all(s.denominator == 1 for s in scaled), (enc, fb)
        ints = [int(s) for s in scaled]
        assert float(Fraction(sum(ints), ONE)) == math.fsum(x.tolist()), (enc, fb)
        scaled_all += ints
        x_all += x.tolist()
    # a mix of scales in one sum
    assert float(Fraction(sum(scaled_all), ONE)) == math.fsum(x_all)
    order = np.random.default_rng(3).permutation(len(x_all))
    assert math.fsum([x_all[i] for i in order]) == math.fsum(x_all)


# ---- the helpers of k2r_space.h on the CPU -----------------------------------------------------------------------------------
def rounding_cases():
    """[(records, exact Fraction)]: records = [(integer within 128 signed bits, shift, negative)]."""
    cases = []

    def add(recs):
        cases.append((recs, Fraction(sum((-v if g else v) << s for v, s, g in recs), ONE)))

    add([])                                                   # nothing: +0.0
    add([(5, 0, False), (5, 0, True)])                         # cancels to 0
    add([(1, 0, False)])                                       # 2^-63, the smallest step
    add([((1 << 53) + 1, 0, False)])                           # tie: down to even
    add([((1 << 53) + 3, 0, False)])                           # tie: up to even
    add([((1 << 53) + 1, 1, False), (1, 0, False)])            # just above a tie: up
    add([((1 << 53) + 1, 1, False), (1, 0, True)])             # just below a tie: down
    add([((1 << 54) - 1, 0, False)])                           # rounds up across a power of two
    add([((1 << 54) - 1, 10, False), (1 << 9, 0, False)])      # the same, the half bit from another record
    add([((1 << 54) - 1, 0, True)])                            # negative, across a power of two
    add([((1 << 53) + 1, 7, True)])                            # negative tie
    add([((1 << 94) + (1 << 41), 63, False)])                  # 2^94-sized: a tie at 2^157 / 2^63
    add([((1 << 94) + (1 << 41) + 1, 63, True)])
    add([(-(1 << 94) - 12345678901234567, 63, False), (987654321987654321, 62, True)])
    add([((1 << 127) - 1, 63, False)])                         # the largest record
    add([(-(1 << 127), 63, False)])
    add([(-(1 << 127), 63, True)])
    add([((1 << 63), 0, False)] * 3 + [(1, 63, False)])
    rng = np.random.default_rng(77)
    for _ in range(300):
        k = int(rng.integers(1, 9))
        recs = []
        for _ in range(k):
            width = int(rng.integers(1, 127))
            v = int.from_bytes(rng.bytes(16), "little") >> (128 - width)
            recs.append((-v if rng.random() < 0.5 else v, int(rng.integers(0, 64)), bool(rng.random() < 0.3)))
        add(recs)
    for _ in range(200):  # near ties: a 54-bit odd integer at some shift, plus or minus a little something far below
        q = int(rng.integers(1 << 53, 1 << 54)) | 1
        s = int(rng.integers(1, 60))
        recs = [(q, s, False)]
        eps = int(rng.integers(0, 3)) - 1
        if eps:
            recs.append((1, int(rng.integers(0, s)), eps < 0))
        add(recs)
    return cases


def test_space_fold_records_rounds_once_to_nearest_even():
    from dcdf_amd import _lib
    for recs, exact in rounding_cases():
        got = _lib.space_fold_records(recs)
        want = float(exact)  # (Fraction -> float is correctly rounded, ties to even)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (recs, got, want)
    assert math.copysign(1.0, _lib.space_fold_records([])) == 1.0  # +0.0
    lib = _lib.lib()
    out = C.c_double()
    one = (C.c_uint64 * 1)(1)
    assert lib.dcdf_space_fold_records(one, one, (C.c_uint32 * 1)(64), 1, C.byref(out)) == -1   # a shift beyond 63
    assert lib.dcdf_space_fold_records(one, one, (C.c_uint32 * 1)(512), 1, C.byref(out)) == -1
    assert lib.dcdf_space_fold_records(None, one, (C.c_uint32 * 1)(0), 1, C.byref(out)) == -1
    assert lib.dcdf_space_fold_records(one, one, (C.c_uint32 * 1)(0), 1, None) == -1


def test_helpers_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/sim/space_check.cpp over k2r_space.h, host code only, with AddressSanitizer and UBSan: per-cell records of every
    encoding (space_m, space_add_m, space_scale), elided pieces (space_mul_m), raw records -- against exact rationals."""
    exe = str(tmp_path / "space_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", exe, os.path.join(HERE, "sim", "space_check.cpp")])
    lines, want = [], []
    cells = []
    for enc, fb, n in leaf_cases():
        x = widen(enc, fb, n)
        group = [(enc, fb, int(v)) for v in n]
        lines.append("C %d %s" % (len(group), " ".join("%d %d %d" % g for g in group)))
        want.append(("C", math.fsum(x.tolist()), x))
        cells += list(zip(group, x.tolist()))
    pick = np.random.default_rng(8).permutation(len(cells))[:1500]   # every scale in one sum
    lines.append("C %d %s" % (len(pick), " ".join("%d %d %d" % cells[i][0] for i in pick)))
    want.append(("C", math.fsum([cells[i][1] for i in pick]), np.array([cells[i][1] for i in pick])))
    for (enc, fb, n), x in [cells[i] for i in pick[:200]]:
        for cnt in (0, 1, 4096, (1 << 32) - 1):
            lines.append("E %d %d %d %d" % (enc, fb, n, cnt))
            want.append(("E", float(Fraction(x) * cnt), None))
    for recs, exact in rounding_cases():
        lines.append("R %d %s" % (len(recs), " ".join("%d %d %d" % ((v >> 64) & (2 ** 64 - 1), v & (2 ** 64 - 1), s | (256 if g else 0)) for v, s, g in recs)))
        want.append(("R", float(exact), None))
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for line, (kind, s, x) in zip(got, want):
        words = [int(w, 16) for w in line.split()]
        assert words[0] == int(np.float64(s).view(np.uint64)), (kind, line[:40], s)
        if kind == "C":  # the program's decoded values are the NumPy model's
            np.testing.assert_array_equal(np.array(words[1:], dtype=np.uint64), x.view(np.uint64))
