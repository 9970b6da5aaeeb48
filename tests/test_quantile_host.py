"""Quantiles over time without a GPU: the entry point is declared and exported, the Python wrappers lay out planes and offsets (the
library call stubbed), the NumPy model the GPU tests compare with is pinned against a per-cell loop and against numpy.nanquantile,
the selection of the shipped library (its host form) agrees with the model, the inputs of the GPU tests are shown to hold ties, NaN
instants, cells with one and with no value, and tests/sim/quantile_check.cpp runs the keys, the selection loop and the planner on
the CPU under AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import quantile_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PROBS = [0, 0.1, 0.5, 0.9, 1]


def test_symbol_declared_and_exported():
    from dcdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    m = re.search(r"int dcdf_raster_quantile_time_batch\(([^;]*)\);", hdr)
    assert m, "dcdf_raster_quantile_time_batch is not declared"
    args = re.sub(r"\s+", " ", m.group(1))
    assert args == ("const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, const double* probs, uint32_t n_probs, int32_t method, "
                    "double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms")
    assert re.search(r"enum \{ DCDF_QUANTILE_LOWER = 0, DCDF_QUANTILE_HIGHER = 1, DCDF_QUANTILE_NEAREST = 2, DCDF_QUANTILE_LINEAR = 3 \};", hdr)
    assert "dcdf_raster_quantile_time_batch" in _lib.SYMBOLS and "dcdf_quantile_select_host" in _lib.SYMBOLS
    assert _lib.QUANTILE_METHODS == {"lower": 0, "higher": 1, "nearest": 2, "linear": 3} == M.METHODS
    so = _lib.LIB_PATH
    assert os.path.exists(so), "library not built"
    lib = C.CDLL(so)  # (loading needs no GPU)
    assert lib.dcdf_raster_quantile_time_batch and lib.dcdf_quantile_select_host
    assert lib.dcdf_abi_version() == 3  # an added entry point: the ABI version stays


class _Stub:
    """Stands in for the loaded library: records what the entry point is called with."""

    def __init__(self):
        self.calls = []

    def dcdf_raster_quantile_time_batch(self, h, cubes, nq, probs, n_probs, method, out, mem, off, stats, ms):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        p = np.ctypeslib.as_array(C.cast(probs, C.POINTER(C.c_double)), shape=(n_probs.value,)).copy()
        self.calls.append((q, o, p, method.value, mem, out.value))
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
        for probs, method, code in ((PROBS, "linear", 3), ([0.5], "lower", 0), (0.25, "higher", 1), (np.linspace(0, 1, 16), "nearest", 2), ([0.3, 0.3], 3, 3)):
            stub.calls.clear()
            n = np.asarray(probs).size
            flat, off, ms, stats = R.quantile_time_flat(cubes, probs, method)
            q, o, p, got_code, mem, _ = stub.calls[0]
            assert got_code == code and mem == _lib.MEM_HOST and p.tolist() == np.asarray(probs, dtype=np.float64).reshape(-1).tolist()
            np.testing.assert_array_equal(q, cubes)  # (the library normalises reversed bounds itself)
            np.testing.assert_array_equal(off, [0, 35 * n, 175 * n, 175 * n, 3175 * n])
            np.testing.assert_array_equal(o, off)
            assert flat.dtype == np.float64 and flat.size == 3175 * n and stats.tolist() == [5, 6, 7]
        stub.calls.clear()
        R.quantile_time_flat(cubes, 0.5)  # the default method
        assert stub.calls[0][3] == 3
        # device form: the caller's offsets go through untouched
        stub.calls.clear()
        ms, stats = R.quantile_time_flat(cubes, [0.1, 0.9], "lower", out_device_ptr=4096, out_offset=[9, 200, 700, 701, 40000])
        q, o, p, code, mem, ptr = stub.calls[0]
        assert (code, mem, ptr) == (0, _lib.MEM_DEVICE, 4096) and o.tolist() == [9, 200, 700, 701, 40000] and p.tolist() == [0.1, 0.9]
        # quantile_time(): one cube, [n_probs, rows, cols]; a scalar gives [rows, cols]
        stub.calls.clear()
        a = R.quantile_time([0.5, 0.9], 2, 7)
        assert a.shape == (2, 50, 60) and a.dtype == np.float64 and stub.calls[0][0].tolist() == [[2, 7, 0, 50, 0, 60]] and stub.calls[0][3] == 3
        a = R.quantile_time(0.5, window=(3, 10, 20, 60), method="nearest")
        assert a.shape == (7, 40) and stub.calls[1][0].tolist() == [[0, 10, 3, 10, 20, 60]] and stub.calls[1][2].tolist() == [0.5] and stub.calls[1][3] == 2
        a = R.quantile_time([0.5, 0.9, 1.0], 3, 3)  # no instants: nothing to read, no call
        assert len(stub.calls) == 2 and a.shape == (3, 50, 60) and a.dtype == np.float64 and np.isnan(a).all()
        a = R.quantile_time(0.5, window=(4, 4, 0, 60))  # no cells
        assert len(stub.calls) == 2 and a.shape == (0, 60)
        for bad in (dict(start=5, stop=4), dict(stop=11), dict(start=-1, stop=3), dict(window=(0, 51, 0, 60)), dict(window=(4, 3, 0, 60)),
                    dict(method="median"), dict(method=4)):
            with pytest.raises(ValueError):
                R.quantile_time(0.5, **bad)
        for bad in ([], np.nan, [0.5, np.nan], 1.5, [-0.1], np.linspace(0, 1, 17)):
            with pytest.raises(ValueError):
                R.quantile_time(bad)
            with pytest.raises(ValueError):
                R.quantile_time(bad, start=3, stop=3)
            with pytest.raises(ValueError):
                R.quantile_time_flat(cubes, bad)
        assert len(stub.calls) == 2
    finally:
        R._native = None


def loop(series, p, method):
    """One cell by a plain Python loop: sort, then the rank rule of the contract."""
    v = sorted((x for x in series if x == x), key=lambda x: (x, not math.copysign(1.0, x) < 0))
    n = len(v)
    if n == 0:
        return float("nan")
    h = float(n - 1) * float(p)
    j = int(math.floor(h))
    g = h - j
    j1 = min(j + 1, n - 1)
    if method == "lower":
        return v[j]
    if method == "higher":
        return v[j] if g == 0 else v[j1]
    if method == "nearest":
        return v[j] if g < 0.5 else v[j1] if g > 0.5 else (v[j] if j % 2 == 0 else v[j1])
    return v[j] if g == 0 else v[j] + (v[j1] - v[j]) * g  # (Python floats: every operation rounds on its own)


def cases():
    rng = np.random.default_rng(11)
    for T in (1, 2, 5, 20, 33):
        a = rng.integers(-40, 40, size=(T, 6, 7)).astype(np.float64) / 8
        a[rng.random(a.shape) < 0.2] = np.nan
        a[:, 0, 0] = np.nan                  # no value at all
        a[:, 0, 1] = 3.25                    # all equal
        a[1:, 0, 2] = np.nan                 # one value
        a[:, 0, 3] = np.where(np.arange(T) % 2 == 0, -0.0, 0.0)  # both zeros
        yield a
    yield rng.integers(-2 ** 62, 2 ** 62, size=(9, 4, 5))  # int64 beyond 2^53: widened first
    yield (rng.integers(-2 ** 20, 2 ** 20, size=(12, 4, 5)) / 2 ** 7).astype(np.float32)


def test_model_against_a_per_cell_loop():
    for a in cases():
        x = M.widen(a)
        for method in M.METHODS:
            got = M.quantile_time(a, PROBS + [0.37], method)
            assert got.shape == (6,) + a.shape[1:] and got.dtype == np.float64
            want = np.array([[[loop(x[:, r, c].tolist(), p, method) for c in range(a.shape[2])] for r in range(a.shape[1])] for p in PROBS + [0.37]])
            M.same_bits(got, want)
        if a.shape[0] > 1 and a.dtype == np.float64:
            assert np.isnan(M.quantile_time(a, [0.5])[0, 0, 0]) and M.quantile_time(a, [0.3], "nearest")[0, 0, 1] == 3.25
            z = M.quantile_time(a, [0, 1], "lower")[:, 0, 3]
            assert np.signbit(z[0]) and not np.signbit(z[1])  # -0.0 sorts before +0.0


def test_model_against_numpy_nanquantile():
    """LOWER and HIGHER at p in {0, 0.25, 0.5, 0.75, 1} over series of 4 k + 1 values, where (n - 1) p is exact: numpy's own."""
    rng = np.random.default_rng(12)
    for T in (1, 5, 21):
        a = rng.integers(-1000, 1000, size=(T, 8, 9)).astype(np.float64) / 16
        if T > 5:
            nan = np.zeros(a.shape, dtype=bool)
            nan[:4, :, 0] = nan[:8, :, 1] = True  # n = 17 and n = 13: still 4 k + 1
            a[nan] = np.nan
        for method in ("lower", "higher"):
            got = M.quantile_time(a, [0, 0.25, 0.5, 0.75, 1], method)
            want = np.nanquantile(a, [0, 0.25, 0.5, 0.75, 1], axis=0, method=method)
            M.same_bits(got, want)


def test_the_library_selection_against_the_model():
    """dcdf_quantile_select_host: the kernel's selection loop as the library ships it, on the host."""
    from dcdf_amd import _lib
    for a in cases():
        x = M.widen(a)
        for method in M.METHODS:
            for probs in (PROBS, [0.5], list(np.linspace(0, 1, 16))):
                got, passes = _lib.quantile_select_host(x, probs, method)
                M.same_bits(got, M.quantile_time(a, probs, method))
                assert passes.shape == a.shape[1:] and int(passes.max()) <= 22 * 2 * len(probs)
                assert (passes[np.isnan(x).all(0)] == 0).all()  # (nothing to select: the first pass alone)
    with pytest.raises(_lib.DcdfError):
        _lib.quantile_select_host(np.zeros((3, 2)), [1.5])
    with pytest.raises(_lib.DcdfError):
        _lib.quantile_select_host(np.zeros((3, 2)), [np.nan])
    with pytest.raises(_lib.DcdfError):
        _lib.quantile_select_host(np.zeros((3, 2)), list(np.linspace(0, 1, 17)))


def test_the_inputs_prove_something():
    """The rasters of the GPU tests (test_gpu_reduce_time.source at (20, 264, 264)): for each float kind some cell has a tie at a
    selected rank, some cell is NaN on some instants, some has one value and some none; and for p = 0.9 over 20 instants g is neither
    0 nor 0.5, so LINEAR interpolates, NEAREST rounds and HIGHER differs from LOWER."""
    import test_gpu_reduce_time as RT
    j, j1, g = M.ranks(np.array([20]), 0.9)
    assert (int(j[0]), int(j1[0])) == (17, 18) and g[0] not in (0.0, 0.5) and 0 < g[0] < 1
    for kind in ("i32", "i64", "f32", "f64"):
        a = RT.source(kind)
        assert a.shape == (20, 264, 264)
        v, n = M.sorted_values(a)
        full = n == 20
        assert full.any()
        for p in (0.1, 0.5, 0.9):
            jj, jj1, gg = M.ranks(np.maximum(n, 2), p)
            vj, vj1 = np.take_along_axis(v, jj[None], 0)[0], np.take_along_axis(v, jj1[None], 0)[0]
            tie, apart = full & (vj == vj1), full & (vj != vj1)
            print(kind, p, "ties at the rank", int(tie.sum()), "apart", int(apart.sum()))
            assert apart.any()
            if kind[0] == "f":
                assert tie.any()
        lo, hi = M.quantile_time(a, [0.9], "lower")[0], M.quantile_time(a, [0.9], "higher")[0]
        assert (lo[full] != hi[full]).any()
        if kind[0] == "f":
            print(kind, "n == 0:", int((n == 0).sum()), "n == 1:", int((n == 1).sum()), "0 < n < 20:", int(((n > 0) & (n < 20)).sum()))
            assert (n == 0).any() and (n == 1).any() and ((n > 1) & (n < 20)).any()
            assert n[17, 23] == 0 and n[200, 5] == 1 and n[258, 259] == 0 and n[260, 261] == 1  # (bulk chunks and the corner chunk)


def test_keys_selection_and_planner_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/sim/quantile_check.cpp over k2r_quantile.h and plan_quantile_time, host code only, with AddressSanitizer and UBSan."""
    exe = str(tmp_path / "quantile_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", exe, os.path.join(HERE, "sim", "quantile_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    got = dict(line.split()[1:3] for line in out.stdout.splitlines() if line.startswith("ok "))
    assert set(got) == {"keys", "ranks", "small", "random", "plan"}, out.stdout
    assert int(got["keys"]) > 40 and int(got["small"]) == sum(5 ** k for k in range(8)) and int(got["random"]) == 10000 and int(got["plan"]) > 1000
