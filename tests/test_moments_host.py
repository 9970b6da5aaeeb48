"""Moments over time without a GPU: the model (moment_model.py) against a per-cell loop and against exact rational arithmetic, the
exact properties the header states, dcdf_moments_host against the model bit for bit, the Python wrappers' argument checks, and
tests/sim/moment_check.cpp -- a stand-alone program built with AddressSanitizer and UBSan -- for the header's step, store / load
and finish at every cut, and for the planner's records of a one-group and a 300-group plan."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from dcdf_amd import dataset
from dcdf_amd.raster import EncodedRaster

import moment_model as MM
import test_raster_plan_host as PH
import test_reduce_time_groups_host as GH

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def same(got, want):
    np.testing.assert_array_equal(MM.bits(got), MM.bits(want))


# ---- the model -------------------------------------------------------------------------------------------------------------------
def loop_cell(xs, ddof):
    """One cell, plain Python floats: the recurrence as the header writes it."""
    c, K, s1, s2 = 0, np.nan, 0.0, 0.0
    for x in xs:
        x = float(x)
        if x != x:
            continue
        if c == 0:
            K = x
        d = x - K
        s1 = s1 + d
        s2 = s2 + d * d
        c += 1
    if c == 0:
        return dict(count=0.0, mean=np.nan, var=np.nan, std=np.nan)
    m = s1 / c
    q = s2 - s1 * m
    q = 0.0 if q < 0 else q
    var = q / (c - ddof) if c > ddof else np.nan
    return dict(count=float(c), mean=K + m, var=var, std=float(np.sqrt(var)))


def test_model_against_a_per_cell_loop():
    rng = np.random.default_rng(11)
    a = rng.normal(size=(9, 3, 4)).astype(np.float32)
    a[rng.random(a.shape) < 0.3] = np.nan
    labels = np.array([0, 2, MM.NONE, 0, 7, 2, 2, 0, MM.NONE])  # group 1 has no instant, group 3 neither; label 7 is in no group
    for ddof in (0, 1):
        plain, grouped = MM.moments_time(a, ddof), MM.moments_time_groups(a, labels, 4, ddof)
        for r in range(3):
            for c in range(4):
                want = loop_cell(a[:, r, c], ddof)
                for name in MM.NAMES:
                    same(plain[name][r, c], want[name])
                for g in range(4):
                    want = loop_cell(a[labels == g, r, c], ddof)
                    for name in MM.NAMES:
                        same(grouped[name][g, r, c], want[name])
        assert (grouped["count"][1] == 0).all() and np.isnan(grouped["var"][3]).all() and (grouped["count"][0] > 0).any()
    one = MM.moments_time_groups(a, np.zeros(9, dtype=np.uint16), 1)
    for name in MM.NAMES:
        same(one[name][0], MM.moments_time(a)[name])


def families(rng, n):
    """Eight families of series of n instants, in the leaves' dtypes."""
    rain = np.where(rng.random(n) < 0.8, 0.0, rng.gamma(0.7, 9.0, n)).astype(np.float32)
    t0 = np.float32(287.15)
    ulps = np.frombuffer((np.array([t0]).view(np.uint32) + rng.integers(0, 6, n).astype(np.uint32)).tobytes(), dtype=np.float32)
    ext = np.where(rng.random(n) < 0.5, np.iinfo(np.int32).min, np.iinfo(np.int32).max).astype(np.int32)
    return {
        "int32 near 2^30": ((1 << 30) + rng.integers(-3, 4, n)).astype(np.int32),
        "1e6 then noise": np.concatenate([[1e6], rng.normal(0.0, 1e-3, n - 1)]),
        "rain": rain,
        "int64 near 2^62": ((1 << 62) + rng.integers(-(1 << 40), 1 << 40, n)).astype(np.int64),
        "float32 ulps apart": ulps,
        "int32 extremes": ext,
        "uniform": rng.random(n),
        "trend": (np.linspace(250.0, 310.0, n) + rng.normal(0.0, 0.05, n)).astype(np.float32),
    }


def test_definition_is_accurate_against_exact_arithmetic(capsys):
    """The relative error of VAR against fractions.Fraction over the widened values is at most 4 (n + 2)^2 2^-53: the derived order,
    about six times the worst the recurrence showed (0.67 n^2 2^-53).  Prints the worst ratio to n^2 2^-53 it meets."""
    rng = np.random.default_rng(2026)
    worst = (0.0, None)
    for n in (2, 3, 8, 33, 100, 365):
        for name, a in families(rng, n).items():
            x = MM.widen(a)
            xs = [Fraction(float(v)) for v in x]
            s, ss = sum(xs), sum(v * v for v in xs)
            for ddof in (0, 1):
                got = MM.moments_time(a.reshape(n, 1, 1), ddof)
                var = float(got["var"][0, 0])
                exact = (ss - s * s / n) / (n - ddof)
                if exact == 0:
                    assert var == 0.0, (name, n, ddof)
                    continue
                rel = float(abs(Fraction(var) - exact) / exact)
                assert rel <= 4.0 * (n + 2) ** 2 * 2.0 ** -53, (name, n, ddof, rel / ((n + 2) ** 2 * 2.0 ** -53))
                ratio = rel / (n * n * 2.0 ** -53)
                if ratio > worst[0]:
                    worst = (ratio, (name, n, ddof))
                mean_err = float(abs(Fraction(float(got["mean"][0, 0])) - s / n))
                assert mean_err <= (n + 2) * 2.0 ** -52 * float(max(abs(v) for v in xs)), (name, n)
    with capsys.disabled():
        print("\nworst relative error of VAR: %.3f * n^2 * 2^-53 at %r" % worst)


def test_exact_properties_of_the_model():
    for v, dt in ((0.1, np.float64), (-3.25, np.float32), (1 << 30, np.int32), (0, np.int64)):
        a = np.full((7, 1, 2), v, dtype=dt)
        got = MM.moments_time(a, 1)
        same(got["var"], np.zeros((1, 2)))
        same(got["std"], np.zeros((1, 2)))
        same(got["mean"], MM.widen(a[0]))
    one = MM.moments_time(np.array([[[5.5]]]), 1)
    assert one["count"][0, 0] == 1 and one["mean"][0, 0] == 5.5 and np.isnan(one["var"][0, 0]) and np.isnan(one["std"][0, 0])
    assert MM.moments_time(np.array([[[5.5]]]), 0)["var"][0, 0] == 0.0
    none = MM.moments_time(np.full((3, 1, 1), np.nan))
    assert none["count"][0, 0] == 0 and all(np.isnan(none[n][0, 0]) for n in ("mean", "var", "std"))
    rng = np.random.default_rng(4)
    a = rng.integers(-2000, 2000, size=(40, 5, 5)).astype(np.int32)
    for ddof in (0, 1):
        x, y = MM.moments_time(a, ddof), MM.moments_time(a + 1_000_000, ddof)
        same(x["var"], y["var"])
        same(x["std"], y["std"])
    # near 2^30 the unshifted sums of squares lose the differences: the same input on the GPU proves the shift is there
    b = shift_source()
    x = MM.widen(b)
    s = ss = np.zeros(b.shape[1:])
    for t in range(len(x)):
        s, ss = s + x[t], ss + x[t] * x[t]
    unshifted = (ss - s * (s / len(x))) / len(x)
    assert (MM.bits(unshifted) != MM.bits(MM.moments_time(b)["var"])).any()


def shift_source(base=1 << 30, shape=(24, 64, 64)):
    """int32 values base - 3 .. base + 3 (tests/test_gpu_moments.py stores the same raster)."""
    return (base + np.random.default_rng(30).integers(-3, 4, size=shape)).astype(np.int32)


# ---- dcdf_moments_host ----------------------------------------------------------------------------------------------------------
def test_host_function_equals_the_model_at_every_cut():
    """Every series of up to 8 instants over {1e6 + 1e-3, -2.5, NaN}: the whole series in one call, one value per call, and cut in
    two at every place, the second call continuing the first's state; both ddof."""
    from dcdf_amd import _lib
    lib = _lib.lib()
    values = np.array([1e6 + 1e-3, -2.5, np.nan])
    st, out = np.empty(4), np.empty(4)
    sp, op = C.c_void_p(st.ctypes.data), C.c_void_p(out.ctypes.data)
    for n in range(0, 9):
        codes = np.arange(3 ** n)
        X = np.ascontiguousarray(values[(codes[:, None] // 3 ** np.arange(n)[None, :]) % 3].reshape(len(codes), n))
        want_state = MM.state_of(X.T.reshape(n, len(codes), 1))
        want = [MM.finish(want_state, ddof) for ddof in (0, 1)]
        for i in range(len(codes)):
            base = X.ctypes.data + i * n * 8
            cuts = [(0, n)] + [(0, k) for k in range(1, n)] + [None]
            for cut in cuts:
                st[:] = [0.0, np.nan, 0.0, 0.0]
                if cut is None:  # one value per call
                    for k in range(n):
                        assert lib.dcdf_moments_host(C.c_void_p(base + 8 * k), 1, 0, sp, None) == 0
                else:
                    assert lib.dcdf_moments_host(C.c_void_p(base), cut[1], 0, sp, None) == 0
                    assert lib.dcdf_moments_host(C.c_void_p(base + 8 * cut[1]), n - cut[1], 1, sp, op) == 0
                    same(out, [want[1][name][i, 0] for name in MM.NAMES])
                same(st, [w[i, 0] for w in want_state])
                assert lib.dcdf_moments_host(None, 0, 0, sp, op) == 0
                same(out, [want[0][name][i, 0] for name in MM.NAMES])
    s, o = _lib.moments_host([3.0, np.nan, 5.0], ddof=1)
    assert s.tolist() == [2.0, 3.0, 2.0, 4.0] and o.tolist() == [2.0, 4.0, 2.0, np.sqrt(2.0)]
    s2, o2 = _lib.moments_host([5.0], ddof=1, state=_lib.moments_host([3.0, np.nan], finish=False)[0])
    same(s2, s)
    same(o2, o)
    x = np.zeros(2)
    xp = C.c_void_p(x.ctypes.data)
    assert lib.dcdf_moments_host(xp, 2, 2, sp, op) == -1      # ddof above 1: DCDF_ERR_BAD_ARG
    assert lib.dcdf_moments_host(xp, 2, 0, None, op) == -1    # NULL state
    assert lib.dcdf_moments_host(None, 2, 0, sp, op) == -1    # NULL series with instants


# ---- the declarations and the wrappers --------------------------------------------------------------------------------------------
def test_symbols_declared_and_listed():
    from dcdf_amd import _lib
    text = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    assert "enum { DCDF_MOMENT_COUNT = 1, DCDF_MOMENT_MEAN = 2, DCDF_MOMENT_VAR = 4, DCDF_MOMENT_STD = 8 };" in text
    assert "int dcdf_raster_moments_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t ddof, double* out," in text
    assert "int dcdf_raster_moments_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t ddof," in text
    assert "int dcdf_moments_host(const double* x, size_t n, uint32_t ddof, double state[4], double out[4]);" in text
    for s in ("dcdf_raster_moments_time_batch", "dcdf_raster_moments_time_groups_batch", "dcdf_moments_host"):
        assert s in _lib.SYMBOLS and getattr(_lib.lib(), s)
    assert _lib.MOMENT_OPS == MM.BITS and list(_lib.MOMENT_OPS) == list(MM.NAMES)
    assert _lib.lib().dcdf_abi_version() == 3


class FakeRaster(EncodedRaster):
    """EncodedRaster's wrappers over a _region_call that answers from the model: what they pass down and how they shape the result."""

    def __init__(self, a):
        self.a, self.shape, self.calls, self._native = a, a.shape, [], None

    def _region_call(self, name, q, counts, dtype, args, zeroed=False, stats=True, out_device_ptr=None, out_offset=None):
        own = args(len(q), None, 0, None, None)
        assert dtype == np.float64 and name in ("moments_time", "moments_time_groups") and len(own) == (7 if name == "moments_time" else 10)
        mask, ddof = own[1].value, own[2].value
        grouped = name == "moments_time_groups"
        assert own[-4:] == (None, 0, None, None) and own[0] == len(q)
        if grouped:
            l_ptr, l_off, n_groups = own[3], own[4], own[5].value
            loff = np.ctypeslib.as_array(C.cast(l_off, C.POINTER(C.c_uint64)), (len(q),))
        vol = counts()
        flat, off = [], np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64)
        for i, c in enumerate(q.astype(int)):
            t0, t1, r0, r1, c0, c1 = PH.norm(c)
            sub = self.a[t0:t1, r0:r1, c0:c1]
            if grouped:
                lab = np.ctypeslib.as_array(C.cast(l_ptr.value + 2 * int(loff[i]), C.POINTER(C.c_uint16)), (max(1, t1 - t0),))[:t1 - t0]
                self.calls.append((name, mask, ddof, n_groups, lab.copy()))
                x = MM.moments_time_groups(sub, lab, n_groups, ddof) if vol[i] else None
            else:
                self.calls.append((name, mask, ddof))
                x = MM.moments_time(sub, ddof) if vol[i] else None
            if vol[i]:
                flat += [x[n].ravel() for n in MM.names_of(mask)]
        return np.concatenate(flat + [np.zeros(1)]), off, 0.0, np.zeros(3, dtype=np.uint64)


def test_wrappers_lay_out_planes_and_refuse_bad_arguments():
    a = np.random.default_rng(5).integers(-9, 9, size=(7, 4, 5)).astype(np.int32)
    R = FakeRaster(a)
    got = R.moments_time()
    assert list(got) == ["mean", "std"] and R.calls[-1] == ("moments_time", 10, 0)
    want = MM.moments_time(a)
    for n in got:
        same(got[n], want[n])
    got = R.moments_time(("std", "count", "var"), 2, 6, window=(1, 3, 0, 5), ddof=1)
    assert list(got) == ["count", "var", "std"] and R.calls[-1] == ("moments_time", 13, 1) and got["var"].shape == (2, 5)
    want = MM.moments_time(a[2:6, 1:3], 1)
    for n in got:
        same(got[n], want[n])
    assert list(R.moments_time(15)) == list(MM.NAMES) and list(R.moments_time("var")) == ["var"]
    flat, off, _, _ = R.moments_time_flat([[0, 7, 0, 4, 0, 5], [5, 1, 3, 0, 4, 2], [3, 3, 0, 4, 0, 5]], ("mean", "var"), ddof=1)
    assert off.tolist() == [0, 2 * 20, 2 * 20 + 2 * 6]  # the cube without instants writes nothing
    same(MM.planes(flat, off, 1, 6, 3, 2)["var"], MM.moments_time(a[1:5, 0:3, 2:4], 1)["var"])
    # the grouped form: n_groups defaults to the largest label present, NONE apart, plus 1
    lab = np.array([1, 0, MM.NONE, 1, 3, 0, 1], dtype=np.uint16)
    got = R.moments_time_groups(("std", "mean"), lab, ddof=1)
    assert list(got) == ["mean", "std"] and got["std"].shape == (4, 4, 5) and R.calls[-1][:4] == ("moments_time_groups", 10, 1, 4)
    want = MM.moments_time_groups(a, lab, 4, 1)
    for n in got:
        same(got[n], want[n])
    got = R.moments_time_groups("var", lab[2:6], 2, 6, window=(1, 3, 0, 5), n_groups=2)
    same(got["var"], MM.moments_time_groups(a[2:6, 1:3], lab[2:6], 2)["var"])
    flat, off, _, _ = R.moments_time_groups_flat([[0, 7, 0, 4, 0, 5], [5, 1, 3, 0, 4, 2]], 15, [lab, lab[1:5]], 3)
    assert off.tolist() == [0, 4 * 3 * 20] and R.calls[-1][4].tolist() == lab[1:5].tolist()
    same(MM.planes(flat, off, 1, 15, 3, 2, 3)["std"], MM.moments_time_groups(a[1:5, 0:3, 2:4], lab[1:5], 3)["std"])
    # the empty cases: count 0, NaN elsewhere, nothing is called
    n_calls = len(R.calls)
    none = R.moments_time(("count", "std"), 3, 3)
    assert none["count"].shape == (4, 5) and (none["count"] == 0).all() and np.isnan(none["std"]).all()
    assert R.moments_time("mean", window=(2, 2, 0, 5))["mean"].shape == (0, 5)
    none = R.moments_time_groups(("count", "var"), np.zeros(0, dtype=np.uint16), 3, 3)
    assert none["count"].shape == (1, 4, 5) and (none["count"] == 0).all() and np.isnan(none["var"]).all()
    assert R.moments_time_groups("mean", lab, window=(2, 2, 0, 5), n_groups=6)["mean"].shape == (6, 0, 5)
    assert len(R.calls) == n_calls
    assert R.moments_time_groups("mean", np.full(7, MM.NONE, dtype=np.uint16))["mean"].shape == (1, 4, 5)
    # every ValueError; the messages name moments_time and its own statistics
    for ops in (0, 16, 31, "median", ("mean", "sum"), "min"):
        with pytest.raises(ValueError, match="moments_time: .*count, mean, var, std"):
            R.moments_time(ops)
        with pytest.raises(ValueError, match="moments_time"):
            R.moments_time_groups(ops, lab)
        with pytest.raises(ValueError, match="moments_time"):
            R.moments_time_flat([[0, 7, 0, 4, 0, 5]], ops)
    for ddof in (2, -1, 0.5, None):
        with pytest.raises(ValueError, match="moments_time: ddof"):
            R.moments_time("var", ddof=ddof)
        with pytest.raises(ValueError, match="moments_time: ddof"):
            R.moments_time_groups_flat([[0, 7, 0, 4, 0, 5]], 4, [lab], 4, ddof=ddof)
    with pytest.raises(ValueError):
        R.moments_time("var", 5, 3)
    with pytest.raises(ValueError):
        R.moments_time("var", window=(0, 5, 0, 5))
    for bad, kw in ((lab.astype(np.int32), {}), (lab[:6], {}), (lab, dict(n_groups=0)), (lab, dict(n_groups=65536)), (lab.reshape(7, 1), {})):
        with pytest.raises(ValueError, match="moments_time_groups"):
            R.moments_time_groups("var", bad, **kw)
    for labels, ng in (([lab.astype(np.int64)], 2), ([lab[:3]], 2), ([lab, lab], 2), ([lab], 0), ([lab], 65536)):
        with pytest.raises(ValueError, match="moments_time_groups"):
            R.moments_time_groups_flat([[0, 7, 0, 4, 0, 5]], 1, labels, ng)


def test_variable_maps_ids_and_handles_the_empty_cases():
    class FakeVar(dataset.Variable):
        def __init__(self, a):
            self.a, self.R = a, FakeRaster(a)

        def _region(self, start, stop, top, bottom, left, right):
            T, Rr, Cc = self.a.shape
            return (T if stop is None else stop), (Rr if bottom is None else bottom), (Cc if right is None else right)

        def raster(self):
            return self.R

    a = np.random.default_rng(8).integers(-9, 9, size=(8, 3, 4)).astype(np.int32)
    v = FakeVar(a)
    got = v.moments_time()
    assert list(got) == ["mean", "std"]
    same(got["std"], MM.moments_time(a)["std"])
    got = v.moments_time(("var",), 1, 7, 1, 3, 0, 2, ddof=1)
    same(got["var"], MM.moments_time(a[1:7, 1:3, 0:2], 1)["var"])
    none = v.moments_time(("count", "mean"), 4, 4)
    assert (none["count"] == 0).all() and none["count"].shape == (3, 4) and np.isnan(none["mean"]).all()
    ids_in = np.array([12, -1, 3, 12, 700000, 3, -5, 12])
    ids, got = v.moments_time_groups(ids_in, ("var", "count"), ddof=1)
    assert ids.tolist() == [3, 12, 700000] and list(got) == ["count", "var"] and got["var"].shape == (3, 3, 4)
    for i, g in enumerate(ids):
        want = MM.moments_time(a[ids_in == g], 1)
        same(got["var"][i], want["var"])
        same(got["count"][i], want["count"])
    assert v.R.calls[-1][2:4] == (1, 3) and v.R.calls[-1][4].tolist() == [1, MM.NONE, 0, 1, 2, 0, MM.NONE, 1]
    assert list(v.moments_time_groups(ids_in)[1]) == ["mean", "std"]
    n_calls = len(v.R.calls)
    ids, got = v.moments_time_groups(np.full(8, -1), ("count",))
    assert ids.size == 0 and got["count"].shape == (0, 3, 4)
    ids, got = v.moments_time_groups(np.zeros(0, dtype=np.int64), ("std",), 4, 4)
    assert ids.size == 0 and got["std"].shape == (0, 3, 4) and len(v.R.calls) == n_calls
    for bad in (ids_in.astype(np.float64), ids_in[:7], ids_in.reshape(8, 1)):
        with pytest.raises(ValueError, match="moments_time_groups"):
            v.moments_time_groups(bad)
    with pytest.raises(ValueError, match="moments_time: ddof"):
        v.moments_time_groups(ids_in, ddof=2)
    with pytest.raises(ValueError, match="moments_time"):
        v.moments_time("sum")
    big = FakeVar(np.zeros((65536, 1, 1), dtype=np.int32))
    with pytest.raises(ValueError, match="65536 distinct"):
        big.moments_time_groups(np.arange(65536))


# ---- the stand-alone program ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("moment") / "moment_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", path, os.path.join(HERE, "sim", "moment_check.cpp")])
    return path


def test_step_store_load_and_finish_equal_the_model_at_every_cut(exe):
    """Every label series up to 8 instants over {0, 1, 2, NONE} at every cut into consecutive pieces -- the sum over len of
    4^len * 2^(len - 1) cases --, and the label-less form at every cut with every set of statistics."""
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    full = 1 + sum(4 ** n * 2 ** (n - 1) for n in range(1, 9))
    assert out.stdout.split()[:2] == ["ok", "cuts"] and int(out.stdout.split()[2]) == full + 15 * (1 + sum(2 ** (n - 1) for n in range(1, 9)))


@pytest.mark.parametrize("n_groups", [1, 300])
def test_plan_records_of_the_moments(exe, tmp_path, n_groups):
    """The plan the two entry points make -- plan_reduce_time_groups, for the plain call with one group --, painted as
    tests/test_raster_plan_host.py paints reduce_time's: plain rasters and a tiled one; with 300 groups the tiled one, at both
    walk steps and slab caps."""
    rasters = ((PH.plain("bulk"), [1, 19, 33, 99, 63, 193]), (PH.plain("checker"), [1, 19, 33, 99, 63, 193]), (PH.tiled(), [1, 19, 5, 39, 20, 90]))
    for G, inner in rasters[2 if n_groups > 1 else 0:]:
        cases = GH.matrix(G, inner, n_groups)
        cases = cases if n_groups == 1 else [cases[0], cases[3]]
        for (G_, B, step, slab), g in zip(cases, GH.run(exe, tmp_path, cases)):
            GH.check_groups(G_, B, g, slab, step)
