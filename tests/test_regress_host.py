"""Regression over time without a GPU: the model (regress_model.py) against a per-cell loop and against exact rational arithmetic,
the exact properties the header states, dcdf_regress_host against the model bit for bit, and tests/sim/regress_check.cpp -- a
stand-alone program built with AddressSanitizer and UBSan -- for the header's step and finish with the state stored and loaded at
every cut of a series."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import regress_model as RM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def same(got, want):
    np.testing.assert_array_equal(RM.bits(got), RM.bits(want))


# ---- the model -------------------------------------------------------------------------------------------------------------------
def loop_cell(xs, es):
    """One cell, plain Python floats: the recurrence and the finish as the header writes them."""
    c, K, sy, syy, se, see, sey = 0, np.nan, 0.0, 0.0, 0.0, 0.0, 0.0
    for x, e in zip(xs, es):
        x, e = float(x), float(e)
        if x != x:
            continue
        if c == 0:
            K = x
        d = x - K
        sy = sy + d
        syy = syy + d * d
        se = se + e
        see = see + e * e
        sey = sey + e * d
        c += 1
    out = dict(count=float(c), slope=np.nan, intercept=np.nan, corr=np.nan)
    if c < 2:
        return out
    me, my = se / c, sy / c
    See, Syy, Sey = max(see - se * me, 0.0), max(syy - sy * my, 0.0), sey - se * my
    if not See > 0:
        return out
    out["slope"] = Sey / See
    out["intercept"] = (K + my) - out["slope"] * me
    if Syy > 0:
        out["corr"] = min(1.0, max(-1.0, Sey / float(np.sqrt(See * Syy))))
    return out


def test_model_against_a_per_cell_loop():
    rng = np.random.default_rng(11)
    a = rng.normal(size=(9, 3, 4)).astype(np.float32)
    a[rng.random(a.shape) < 0.3] = np.nan
    e = RM.shifted(rng.normal(size=9) * 3.0)
    labels = np.array([0, 2, RM.NONE, 0, 7, 2, 2, 0, RM.NONE])  # group 1 has no instant, group 3 neither; label 7 is in no group
    plain, grouped = RM.regress_time(a, e), RM.regress_time_groups(a, e, labels, 4)
    for r in range(3):
        for c in range(4):
            want = loop_cell(a[:, r, c], e)
            for name in RM.NAMES:
                same(plain[name][r, c], want[name])
            for g in range(4):
                want = loop_cell(a[labels == g, r, c], e[labels == g])
                for name in RM.NAMES:
                    same(grouped[name][g, r, c], want[name])
    assert (grouped["count"][1] == 0).all() and np.isnan(grouped["slope"][3]).all() and (grouped["count"][0] > 1).any()
    assert np.isfinite(plain["corr"]).any()
    one = RM.regress_time_groups(a, e, np.zeros(9, dtype=np.uint16), 1)
    for name in RM.NAMES:
        same(one[name][0], plain[name])
    assert e[0] == 0 and RM.shifted(None, 4).tolist() == [0, 1, 2, 3] and RM.shifted([5.5, 7.5]).tolist() == [0, 2] and RM.shifted(None, 0).size == 0


def families(rng, n):
    """(values in the leaves' dtypes, regressor with first value 0) of n instants"""
    i = np.arange(n, dtype=np.float64)
    enso = RM.shifted(np.cumsum(rng.normal(0.0, 0.4, n)))
    years = RM.shifted(1950.0 + i / 12.0)
    return {
        "float32 trend on the index": ((np.linspace(250.0, 310.0, n) + rng.normal(0.0, 0.05, n)).astype(np.float32), i),
        "int32 near 2^30 on the index": (((1 << 30) + rng.integers(-3, 4, n)).astype(np.int32), i),
        "noise on the index": (rng.normal(0.0, 1.0, n), i),
        "rain on an index series": (np.where(rng.random(n) < 0.8, 0.0, rng.gamma(0.7, 9.0, n)).astype(np.float32), enso),
        "a response to an index series": ((3.0 * enso + rng.normal(0.0, 0.3, n) + 280.0).astype(np.float32), enso),
        "int64 near 2^62 on years": (((1 << 62) + rng.integers(-(1 << 40), 1 << 40, n)).astype(np.int64), years),
        "a near-perfect line on years": (1e6 + 2.5 * years + rng.normal(0.0, 1e-6, n), years),
        "int32 extremes on the index": (np.where(rng.random(n) < 0.5, np.iinfo(np.int32).min, np.iinfo(np.int32).max).astype(np.int32), i),
    }


BOUND = 6.0  # times (n + 2)^2 2^-53: DESIGN.md section 4n derives it
SIZES = tuple(range(3, 41)) + (64, 100, 365)


def exact_fit(xs, es):
    """(See, Syy, Sey) of the pairs, as fractions"""
    n = len(xs)
    sx, se = sum(xs), sum(es)
    return sum(v * v for v in es) - se * se / n, sum(v * v for v in xs) - sx * sx / n, sum(p * q for p, q in zip(es, xs)) - se * sx / n


def test_definition_is_accurate_against_exact_arithmetic(capsys):
    """Against fractions.Fraction over the widened values and the regressor as passed, n = 3 .. 40, 64, 100, 365 valid pairs:
    |SLOPE - exact| sqrt(See / Syy) and |CORR - exact| are at most 6 (1 + rho)^2 (n + 2)^2 2^-53, rho = a / sqrt(See) with a the
    least |e| among the valid pairs.  The bound is derived: a value a of the regressor and the value 0 of the
    shifted values are samples, so the raw sums are at most (n + 1) (1 + rho)^2 and n + 1 times the centred ones, and the n-term
    sequential sums behind Sey, See and Syy each cost about 3 (n + 1)^2 2^-53 of sqrt(See Syy), See and Syy, times 1 + rho and
    (1 + rho)^2.  First every family with the regressor's first value 0 and no NaN (rho = 0: 6 (n + 2)^2 2^-53); then the same
    families with the values of the first one to three instants NaN, as a cell has them whose first instants hold no value -- there
    0 is no longer among the valid pairs' regressor values and rho says what that costs.  Prints the worst ratios to n^2 2^-53."""
    rng = np.random.default_rng(2026)
    worst = {(k, late): (0.0, None) for k in ("slope", "corr") for late in (False, True)}
    u53 = 2.0 ** -53
    for n in SIZES:
        for name, (a, e) in families(rng, n + 3).items():
            assert e[0] == 0
            for lead in (0, 1 + n % 3):  # the instants without a value at the start
                x = RM.widen(a)[:n + lead].copy()
                x[:lead] = np.nan
                ev = e[:n + lead]
                xs, es = [Fraction(float(v)) for v in x[lead:]], [Fraction(float(v)) for v in ev[lead:]]
                See, Syy, Sey = exact_fit(xs, es)
                if See == 0 or Syy == 0:
                    continue
                rho = float(min(abs(v) for v in es)) / float(np.sqrt(float(See)))
                assert lead or rho == 0
                got = RM.regress_time(x.reshape(n + lead, 1, 1), ev)
                assert got["count"][0, 0] == n
                scale = float(np.sqrt(float(See / Syy)))
                r_exact = float(Sey) / float(np.sqrt(float(See * Syy)))
                errs = dict(slope=float(abs(Fraction(float(got["slope"][0, 0])) - Sey / See)) * scale,
                            corr=abs(float(got["corr"][0, 0]) - r_exact))
                for k, err in errs.items():
                    # (scale, rho and r_exact are themselves rounded: a few 2^-53, far below the bound's slack over the derivation)
                    limit = BOUND * (1.0 + rho) ** 2 * (n + 2) ** 2 * u53
                    assert err <= limit, (name, n, lead, k, err / ((n + 2) ** 2 * u53), rho)
                    ratio = err / (n * n * u53)
                    if ratio > worst[k, lead > 0][0]:
                        worst[k, lead > 0] = (ratio, (name, n, round(rho, 2)))
                assert -1.0 <= got["corr"][0, 0] <= 1.0
    with capsys.disabled():
        for (k, late), w in worst.items():
            print("\nworst error of %s%s: %.3f * n^2 * 2^-53 at %r" % (k, ", first instants NaN" if late else "", w[0], w[1]))


def test_exact_properties_of_the_model():
    e = RM.shifted([3.0, 4.5, 4.0, 7.0, -2.0, 0.5, 9.0])
    for v, dt in ((0.1, np.float64), (-3.25, np.float32), (1 << 30, np.int32), (0, np.int64)):
        a = np.full((7, 1, 2), v, dtype=dt)
        got = RM.regress_time(a, e)  # a constant cell
        same(got["slope"], np.zeros((1, 2)))
        same(got["intercept"], RM.widen(a[0]))
        assert np.isnan(got["corr"]).all() and (got["count"] == 7).all()
    one = RM.regress_time(np.array([[[np.nan]], [[5.5]], [[np.nan]]]), [0.0, 1.0, 2.0])  # one valid instant
    assert one["count"][0, 0] == 1 and all(np.isnan(one[n][0, 0]) for n in ("slope", "intercept", "corr"))
    none = RM.regress_time(np.full((3, 1, 1), np.nan), [0.0, 1.0, 2.0])
    assert none["count"][0, 0] == 0 and all(np.isnan(none[n][0, 0]) for n in ("slope", "intercept", "corr"))
    for n in ("slope", "intercept", "corr"):
        same(none[n], [[np.nan]])  # the one quiet NaN
    rng = np.random.default_rng(4)
    a = rng.integers(-2000, 2000, size=(40, 5, 5)).astype(np.int32)
    flat = RM.regress_time(a, np.full(40, 2.5))  # all regressor values equal: See == 0
    assert (flat["count"] == 40).all() and all(np.isnan(flat[n]).all() for n in ("slope", "intercept", "corr"))
    u = RM.shifted(rng.normal(size=40))
    x, y = RM.regress_time(a, u), RM.regress_time(a + 1_000_000, u)  # a constant added to integer values
    same(x["slope"], y["slope"])
    same(x["corr"], y["corr"])
    assert np.isfinite(x["corr"]).all() and (RM.bits(x["intercept"]) != RM.bits(y["intercept"])).all()
    # CORR stays inside [-1, 1] on near-perfect lines, where the quotient alone leaves it
    i = np.arange(50, dtype=np.float64)
    lines = np.stack([s * i * k + rng.normal(0.0, 1e-9, 50) for s in (1.0, -1.0) for k in (1.0, 3.0, 0.1, 7.7)] +
                     [s * i * k for s in (1.0, -1.0) for k in (0.1, 1.0 / 3.0, 7.7, 1e-3)], axis=1).reshape(50, 1, 16)
    got = RM.regress_time(lines, i)
    assert (np.abs(got["corr"]) <= 1.0).all() and (np.abs(got["corr"]) > 1.0 - 1e-12).all()
    # the regressor enters as given: an offset index gives other bits than the same index less its first value
    b = (np.linspace(0.0, 9.0, 40)[:, None, None] + rng.normal(size=(40, 5, 5))).astype(np.float32)
    far, near = RM.regress_time(b, 20000.0 + np.arange(40)), RM.regress_time(b, RM.shifted(20000.0 + np.arange(40)))
    assert (RM.bits(far["slope"]) != RM.bits(near["slope"])).any()
    for n in RM.NAMES:
        same(near[n], RM.regress_time(b, np.arange(40.0))[n])


# ---- dcdf_regress_host ----------------------------------------------------------------------------------------------------------
def test_host_function_equals_the_model_at_every_cut():
    """Every series of up to 8 instants over {1e6 + 1e-3, -2.5, NaN} -- NaN at the first, the last and all instants among them --
    against a fixed regressor: the whole series in one call, one value per call, and cut in two at every place, the second call
    continuing the first's state."""
    from dcdf_amd import _lib
    lib = _lib.lib()
    values = np.array([1e6 + 1e-3, -2.5, np.nan])
    E = np.ascontiguousarray(np.array([0.0, 1.5, -2.25, 3.0, 1000.125, 5.5, -7.0, 0.3]))
    st, out = np.empty(7), np.empty(4)
    sp, op = C.c_void_p(st.ctypes.data), C.c_void_p(out.ctypes.data)
    for n in range(0, 9):
        codes = np.arange(3 ** n)
        X = np.ascontiguousarray(values[(codes[:, None] // 3 ** np.arange(n)[None, :]) % 3].reshape(len(codes), n))
        want_state = RM.state_of(X.T.reshape(n, len(codes), 1), E[:n])
        want = RM.finish(want_state)
        if n == 8:
            assert np.isnan(X[:, 0]).any() and np.isnan(X[:, -1]).any() and np.isnan(X).all(axis=1).any()
        for i in range(len(codes)):
            base = X.ctypes.data + i * n * 8
            for cut in [(0, n)] + [(0, k) for k in range(1, n)] + [None]:
                st[:] = RM.INIT
                if cut is None:  # one value per call
                    for k in range(n):
                        assert lib.dcdf_regress_host(C.c_void_p(base + 8 * k), C.c_void_p(E.ctypes.data + 8 * k), 1, sp, None) == 0
                else:
                    assert lib.dcdf_regress_host(C.c_void_p(base), C.c_void_p(E.ctypes.data), cut[1], sp, None) == 0
                    assert lib.dcdf_regress_host(C.c_void_p(base + 8 * cut[1]), C.c_void_p(E.ctypes.data + 8 * cut[1]), n - cut[1], sp, op) == 0
                    same(out, [want[name][i, 0] for name in RM.NAMES])
                same(st, [w[i, 0] for w in want_state])
                assert lib.dcdf_regress_host(None, None, 0, sp, op) == 0
                same(out, [want[name][i, 0] for name in RM.NAMES])
    s, o = _lib.regress_host([3.0, np.nan, 5.0, 4.0], [0.0, 1.0, 2.0, 4.0])
    assert s.tolist() == [3.0, 3.0, 3.0, 5.0, 6.0, 20.0, 8.0] and o.tolist() == [3.0, 0.25, 3.5, 0.5]
    s2, o2 = _lib.regress_host([5.0, 4.0], [2.0, 4.0], state=_lib.regress_host([3.0, np.nan], [0.0, 1.0], finish=False)[0])
    same(s2, s)
    same(o2, o)
    x = np.zeros(2)
    xp = C.c_void_p(x.ctypes.data)
    assert lib.dcdf_regress_host(xp, xp, 2, None, op) == -1    # NULL state: DCDF_ERR_BAD_ARG
    assert lib.dcdf_regress_host(None, xp, 2, sp, op) == -1    # NULL series with instants
    assert lib.dcdf_regress_host(xp, None, 2, sp, op) == -1    # NULL regressor with instants
    for bad in (np.nan, np.inf, -np.inf):
        e = np.array([1.0, bad])
        st[:] = RM.INIT
        assert lib.dcdf_regress_host(xp, C.c_void_p(e.ctypes.data), 2, sp, op) == -1
        same(st, RM.INIT)  # refused before the state is touched
        assert lib.dcdf_regress_host(xp, C.c_void_p(e.ctypes.data), 1, sp, op) == 0  # (the bad value is not among those read)


# ---- the declarations and the wrappers --------------------------------------------------------------------------------------------
def test_symbols_declared_and_listed():
    from dcdf_amd import _lib
    text = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    assert "enum { DCDF_REGRESS_COUNT = 1, DCDF_REGRESS_SLOPE = 2, DCDF_REGRESS_INTERCEPT = 4, DCDF_REGRESS_CORR = 8 };" in text
    assert "int dcdf_regress_host(const double* x, const double* e, size_t n, double state[7], double out[4]);" in text
    assert "accuracy needs a regressor near zero" in text
    assert "dcdf_regress_host" in _lib.SYMBOLS and _lib.lib().dcdf_regress_host
    assert _lib.REGRESS_OPS == RM.BITS and list(_lib.REGRESS_OPS) == list(RM.NAMES)
    assert _lib.lib().dcdf_abi_version() == 3
    with pytest.raises(ValueError, match="regress_host"):
        _lib.regress_host([1.0, 2.0], [0.0])
    with pytest.raises(ValueError, match="regress_host"):
        _lib.regress_host([1.0], [0.0], state=np.zeros(4))
    with pytest.raises(_lib.DcdfError):
        _lib.regress_host([1.0, 2.0], [0.0, np.inf])


# ---- the stand-alone program ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("regress") / "regress_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", path, os.path.join(HERE, "sim", "regress_check.cpp")])
    return path


def test_step_store_load_and_finish_equal_the_model_at_every_cut(exe):
    """Every series up to 8 instants over three kinds of value, NaN among them, at every cut into consecutive pieces -- the sum
    over len of 3^len * 2^(len - 1) cases --, the state stored and loaded whole between the pieces."""
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert out.stdout.split()[:2] == ["ok", "cuts"] and int(out.stdout.split()[2]) == 1 + sum(3 ** n * 2 ** (n - 1) for n in range(1, 9))
