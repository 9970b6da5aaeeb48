"""dcdf_value_bounds: real-valued search bounds -> the stored integers that match, checked on the host (no GPU) against a numpy
brute force of the predicate value search is defined by: lower <= v <= upper, v = what the typed fill_window returns for the
stored n (from_fixed in float32 / float64, NaN for n = 0; n itself for integer chunks)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dcdf_amd import _lib as L  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
INF = float("inf")


def divisor(bits):
    """from_fixed's divisor (int64_t)1 << (bits + 1) (fixed.rs:84): wrapped to -2^63 at 62 fractional bits."""
    d = 1 << (bits + 1)
    return d - (1 << 64) if d >= 1 << 63 else d


def value(enc, bits, n):
    """The typed value of stored n, as store_typed computes it (None for the NaN code)."""
    if enc == L.DCDF_F32:
        return None if n == 0 else float(np.float32(np.int64(n - 1)) / np.float32(divisor(bits)))
    if enc == L.DCDF_F64:
        return None if n == 0 else float(np.float64(np.int64(n - 1)) / np.float64(divisor(bits)))
    return n  # (a Python int: compared with a float exactly)


def matches(enc, bits, n, lower, upper):
    v = value(enc, bits, n)
    return v is not None and lower <= v <= upper


def domain(enc):
    if enc == L.DCDF_I32:
        return I32_MIN, I32_MAX
    if enc == L.DCDF_I64:
        return I64_MIN, I64_MAX
    return I64_MIN + 1, I64_MAX  # (from_fixed of INT64_MIN overflows; to_fixed never stores it)


def first(enc, bits, pred):
    """Smallest n of the domain with pred(w(n)) for a monotone pred, by bisection over Python ints (None: there is none).
    w(n) = v(n), the typed value, where that is non-decreasing in n; -v(n) at 62 fractional bits, where the divisor is negative."""
    lo, hi = domain(enc)
    sign = -1.0 if divisor(bits) < 0 else 1.0
    f = (lambda n: pred(n)) if enc in (L.DCDF_I32, L.DCDF_I64) else (lambda n: pred(sign * value(enc, bits, n if n != 0 else 1)))
    if not f(hi):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if f(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def reference(enc, bits, lower, upper):
    """(lo, hi, hole) or None when nothing matches, from the predicate alone."""
    lower, upper = min(lower, upper), max(lower, upper)
    if enc in (L.DCDF_F32, L.DCDF_F64) and divisor(bits) < 0:  # lower <= v <= upper  <=>  -upper <= -v <= -lower
        lower, upper = -upper, -lower
    dlo, dhi = domain(enc)
    # -inf is unbounded: every stored integer, INT64_MIN included (which to_fixed never produces)
    nlo = (I32_MIN if enc == L.DCDF_I32 else I64_MIN) if lower == -INF else first(enc, bits, lambda v: v >= lower)
    if nlo is None:
        return None
    if upper == INF:
        nhi = dhi
    else:
        above = first(enc, bits, lambda v: v > upper)
        if above == dlo:  # every value lies above upper (no stored value is infinite)
            return None
        nhi = dhi if above is None else above - 1
    if enc in (L.DCDF_F32, L.DCDF_F64) and nlo <= 0 <= nhi:
        if nlo == nhi == 0:
            return None
        if nlo == 0:
            nlo = 1
        elif nhi == 0:
            nhi = -1
        else:
            return nlo, nhi, True
    return (nlo, nhi, False) if nlo <= nhi else None


def check(enc, bits, lower, upper):
    lo, hi, hole = L.value_bounds(enc, bits, lower, upper)
    want = reference(enc, bits, lower, upper)
    if want is None:
        assert lo > hi and not hole, (enc, bits, lower, upper, lo, hi)
        return
    assert (lo, hi, hole) == want, (enc, bits, lower, upper)
    a, b = min(lower, upper), max(lower, upper)
    dlo, dhi = domain(enc)
    # the ends match, the integers just outside them do not (stepping over the NaN code, which never matches)
    assert (lo == I64_MIN or matches(enc, bits, lo, a, b)) and matches(enc, bits, hi, a, b)
    below, above = lo - 1, hi + 1
    if below == 0 and enc in (L.DCDF_F32, L.DCDF_F64):
        below = -1
    if above == 0 and enc in (L.DCDF_F32, L.DCDF_F64):
        above = 1
    if below >= dlo:
        assert not matches(enc, bits, below, a, b)
    if above <= dhi:
        assert not matches(enc, bits, above, a, b)
    if hole:
        assert lo < 0 < hi and not matches(enc, bits, 0, a, b)
        assert matches(enc, bits, -1, a, b) and matches(enc, bits, 1, a, b)


FLOATS = [(L.DCDF_F32, b) for b in (0, 1, 2, 8, 16, 29, 34, 62)] + [(L.DCDF_F64, b) for b in (0, 1, 2, 8, 16, 29, 34, 52, 61, 62)]


def representable(enc, bits):
    """Bounds that are exactly values of some stored n, and their nextafter neighbours."""
    out = []
    for n in (1, 2, 3, -1, -5, 1000, -(1 << 20), (1 << 24) + 1, (1 << 24) + 3, (1 << 40) + 12345, -(1 << 40) - 7,
              (1 << 61) + 1, -(1 << 61) + 1, (1 << 62) + 12345):
        v = value(enc, bits, n)
        out += [v, math.nextafter(v, INF), math.nextafter(v, -INF)]
    return out


@pytest.mark.parametrize("enc,bits", FLOATS)
def test_float_bounds_at_representable_values_and_neighbours(enc, bits):
    vals = representable(enc, bits)
    for i, x in enumerate(vals):
        check(enc, bits, x, x)  # a point range: exactly the n whose value is x (or nothing)
        for y in vals[i + 1:i + 6]:
            check(enc, bits, x, y)


@pytest.mark.parametrize("enc,bits", FLOATS)
def test_float_zero_infinities_reversed_and_the_hole(enc, bits):
    for lo, hi in [(0.0, 0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 1.0), (-1.0, -0.0), (-INF, INF), (-INF, 0.0), (0.0, INF),
                   (INF, INF), (-INF, -INF), (1.0, -1.0), (-2.5, 3.25), (5.0, 3.0), (1e-30, 2e-30), (-1e300, 1e300)]:
        check(enc, bits, lo, hi)
    # a range that straddles the NaN code's neighbourhood sets the hole; one on either side does not
    lo, hi, hole = L.value_bounds(enc, bits, -1.0, 1.0)
    assert hole and lo < 0 < hi
    # (value 0 is stored 1: a range that ends at 0 on the side of the stored integers above it has no hole -- the positive
    # values, except at 62 bits, where the negative divisor puts the negative values there)
    for a, b in [(0.0, 1.0) if divisor(bits) > 0 else (-1.0, 0.0), (-1.0, -0.5), (0.5, 1.0)]:
        assert not L.value_bounds(enc, bits, a, b)[2]
    assert L.value_bounds(enc, bits, 2.0, 1.0) == L.value_bounds(enc, bits, 1.0, 2.0)


@pytest.mark.parametrize("enc,bits", FLOATS)
def test_float_empty_ranges(enc, bits):
    step = 2.0 ** -(bits + 1)
    for lo, hi in [(0.25 * step, 0.75 * step), (-0.75 * step, -0.25 * step), (1e30, 1e31) if enc == L.DCDF_F32 else (1e300, INF),
                   (INF, INF), (-INF, -INF)]:
        a, b, hole = L.value_bounds(enc, bits, lo, hi)
        want = reference(enc, bits, lo, hi)
        check(enc, bits, lo, hi)
        if want is None:
            assert a > b and not hole


def test_float32_collapses_many_stored_integers_into_one_value():
    # at 29 bits every float32 value above ~0.016 stands for many stored n: the closed form ceil(lower * 2^30) + 1 is wrong
    bits = 29
    for x in (0.02, 1.0, 10.0, 20.0, 123.456):
        lo, hi, _ = L.value_bounds(L.DCDF_F32, bits, x, x)
        closed = math.ceil(x * 2.0 ** (bits + 1)) + 1
        if lo <= hi:
            assert hi > lo  # a whole run of n shares the value
        check(L.DCDF_F32, bits, x, x)
        check(L.DCDF_F32, bits, 10.0, x)
        assert reference(L.DCDF_F32, bits, x, INF)[0] != closed or value(L.DCDF_F32, bits, closed - 1) < x


def test_brute_force_small_bits():
    # every n in a window around the bounds, directly against the predicate
    for enc, bits in [(L.DCDF_F32, 0), (L.DCDF_F32, 2), (L.DCDF_F64, 1), (L.DCDF_I32, 0), (L.DCDF_I64, 0)]:
        for lower, upper in [(-3.3, 4.1), (0.0, 2.0), (-2.0, 0.0), (1.0, 1.0), (-0.1, 0.1), (2.6, 2.4), (7.0, 7.0)]:
            lo, hi, hole = L.value_bounds(enc, bits, lower, upper)
            a, b = min(lower, upper), max(lower, upper)
            for n in range(-64, 65):
                got = lo <= n <= hi and not (hole and n == 0)
                assert got == matches(enc, bits, n, a, b), (enc, bits, lower, upper, n)


@pytest.mark.parametrize("enc,bits", [(L.DCDF_F32, 62), (L.DCDF_F64, 62), (L.DCDF_F64, 61)])
def test_brute_force_top_bits(enc, bits):
    """61 and 62 fractional bits: every stored n of windows around 0, around the stored integers of +-0.25 and +-0.5 and at
    both ends of int64, directly against the predicate.  At 62 bits the decoder's divisor is -2^63 (the reference's too), so
    the value falls as n rises: stored -2^61 + 1 decodes to +0.25."""
    assert divisor(61) == 1 << 62 and divisor(62) == -(1 << 63)
    if bits == 62:
        assert value(enc, bits, -(1 << 61) + 1) == 0.25 and value(enc, bits, (1 << 62) + 1) == -0.5
    q = 1 << (bits - 1)  # |n - 1| of a value of magnitude 0.25
    centres = [0, q, -q, 2 * q, -2 * q, I64_MAX - 70, I64_MIN + 71]
    step = 2.0 ** -(bits + 1)
    for lower, upper in [(0.1, 0.5), (-0.5, -0.1), (0.25, 0.25), (-0.25, 0.25), (-3 * step, 5 * step), (0.0, 0.0), (0.5, 0.25),
                         (-INF, 0.25), (-0.25, INF), (-INF, INF), (-40 * step, -2 * step), (0.9999, 2.0), (-2.0, -0.9999)]:
        lo, hi, hole = L.value_bounds(enc, bits, lower, upper)
        a, b = min(lower, upper), max(lower, upper)
        hits = 0
        for c in centres:
            for n in range(max(c - 70, I64_MIN + 1), min(c + 70, I64_MAX) + 1):
                got = lo <= n <= hi and not (hole and n == 0)
                assert got == matches(enc, bits, n, a, b), (enc, bits, lower, upper, n)
                hits += got
        if (lower, upper) in [(0.1, 0.5), (-0.5, -0.1), (0.25, 0.25)]:
            assert hits > 0 and lo <= hi  # the range the 62-bit search used to report as empty


@pytest.mark.parametrize("enc", [L.DCDF_I32, L.DCDF_I64])
def test_integer_bounds(enc):
    cases = [(1.5, 2.5), (-1.5, 1.5), (0.0, 0.0), (-0.0, 0.0), (2.0, 2.0), (2.1, 2.9), (3.0, -3.0), (-INF, INF), (-INF, 5.0), (5.0, INF),
             (INF, INF), (-INF, -INF), (2.0 ** 53 + 2, 2.0 ** 60), (-2.0 ** 62, -2.0 ** 54), (2.0 ** 63, 2.0 ** 64), (-2.0 ** 64, -2.0 ** 63),
             (-2.0 ** 63, -2.0 ** 63), (2.0 ** 31, 2.0 ** 40), (-2.0 ** 40, -2.0 ** 31 - 1), (-2.0 ** 40, 2.0 ** 40)]
    for lo, hi in cases:
        check(enc, 0, lo, hi)
        a, b, hole = L.value_bounds(enc, 0, lo, hi)
        assert not hole  # zero is an ordinary value of an integer chunk
    assert L.value_bounds(enc, 0, 0.0, 0.0)[:2] == (0, 0)
    assert L.value_bounds(enc, 0, 1.5, 2.5)[:2] == (2, 2)
    # beyond 2^53: the stored integer is never rounded to double
    big = 2.0 ** 60
    lo, hi, _ = L.value_bounds(L.DCDF_I64, 0, big, big)
    assert lo == hi == 1 << 60
    assert L.value_bounds(L.DCDF_I32, 0, -INF, INF)[:2] == (I32_MIN, I32_MAX)
    assert L.value_bounds(L.DCDF_I64, 0, -INF, INF)[:2] == (I64_MIN, I64_MAX)


def test_bad_arguments():
    nan = float("nan")
    for enc in (L.DCDF_I32, L.DCDF_I64, L.DCDF_F32, L.DCDF_F64):
        for lo, hi in [(nan, 1.0), (1.0, nan), (nan, nan)]:
            with pytest.raises(L.DcdfError) as e:
                L.value_bounds(enc, 0, lo, hi)
            assert e.value.code == -1  # DCDF_ERR_BAD_ARG
    for enc, bits in [(7, 0), (L.DCDF_F32, 63), (L.DCDF_F64, 200)]:
        with pytest.raises(L.DcdfError):
            L.value_bounds(enc, bits, 0.0, 1.0)
    # 62 bits is the most Chunk::build accepts; the divisor is -2^63 there, so [0, 1] is stored 1 (value 0) and everything below
    assert L.value_bounds(L.DCDF_F64, 61, 0.0, 1.0)[0] == 1
    assert L.value_bounds(L.DCDF_F64, 62, 0.0, 1.0) == (I64_MIN + 1, 1, True)
    assert L.value_bounds(L.DCDF_F64, 62, -1.0, 0.0)[0] == 1


def test_python_decode_mirrors_use_the_wrapped_divisor():
    """dataset._from_fixed / Variable._typed decode elided fills on the host: the same value as the device decode and the
    reference (the oracle's from_fixed), 62 fractional bits and its sign flip included."""
    import oracle_lib as O
    from dcdf_amd import dataset
    assert [dataset._fixed_divisor(b) for b in range(63)] == [float(divisor(b)) for b in range(63)]
    var = dataset.Variable.__new__(dataset.Variable)
    ns = [1, 2, -1, 9, -(1 << 61) + 1, (1 << 61) + 1, (1 << 62) + 1, -(1 << 62) + 1, 12345678901, I64_MAX, I64_MIN + 1]
    for bits in (0, 3, 52, 61, 62):
        for dtype, ftype in ((np.float64, "f64"), (np.float32, "f32")):
            var.encoding = dataset.MMEncoding.F64 if dtype is np.float64 else dataset.MMEncoding.F32
            assert var.dtype is dtype
            want = np.array([O.from_fixed(n, bits, ftype) for n in ns], dtype=dtype)
            got = np.array([dataset._from_fixed(n, bits, dtype) for n in ns], dtype=dtype)
            assert (got == want).all(), (bits, ftype)
            assert (var._typed(np.array(ns, dtype=np.int64), bits) == want).all(), (bits, ftype)
            assert np.isnan(dataset._from_fixed(0, bits, dtype)) and np.isnan(var._typed([0], bits)[0])
    assert dataset._from_fixed(-(1 << 61) + 1, 62, np.float64) == 0.25
