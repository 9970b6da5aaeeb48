"""The NumPy model of dcdf_raster_quantile_time_batch, for the tests: the native-dtype values widened to
float64, per cell sorted with NaN last (-0.0 before +0.0: the sort is on order-preserving integer keys), then the rank rule of the
contract: h = (n - 1) * p in float64, j = floor(h), g = h - j, j1 = min(j + 1, n - 1); "linear" is three separate float64
operations.  Where a cell has no value the result is the one quiet NaN NumPy's `nan` is; comparisons are on bits, NaN equal to
NaN."""
import numpy as np

METHODS = {"lower": 0, "higher": 1, "nearest": 2, "linear": 3}
TOP = np.uint64(1) << np.uint64(63)
LAST = np.uint64(0xffffffffffffffff)


def widen(a):
    """x[t]: int -> float64 round-to-nearest (exact below 2^53), float32 -> float64 exactly."""
    return np.asarray(a).astype(np.float64)


def key(x):
    """Order-preserving uint64 keys of float64 (not NaN): unsigned order = numeric order, -0.0 below +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | TOP)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~TOP, ~k).view(np.float64)


def sorted_values(a):
    """(v, n): v [instants, ...] float64 ascending along axis 0 with NaN last, n [...] the number of values that are not NaN."""
    x = widen(a)
    nan = np.isnan(x)
    k = key(x)
    k[nan] = LAST
    k.sort(axis=0)
    n = (~nan).sum(0)
    v = unkey(k)
    v[np.arange(x.shape[0]).reshape((-1,) + (1,) * (x.ndim - 1)) >= n] = np.nan
    return v, n


def ranks(n, p):
    """(j, j1, g) of the contract for counts n >= 1 (int array) and one probability."""
    h = (n - 1).astype(np.float64) * np.float64(p)
    fl = np.floor(h)
    j = fl.astype(np.int64)
    return j, np.minimum(j + 1, n - 1), h - fl


def from_sorted(v, n, probs, method="linear"):
    """The quantiles of sorted_values' (v, n): [n_probs, ...] float64 (one sort serves every method and probability)."""
    some = n > 0
    n1 = np.maximum(n, 1)
    out = []
    for p in np.asarray(probs, dtype=np.float64).reshape(-1):
        j, j1, g = ranks(n1, p)
        vj, vj1 = np.take_along_axis(v, j[None], 0)[0], np.take_along_axis(v, j1[None], 0)[0]
        if method == "lower":
            r = vj
        elif method == "higher":
            r = np.where(g == 0, vj, vj1)
        elif method == "nearest":
            r = np.where(g < 0.5, vj, np.where(g > 0.5, vj1, np.where(j % 2 == 0, vj, vj1)))
        else:
            with np.errstate(all="ignore"):
                d = vj1 - vj
                m = d * g
                r = np.where(g == 0, vj, vj + m)
        out.append(np.where(some, r, np.nan))
    return np.stack(out)


def quantile_time(a, probs, method="linear"):
    """a: [instants >= 1, rows, cols] in the leaves' dtype -> [n_probs, rows, cols] float64."""
    return from_sorted(*sorted_values(a), probs, method)


def same_bits(got, want):
    """float64 arrays equal bit for bit, NaN equal to NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float64 and want.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~both_nan
    assert not bad.any(), "%d of %d differ, first at %r: %r != %r" % (bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def planes(flat, off, q, n_probs, rows, cols):
    """The planes of cube q of a quantile_time_flat result as [n_probs, rows, cols]."""
    return flat[int(off[q]):int(off[q]) + n_probs * rows * cols].reshape(n_probs, rows, cols)
