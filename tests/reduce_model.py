"""The NumPy model of dcdf_raster_reduce_time_batch, for the tests: the native-dtype values widened to
float64, then per cell fmin / fmax over the non-NaN values, the SEQUENTIAL sum in instant order (one IEEE addition per instant),
the count of non-NaN values and sum / count.  Where nothing is counted min, max and mean are the one quiet NaN NumPy's `nan` is
(the contract says "NaN"; a fixed bit pattern lets every comparison be on bits)."""
import numpy as np

NAMES = ("min", "max", "sum", "count", "mean")
BIT = {"min": 1, "max": 2, "sum": 4, "count": 8, "mean": 16}


def widen(a):
    """x[t]: int -> float64 round-to-nearest (exact below 2^53), float32 -> float64 exactly."""
    return np.asarray(a).astype(np.float64)


def sequential_sum(x, valid):
    s = np.zeros(x.shape[1:], dtype=np.float64)
    for t in range(x.shape[0]):
        s = np.where(valid[t], s + x[t], s)
    return s


def reduce_time(a):
    """a: [instants >= 1, rows, cols] in the leaves' dtype -> {name: [rows, cols] float64}."""
    x = widen(a)
    valid = ~np.isnan(x)
    cnt = valid.sum(0).astype(np.float64)
    s = sequential_sum(x, valid)
    with np.errstate(all="ignore"):
        mean = np.where(cnt > 0, s / cnt, np.nan)
        mn = np.where(cnt > 0, np.fmin.reduce(x, axis=0), np.nan)
        mx = np.where(cnt > 0, np.fmax.reduce(x, axis=0), np.nan)
    return {"min": mn, "max": mx, "sum": s, "count": cnt, "mean": mean}


def names_of(mask):
    return [n for n in NAMES if mask & BIT[n]]


def planes(flat, off, q, mask, rows, cols):
    """The planes of cube q of a reduce_time_flat result as {name: [rows, cols]}."""
    ns = names_of(mask)
    p = flat[int(off[q]):int(off[q]) + len(ns) * rows * cols].reshape(len(ns), rows, cols)
    return dict(zip(ns, p))
