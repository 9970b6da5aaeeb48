"""The model of the rolling windows over time (dcdf_raster_rolling_time_batch, dcdf_raster_rolling_time_groups_batch; include/dcdf_k2r.h,
DESIGN.md section 4o), written apart from k2r_rolling.h: Python integers and nothing else.

Every decoded value is a multiple of 2^-63 with |x| <= 2^63, so int(math.ldexp(x, 63)) is exact.  Every window is summed again
from its own values (nothing slides here); the sums are compared as integers; the one rounding is Python's correctly rounded
int / int, the mean's division one float division.  A window belongs to the group of its last instant."""
import math

import numpy as np

NAMES = ("max", "argmax", "min", "argmin", "count")
BITS = dict(max=1, argmax=2, min=4, argmin=8, count=16)
NONE = 0xffff
ONE = 1 << 63


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def names_of(mask):
    return [n for n in NAMES if mask & BITS[n]]


def scaled(cube):
    """x * 2^63 of a decoded cube [nt, ...] as Python integers in an object array (0 where x is NaN), and where x is not NaN."""
    x = np.asarray(cube).astype(np.float64)
    ok = ~np.isnan(x)
    flat = np.empty(x.size, dtype=object)
    flat[:] = [int(math.ldexp(v, 63)) if v == v else 0 for v in x.ravel().tolist()]
    return flat.reshape(x.shape), ok


def window_sums(cube, w):
    """(S, c): S[k] the exact sum at the 2^-63 scale and c[k] the count of the non-NaN values of the window [k, k + w) -- the one
    that ends at instant k + w - 1 --, each summed from its own w values.  Shapes [max(nt - w + 1, 0), ...]."""
    X, ok = scaled(cube)
    n = max(X.shape[0] - w + 1, 0)
    S = np.empty((n,) + X.shape[1:], dtype=object)
    c = np.zeros((n,) + X.shape[1:], dtype=np.int64)
    for k in range(n):
        acc = X[k]
        for u in range(k + 1, k + w):
            acc = acc + X[u]
        S[k] = acc
        c[k] = ok[k:k + w].sum(axis=0)
    return S, c


def fold(S, c, w, min_count=None, mean=False, labels=None, n_groups=1):
    """{name: float64 [n_groups, ...]} from window_sums' (S, c): per group the extremes over the valid windows whose last instant
    carries its label (labels None: every instant 0), the earliest on equal integers."""
    min_count = w if min_count is None else min_count
    assert 1 <= min_count <= w and (not mean or min_count == w)
    cell = S.shape[1:]
    out = {n: np.full((n_groups,) + cell, 0.0 if n == "count" else np.nan) for n in NAMES}
    for g in range(n_groups):
        have = np.zeros(cell, dtype=bool)
        mx = np.zeros(cell, dtype=object)
        mn = np.zeros(cell, dtype=object)
        amx, amn, cnt = np.zeros(cell), np.zeros(cell), np.zeros(cell)
        for k in range(S.shape[0]):
            i = k + w - 1
            if (0 if labels is None else int(labels[i])) != g:
                continue
            ok = c[k] >= min_count
            up = ok & (~have | (S[k] > mx).astype(bool))
            dn = ok & (~have | (S[k] < mn).astype(bool))
            mx, mn = np.where(up, S[k], mx), np.where(dn, S[k], mn)
            amx, amn = np.where(up, float(i), amx), np.where(dn, float(i), amn)
            have |= ok
            cnt += ok
        hi = np.array([m / ONE for m in mx.ravel().tolist()], dtype=np.float64).reshape(cell)  # correctly rounded, 0 -> +0.0
        lo = np.array([m / ONE for m in mn.ravel().tolist()], dtype=np.float64).reshape(cell)
        if mean:
            hi, lo = hi / float(w), lo / float(w)
        out["max"][g] = np.where(have, hi, np.nan)
        out["min"][g] = np.where(have, lo, np.nan)
        out["argmax"][g] = np.where(have, amx, np.nan)
        out["argmin"][g] = np.where(have, amn, np.nan)
        out["count"][g] = cnt
    return out


def rolling_time_groups(cube, w, labels, n_groups, min_count=None, mean=False):
    """{name: float64 [n_groups, rows, cols]} of a decoded cube [nt, rows, cols]"""
    S, c = window_sums(cube, w)
    return fold(S, c, w, min_count, mean, labels, n_groups)


def rolling_time(cube, w, min_count=None, mean=False):
    """{name: float64 [rows, cols]}"""
    return {n: v[0] for n, v in rolling_time_groups(cube, w, None, 1, min_count, mean).items()}
