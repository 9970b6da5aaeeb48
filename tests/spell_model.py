"""The contract of dcdf_raster_spells_batch in NumPy: the fold over a boolean hit cube [T, rows, cols], and the hit rule over the
values decode returns.  Written per instant with whole-plane selects; tests/test_spells_host.py pins it against a per-cell loop."""
import math

import numpy as np

NAMES = ("count", "longest", "longest_start", "first", "last")
BIT = {"count": 1, "longest": 2, "longest_start": 4, "first": 8, "last": 16}
NONE = 0xffffffff


def names_of(mask):
    return [n for n in NAMES if mask & BIT[n]]


def hits(a, lower, upper):
    """Value search's rule on decoded values: integers compare exactly with [ceil(lower), floor(upper)]; floats are widened to
    float64 FIRST (a float32 array compared with a Python float would be compared in float32); NaN never hits.  Reversed bounds
    are swapped, +-inf is unbounded."""
    lower, upper = float(lower), float(upper)
    assert not (math.isnan(lower) or math.isnan(upper))
    if lower > upper:
        lower, upper = upper, lower
    a = np.asarray(a)
    if a.dtype.kind in "iu":
        if lower == math.inf or upper == -math.inf:
            return np.zeros(a.shape, dtype=bool)
        h = np.ones(a.shape, dtype=bool)
        if lower != -math.inf:
            lo = math.ceil(lower)  # (Python integers: exact)
            h &= (a >= lo) if lo <= np.iinfo(a.dtype).max else False
        if upper != math.inf:
            hi = math.floor(upper)
            h &= (a <= hi) if hi >= np.iinfo(a.dtype).min else False
        return h
    x = a.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (x >= lower) & (x <= upper)  # (False for NaN)


def spells(h):
    """{name: uint32 [rows, cols]} of a boolean cube h[T, rows, cols], instants counted from 0."""
    h = np.asarray(h, dtype=bool)
    shape = h.shape[1:]
    count, cur, longest = (np.zeros(shape, dtype=np.int64) for _ in range(3))
    lstart, first, last = (np.full(shape, NONE, dtype=np.int64) for _ in range(3))
    for i in range(h.shape[0]):
        hit = h[i]
        cur = np.where(hit, cur + 1, 0)
        count = count + hit
        up = cur > longest
        lstart = np.where(up, i + 1 - cur, lstart)
        longest = np.where(up, cur, longest)
        first = np.where(hit & (first == NONE), i, first)
        last = np.where(hit, i, last)
    out = dict(count=count, longest=longest, longest_start=lstart, first=first, last=last)
    return {n: v.astype(np.uint32) for n, v in out.items()}


def planes(flat, off, q, mask, rows, cols):
    """Cube q's planes of a spells_flat result as {name: [rows, cols]}."""
    names = names_of(mask)
    o = int(off[q])
    return {n: flat[o + i * rows * cols:o + (i + 1) * rows * cols].reshape(rows, cols) for i, n in enumerate(names)}
