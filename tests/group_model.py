"""The NumPy model of the grouped reduce over time (dcdf_raster_reduce_time_groups_batch): per group g, reduce_model.reduce_time of
the sub-series a[labels == g]; a group without an instant gets the none values NaN, NaN, +0.0, 0, NaN."""
import numpy as np

import reduce_model as M

NONE = 0xffff
NAMES = M.NAMES


def none_planes(rows, cols):
    return {n: np.full((rows, cols), 0.0 if n in ("sum", "count") else np.nan) for n in NAMES}


def reduce_time_groups(a, labels, n_groups):
    """{name: float64 [n_groups, rows, cols]} of a = [instants, rows, cols] in the leaves' own dtype and labels = [instants]."""
    labels = np.asarray(labels)
    assert labels.shape == (a.shape[0],)
    out = {n: np.empty((n_groups,) + a.shape[1:], dtype=np.float64) for n in NAMES}
    for g in range(n_groups):
        sub = a[labels == g]
        x = M.reduce_time(sub) if len(sub) else none_planes(*a.shape[1:])
        for n in NAMES:
            out[n][g] = x[n]
    return out


def planes(flat, off, q, mask, n_groups, rows, cols):
    """Cube q of a reduce_time_groups_flat result as {name: [n_groups, rows, cols]} in plane order."""
    names = M.names_of(mask)
    n = n_groups * rows * cols
    o = int(off[q])
    return {name: flat[o + i * n:o + (i + 1) * n].reshape(n_groups, rows, cols) for i, name in enumerate(names)}
