"""The model of dcdf_raster_reduce_space_batch, for the tests: the native-dtype values widened to float64
(reduce_model.widen), the mask applied and the NaNs dropped, then per instant math.fsum (the exact sum, rounded once), np.fmin /
np.fmax, the count and one division.  Where nothing is counted min, max and mean are the one quiet NaN NumPy's `nan` is -- the
patterns reduce_model uses -- so every comparison can be on bits."""
import math

import numpy as np

import reduce_model as M

NAMES, BIT, names_of = M.NAMES, M.BIT, M.names_of


def reduce_space(a, mask=None):
    """a: [instants, rows, cols] in the leaves' dtype; mask: [rows, cols], non-zero = selected (None: every cell)
    -> {name: [instants] float64}."""
    x = M.widen(a).reshape(a.shape[0], -1)
    if mask is not None:
        x = x[:, np.asarray(mask).reshape(-1) != 0]
    out = {n: np.empty(a.shape[0], dtype=np.float64) for n in NAMES}
    for t in range(a.shape[0]):
        v = x[t][~np.isnan(x[t])]
        s = math.fsum(v.tolist())
        out["sum"][t] = s
        out["count"][t] = float(v.size)
        out["min"][t] = np.fmin.reduce(v) if v.size else np.nan
        out["max"][t] = np.fmax.reduce(v) if v.size else np.nan
        out["mean"][t] = s / float(v.size) if v.size else np.nan
    return out


def series(flat, off, q, mask, nt):
    """The series of cube q of a reduce_space_flat result as {name: [nt]}; mask = the ops bitmask of the call."""
    ns = names_of(mask)
    p = flat[int(off[q]):int(off[q]) + len(ns) * nt].reshape(len(ns), nt)
    return dict(zip(ns, p))
