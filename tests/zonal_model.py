"""The model of dcdf_raster_zonal_batch, for the tests: zone z of a label raster is
space_model.reduce_space over the cells whose label is z -- the values widened to float64, NaNs dropped, per instant math.fsum,
np.fmin / np.fmax, the count and one division -- plus the contract's rule for signed zeros: where a zone holds both -0.0 and +0.0
at one instant, -0.0 is its minimum and +0.0 its maximum (fmin / fmax leave that open).  A zone without a non-NaN cell gets NaN,
NaN, +0.0, 0, NaN; every comparison can be on bits."""
import numpy as np

import reduce_model as M
import space_model as SM

NAMES, names_of = SM.NAMES, SM.names_of
NONE = 0xFFFF


def zonal(a, labels, n_zones):
    """a: [instants, rows, cols] in the leaves' dtype; labels: [rows, cols] unsigned, a cell is in zone labels[r, c] when that is
    < n_zones -> {name: [n_zones, instants] float64}."""
    T = a.shape[0]
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    cells = a.reshape(T, -1)
    order = np.argsort(lab, kind="stable")
    first = np.searchsorted(lab[order], np.arange(n_zones + 1))
    out = {n: np.empty((n_zones, T), dtype=np.float64) for n in NAMES}
    for z in range(n_zones):
        idx = order[first[z]:first[z + 1]]  # the cells with labels == z
        v = cells[:, idx]
        if idx.size == 1:  # a zone of one cell is that cell's series (the exact sum of one value is the value)
            x = M.widen(v)[:, 0]
            nan = np.isnan(x)
            one = {"min": np.where(nan, np.nan, x), "max": np.where(nan, np.nan, x), "sum": np.where(nan, 0.0, x),
                   "count": np.where(nan, 0.0, 1.0), "mean": np.where(nan, np.nan, x)}
        else:
            one = SM.reduce_space(v.reshape(T, idx.size, 1))
            x = M.widen(v)
            zero, neg = x == 0, np.signbit(x)
            has_neg0, has_pos0 = (zero & neg).any(1), (zero & ~neg).any(1)
            one["min"] = np.where((one["min"] == 0) & has_neg0, -0.0, np.where((one["min"] == 0) & ~has_neg0, 0.0, one["min"]))
            one["max"] = np.where((one["max"] == 0) & has_pos0, 0.0, np.where((one["max"] == 0) & ~has_pos0, -0.0, one["max"]))
        for n in NAMES:
            out[n][z] = one[n]
    return out


def matrices(flat, off, q, mask, n_zones, nt):
    """The matrices of cube q of a zonal_flat result as {name: [n_zones, nt]}; mask = the ops bitmask of the call."""
    ns = names_of(mask)
    p = flat[int(off[q]):int(off[q]) + len(ns) * n_zones * nt].reshape(len(ns), n_zones, nt)
    return dict(zip(ns, p))
