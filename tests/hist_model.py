"""The model of dcdf_raster_histogram_batch, for the tests: the native-dtype values widened to float64, the
mask applied, NaN dropped, every value counted in the bin numpy.histogram would put it in for explicit edges -- edges[b] <= x <
edges[b + 1], the last bin closed on both sides -- and values outside the edges counted nowhere.  Counts are integers, so every
comparison with the device is exact."""
import numpy as np


def bin_index(edges, x):
    """The bin of every value of x (float64, no NaN), -1 where it lies outside the edges."""
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.size - 1
    idx = np.searchsorted(edges, x, side="right") - 1
    idx[x == edges[-1]] = bins - 1
    idx[(idx < 0) | (idx >= bins)] = -1
    return idx


def histogram(a, edges, mask=None):
    """a = [instants, rows, cols] of any dtype, mask = [rows, cols] (non-zero = selected) or None: uint64 [instants, bins]."""
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.size - 1
    a = np.asarray(a)
    out = np.zeros((a.shape[0], bins), dtype=np.uint64)
    sel = None if mask is None else (np.asarray(mask) != 0)
    for t in range(a.shape[0]):
        x = a[t].astype(np.float64)
        x = x.ravel() if sel is None else x[sel]
        x = x[~np.isnan(x)]
        idx = bin_index(edges, x)
        out[t] = np.bincount(idx[idx >= 0], minlength=bins).astype(np.uint64)
    return out


def cube(flat, offsets, q, instants, bins):
    """Cube q of a histogram_flat result as [instants, bins]."""
    o = int(offsets[q])
    return flat[o:o + instants * bins].reshape(instants, bins)
