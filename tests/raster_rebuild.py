"""A raster rebuilt from leaf_grid's records alone -- TEST INFRASTRUCTURE ONLY.  Stored Superchunk trees (whoever wrote them:
the oracle or the library) are flattened by dcdf_amd.dataset.leaf_grid; chunk leaves are read with the oracle's
Chunk.fill_window at (row0, col0), elided leaves with from_fixed of their values."""
import numpy as np

import oracle_lib as O
from dcdf_amd.dataset import leaf_grid


def typed(values, bits, dtype):
    v = np.asarray(values, dtype=np.int64)
    if np.dtype(dtype).kind != "f":
        return v.astype(dtype)
    out = ((v - 1) / float(1 << (bits + 1))).astype(dtype)
    out[v == 0] = np.nan
    return out


def rebuild_from(store, cids, a, levels, chunk_size, round_):
    """The array of a's shape and dtype rebuilt from the records of `store` (cid -> object) under the segment roots `cids`, plus
    the records (with their raster positions) for further checks."""
    leaf, grid = leaf_grid(store, cids, levels, round_)
    assert leaf == 1 << levels[-1]
    T, R, C = a.shape
    nti, ntj = -(-R // leaf), -(-C // leaf)
    out = np.zeros_like(a)
    recs = []
    opened = {}
    assert len(grid) == -(-T // chunk_size)
    for s, g in enumerate(grid):
        assert len(g) == nti * ntj
        t0 = s * chunk_size
        nt = min(chunk_size, T - t0)
        for i, lf in enumerate(g):
            r0, c0 = (i // ntj) * leaf, (i % ntj) * leaf
            h, w = min(leaf, R - r0), min(leaf, C - c0)
            assert lf.minmax.shape == (nt, 2)
            if lf.cid is None:
                assert lf.values.shape == (nt,)
                out[t0:t0 + nt, r0:r0 + h, c0:c0 + w] = typed(lf.values, lf.fractional_bits, a.dtype)[:, None, None]
            else:
                ch = opened.setdefault(lf.cid, O.Chunk(bytes(store[lf.cid][8:])))
                out[t0:t0 + nt, r0:r0 + h, c0:c0 + w] = ch.fill_window(0, nt, lf.row0, lf.row0 + h, lf.col0, lf.col0 + w, dtype=a.dtype)
            recs.append((s, t0, nt, r0, c0, h, w, lf, store[lf.cid] if lf.cid else None))
    return out, recs
