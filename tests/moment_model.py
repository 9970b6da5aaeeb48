"""The NumPy model of the moments over time (dcdf_raster_moments_time_batch, dcdf_raster_moments_time_groups_batch): per cell the
state (c, K, s1, s2) starts as (0, NaN, +0.0, +0.0); in instant order every non-NaN x does  if c == 0: K = x;  d = x - K;
s1 = s1 + d;  s2 = s2 + d * d;  c = c + 1  (each one float64 operation); then COUNT = c, m = s1 / c, MEAN = K + m,
q = max(s2 - s1 * m, +0.0), VAR = q / (c - ddof) when c > ddof else NaN, STD = sqrt(VAR).  Vectorised over the cells, a loop over
the instants.  A group is the plain model over the group's instants in order."""
import numpy as np

NONE = 0xffff
NAMES = ("count", "mean", "var", "std")
BITS = dict(count=1, mean=2, var=4, std=8)


def names_of(mask):
    return [n for n in NAMES if mask & BITS[n]]


def widen(a):
    """x[t] of an array in a leaf's own dtype: float64 (integers beyond 2^53 round, as reduce_widen's cast does)."""
    return np.asarray(a).astype(np.float64)


def init(shape):
    return [np.zeros(shape), np.full(shape, np.nan), np.zeros(shape), np.zeros(shape)]


def step(state, x):
    """One instant x (float64, the state's shape) into state = [c, K, s1, s2], in place."""
    c, K, s1, s2 = state
    ok = ~np.isnan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        K[...] = np.where(ok & (c == 0), x, K)
        d = x - K
        p = d * d
        s1[...] = np.where(ok, s1 + d, s1)
        s2[...] = np.where(ok, s2 + p, s2)
        c[...] = np.where(ok, c + 1.0, c)
    return state


def finish(state, ddof=0):
    c, K, s1, s2 = state
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = s1 / c
        mean = np.where(c > 0, K + m, np.nan)
        p = s1 * m
        q = s2 - p
        q = np.where(q < 0, 0.0, q)
        var = np.where(c > ddof, q / (c - ddof), np.nan)
        std = np.where(c > ddof, np.sqrt(var), np.nan)
    return dict(count=c.copy(), mean=mean, var=var, std=std)


def state_of(a, state=None):
    x = widen(a)
    state = init(x.shape[1:]) if state is None else state
    for t in range(x.shape[0]):
        step(state, x[t])
    return state


def moments_time(a, ddof=0):
    """{name: float64 [rows, cols]} of a = [instants, rows, cols] in the leaves' own dtype."""
    return finish(state_of(a), ddof)


def moments_time_groups(a, labels, n_groups, ddof=0):
    """{name: float64 [n_groups, rows, cols]}; labels = [instants], a label >= n_groups is in no group."""
    labels = np.asarray(labels)
    assert labels.shape == (a.shape[0],)
    out = {n: np.empty((n_groups,) + a.shape[1:], dtype=np.float64) for n in NAMES}
    for g in range(n_groups):
        x = moments_time(a[labels == g], ddof)
        for n in NAMES:
            out[n][g] = x[n]
    return out


def planes(flat, off, q, mask, rows, cols, n_groups=None):
    """Cube q of a moments_time_flat (n_groups None) or moments_time_groups_flat result as {name: planes} in plane order."""
    shape = (rows, cols) if n_groups is None else (n_groups, rows, cols)
    n = int(np.prod(shape))
    o = int(off[q])
    return {name: flat[o + i * n:o + (i + 1) * n].reshape(shape) for i, name in enumerate(names_of(mask))}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
