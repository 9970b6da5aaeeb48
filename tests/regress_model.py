"""The NumPy model of the regression over time (include/dcdf_k2r.h, dcdf_regress_host): per cell the
state (c, K, sy, syy, se, see, sey) starts as (0, NaN, +0.0, +0.0, +0.0, +0.0, +0.0); in instant order every instant with a non-NaN
x and the regressor value e does  if c == 0: K = x;  d = x - K;  sy = sy + d;  syy = syy + d * d;  se = se + e;  see = see + e * e;
sey = sey + e * d;  c = c + 1  (each one float64 operation); then n = c, me = se / n, my = sy / n, See = max(see - se * me, +0.0),
Syy = max(syy - sy * my, +0.0), Sey = sey - se * my, COUNT = c, SLOPE = Sey / See when c >= 2 and See > 0 else NaN, INTERCEPT =
(K + my) - SLOPE * me, CORR = clamp(Sey / sqrt(See * Syy), -1, 1) when additionally Syy > 0 else NaN.  Vectorised over the cells, a
loop over the instants.  A group is the plain model over the group's instants in order, each with its own regressor value.  The
contract takes the regressor as given; `shifted` is what a caller with a far-off regressor passes: u - u[0], u its regressor or the
instant index."""
import numpy as np

NONE = 0xffff
NAMES = ("count", "slope", "intercept", "corr")
BITS = dict(count=1, slope=2, intercept=4, corr=8)
INIT = (0.0, np.nan, 0.0, 0.0, 0.0, 0.0, 0.0)


def names_of(mask):
    return [n for n in NAMES if mask & BITS[n]]


def widen(a):
    """x[t] of an array in a leaf's own dtype: float64 (integers beyond 2^53 round, as reduce_widen's cast does)."""
    return np.asarray(a).astype(np.float64)


def shifted(u, nt=None):
    """The regressor u of nt instants less its first value, one float64 subtraction each; None is the instant index."""
    u = np.arange(nt, dtype=np.float64) if u is None else np.asarray(u, dtype=np.float64)
    return u - u[0] if u.size else u


def init(shape):
    return [np.full(shape, v) for v in INIT]


def step(state, x, e):
    """One instant x (float64, the state's shape) with the regressor value e (a float) into state, in place."""
    c, K, sy, syy, se, see, sey = state
    e = np.float64(e)
    ok = ~np.isnan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        K[...] = np.where(ok & (c == 0), x, K)
        d = x - K
        pd = d * d
        pe = e * e
        ped = e * d
        sy[...] = np.where(ok, sy + d, sy)
        syy[...] = np.where(ok, syy + pd, syy)
        se[...] = np.where(ok, se + e, se)
        see[...] = np.where(ok, see + pe, see)
        sey[...] = np.where(ok, sey + ped, sey)
        c[...] = np.where(ok, c + 1.0, c)
    return state


def finish(state):
    c, K, sy, syy, se, see, sey = state
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        me, my = se / c, sy / c
        See = see - se * me
        See = np.where(See < 0, 0.0, See)
        Syy = syy - sy * my
        Syy = np.where(Syy < 0, 0.0, Syy)
        Sey = sey - se * my
        fit = (c >= 2) & (See > 0)
        slope = np.where(fit, Sey / See, np.nan)
        icpt = np.where(fit, (K + my) - slope * me, np.nan)
        r = Sey / np.sqrt(See * Syy)
        r = np.where(r > 1, 1.0, r)
        r = np.where(r < -1, -1.0, r)
        corr = np.where(fit & (Syy > 0), r, np.nan)
    nan = lambda v: np.where(np.isnan(v), np.nan, v)  # (the one quiet NaN)
    return dict(count=c.copy(), slope=nan(slope), intercept=nan(icpt), corr=nan(corr))


def state_of(a, e, state=None):
    x = widen(a)
    e = np.asarray(e, dtype=np.float64)
    assert e.shape == (x.shape[0],)
    state = init(x.shape[1:]) if state is None else state
    for t in range(x.shape[0]):
        step(state, x[t], e[t])
    return state


def regress_time(a, e):
    """{name: float64 [rows, cols]} of a = [instants, rows, cols] in the leaves' own dtype against e = [instants], as given."""
    return finish(state_of(a, e))


def regress_time_groups(a, e, labels, n_groups):
    """{name: float64 [n_groups, rows, cols]}; labels = [instants], a label >= n_groups is in no group."""
    labels, e = np.asarray(labels), np.asarray(e, dtype=np.float64)
    assert labels.shape == (a.shape[0],)
    out = {n: np.empty((n_groups,) + a.shape[1:], dtype=np.float64) for n in NAMES}
    for g in range(n_groups):
        x = regress_time(a[labels == g], e[labels == g])
        for n in NAMES:
            out[n][g] = x[n]
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
