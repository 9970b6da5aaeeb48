"""The case table of the fused encoder's tests: which strided views of a tile must take which kernel
k_encode<L, PADDED, VEC>, and tile contents named for the property they have.  Pure numpy: imports neither the GPU nor
the library, so the host tests (the simulator against the oracle) and the GPU tests (device views against the oracle)
walk the same table.

  views(L, dtype)       -> (name, (padded, loader), make(buffer) -> (byte_offset, strides, shape))
  contents(kind, ...)   -> (array, fractional_bits, round)
  error_tiles(L, dtype) -> (name, array, fractional_bits, round, code)
  classify(...)         -> (log2_sidelen, padded, loader): validate_tile's rule (k2r_session_plan.h) restated
"""
import zlib

import numpy as np

LEVELS = (4, 5, 6, 7, 8)
DTYPES = (np.int32, np.int64, np.float32, np.float64)
LOADER = {np.dtype(np.int32): 1, np.dtype(np.float32): 2, np.dtype(np.int64): 3, np.dtype(np.float64): 4}
VALUE_LIMIT = 1 << 30  # the fused kernel's contract: stored values in [-2^30, 2^30)


def instants(L):
    return 6 if L <= 6 else 4


def is_float(dtype):
    return np.dtype(dtype).kind == "f"


# ---- views ---------------------------------------------------------------------------------------------------------------

def classify(base_address, dtype, strides, shape):
    """validate_tile for k = 2 and sidelen 16..256: (log2_sidelen, padded, loader).  strides in elements."""
    esz = np.dtype(dtype).itemsize
    al = 16 // esz
    st, sr, sc = strides
    _, rows, cols = shape
    lg = 0
    while (1 << lg) < max(rows, cols):
        lg += 1
    assert 4 <= lg <= 8
    S = 1 << lg
    padded = rows != S or cols != S
    rows16 = (not padded and sc == 1 and sr % al == 0 and sr > 0 and st % al == 0 and base_address % 16 == 0
              and ((rows - 1) * sr + cols) * esz < (1 << 31))
    return lg, int(padded), LOADER[np.dtype(dtype)] if rows16 else 0


def extent(byte_offset, strides, shape, itemsize):
    """[first, last) byte a view touches, relative to its buffer's start."""
    lo = hi = byte_offset
    for s, n in zip(strides, shape):
        if s < 0:
            lo += s * (n - 1) * itemsize
        else:
            hi += s * (n - 1) * itemsize
    return lo, hi + itemsize


def buffer_elems(L, dtype):
    """Elements of backing store that hold any view of views(L, dtype)."""
    S, T = 1 << L, instants(L)
    return T * S * (2 * S + 16) + 64


def as_view(buffer, byte_offset, strides, shape):
    """The numpy view a make() result describes, inside `buffer` (1-D, of the view's dtype); bounds are checked."""
    esz = buffer.itemsize
    lo, hi = extent(byte_offset, strides, shape, esz)
    assert 0 <= lo and hi <= buffer.nbytes and byte_offset % esz == 0, (byte_offset, strides, shape, buffer.nbytes)
    return np.lib.stride_tricks.as_strided(buffer[byte_offset // esz:], shape=shape, strides=[s * esz for s in strides])


def views(L, dtype):
    """(name, (padded, loader), make) for sidelen S = 2^L.  make(buffer) -> (byte_offset, strides, shape) places the view in a
    1-D buffer of at least make.nbytes bytes whose start is 16-byte aligned; strides are in elements."""
    S, T = 1 << L, instants(L)
    esz = np.dtype(dtype).itemsize
    al = 16 // esz
    W = S + 3 * al          # a wider buffer's row: still a multiple of 16 bytes
    V = LOADER[np.dtype(dtype)]
    full = (T, S, S)

    def fixed(byte_offset, strides, shape):
        lo, hi = extent(byte_offset, strides, shape, esz)

        def make(buffer):
            assert buffer.ndim == 1 and buffer.dtype == np.dtype(dtype) and 0 <= lo and hi <= buffer.nbytes
            return byte_offset, tuple(strides), tuple(shape)
        make.nbytes = hi  # the bytes of buffer the view needs (buffer_elems(L, dtype) elements hold any of them)
        return make

    # the 16-byte row loader
    yield "dense", (0, V), fixed(0, (S * S, S, 1), full)
    yield "subtile", (0, V), fixed(48, (S * W, W, 1), full)
    # (instant stride 0 is a multiple of 16 bytes: one aligned instant read T times is still the row loader's; what the rule
    # sends to the generic loader is a row stride that is not positive: broadcast_rows, negative_rows below)
    yield "broadcast_instants", (0, V), fixed(0, (0, S, 1), full)
    # near misses: the generic loader
    yield "base_plus_1", (0, 0), fixed(esz, (S * S, S, 1), full)
    yield "row_stride_plus_1", (0, 0), fixed(0, (S * (S + 1), S + 1, 1), full)
    yield "instant_stride_plus_1", (0, 0), fixed(0, (S * S + 1, S, 1), full)
    yield "col_stride_2", (0, 0), fixed(0, (2 * S * S, 2 * S, 2), full)
    yield "transposed", (0, 0), fixed(0, (S * S, 1, S), full)
    yield "negative_rows", (0, 0), fixed((S - 1) * S * esz, (S * S, -S, 1), full)
    yield "broadcast_rows", (0, 0), fixed(0, (S, 0, 1), full)
    # padded tiles
    for rows, cols in ((S - 1, S), (S, S // 2 + 1), (S // 2 + 1, S // 2 + 1), (1, S)):
        yield "padded_%dx%d" % (rows, cols), (1, 0), fixed(0, (rows * cols, cols, 1), (T, rows, cols))
        yield "padded_%dx%d_subtile" % (rows, cols), (1, 0), fixed(48, (S * W, W, 1), (T, rows, cols))


# ---- contents ------------------------------------------------------------------------------------------------------------

INT_KINDS = ("small", "wide", "noise", "const", "sparse")
FLOAT_ONLY_KINDS = ("nan_blocks", "neg_fractions", "round_ties", "subnormal", "edge29", "edge29_over")
REROUTED_KINDS = ("edge29_over",)  # a stored value beyond the fused kernel's contract: the universal kernel encodes the tile


def kinds(dtype):
    return INT_KINDS + FLOAT_ONLY_KINDS if is_float(dtype) else INT_KINDS


def int_field(kind, shape, rng):
    """The five integer fields (int64): `small` one Dac byte, `wide` three and more with a Log-friendly second instant,
    `noise` every instant a Snapshot, `const` uniform instants, `sparse` a few cells changing per instant (Logs, with one
    quadrant "equal")."""
    T, R, Cc = shape
    if kind == "small":
        a = rng.integers(-3, 4, size=shape)
    elif kind == "wide":
        a = rng.integers(-(2 ** 29), 2 ** 29, size=shape)
        if T > 1:
            a[1] = a[0] + rng.integers(-300, 300, size=(R, Cc))
    elif kind == "noise":
        a = rng.integers(0, 70000, size=shape)
    elif kind == "const":
        a = np.zeros(shape, dtype=np.int64) + 5
        a[2:] += 1
    elif kind == "sparse":
        base = rng.integers(-100, 100, size=(R, Cc))
        a = np.stack([base.copy() for _ in range(T)])
        for i in range(1, T):
            for _ in range(3):
                a[i, rng.integers(R), rng.integers(Cc)] += rng.integers(-500, 500)
            if i == 3 % T:
                a[i, : R // 2, : Cc // 2] += 7
    else:
        raise ValueError(kind)
    return a.astype(np.int64)


def largest_below_2_29(dtype):
    """The largest scaled value the fused float kernels keep (|w| < 2^29) that `dtype` can hold at 3 fractional bits: 2^29 - 1
    in float64; float32 has 24 significant bits, its neighbour of 2^29 is 2^29 - 32."""
    return (1 << 29) - 1 if np.dtype(dtype) == np.float64 else (1 << 29) - 32


def contents(kind, shape, dtype, rng):
    """(array, fractional_bits, round) of one tile."""
    dtype = np.dtype(dtype)
    T, R, Cc = shape
    if not is_float(dtype):
        return int_field(kind, shape, rng).astype(dtype), 0, False
    if kind in INT_KINDS:
        bits = 20 if kind == "small" else 3
        return (int_field(kind, shape, rng) / 2.0 ** bits).astype(dtype), bits, False
    bits = 3
    base = rng.integers(-400, 400, size=(R, Cc))
    m = np.stack([base + (rng.random((R, Cc)) < 0.1) * rng.integers(-30, 30, size=(R, Cc)) for _ in range(T)]).astype(np.float64)
    if kind == "nan_blocks":
        x = m / 8.0
        x[0, 4:8, 4:8] = np.nan                  # a 4 x 4 block
        x[0, 8:16, 0:8] = np.nan                 # an 8 x 8 block
        x[T - 1, 8:16, 8:16] = np.nan
        x[T - 1, 0:4, 12:16] = np.nan
        if T > 2:
            x[1] = np.nan                        # a whole instant
            x[2, 0, :] = np.nan                  # a leading row
        if T > 3:
            x[3].reshape(-1)[::2] = np.nan       # every other cell
        return x.astype(dtype), bits, False
    if kind == "neg_fractions":
        # negative non-multiples of 2^-bits are neither rounded nor rejected (fixed.rs:45): the exact conversion, reached by
        # some 4-cell groups of a wave and not by others
        hit = rng.random(shape) < 0.15
        frac = rng.choice([0.25, 0.5, 0.75, 0.375], size=shape)
        x = np.where(hit, -(np.abs(m) + frac), m) / 8.0
        return x.astype(dtype), bits, False
    if kind == "round_ties":
        hit = rng.random(shape) < 0.30
        sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        x = np.where(hit, sign * (np.abs(m) + 0.5), m) / 8.0
        return x.astype(dtype), bits, True
    if kind == "subnormal":
        x = (m / 8.0).astype(dtype)
        tiny = np.finfo(dtype).tiny
        flat = x.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, 9), replace=False)
        flat[idx[0::3]] = dtype.type(tiny) / dtype.type(4)
        flat[idx[1::3]] = -dtype.type(tiny) / dtype.type(4)
        flat[idx[2::3]] = dtype.type(-0.0)
        return x, bits, True
    if kind in ("edge29", "edge29_over"):
        x = m / 8.0
        top = largest_below_2_29(dtype)
        x[0, 0, 0] = top / 8.0
        x[T - 1, R - 1, Cc - 1] = -(2.0 ** 29) / 8.0
        x[T // 2, R // 2, Cc // 3] = top / 8.0
        x[T - 1, R - 1, 0] = top / 8.0            # (the last instant / row is the one a broadcast view keeps)
        if kind == "edge29_over":
            x[T - 1, R - 1, Cc // 2] = (2.0 ** 29) / 8.0  # stored 2^30 + 1
        return x.astype(dtype), bits, False
    raise ValueError(kind)


ERR_NONFINITE, ERR_PRECISION, ERR_OVERFLOW = -2, -3, -4


def error_tiles(L, dtype, shape=None, rng=None):
    """Float tiles the reference panics on, one error KIND per tile (with several kinds in a tile the oracle reports the
    first it visits, the kernel the lowest-ranked): (name, array, fractional_bits, round, code)."""
    assert is_float(dtype)
    dtype = np.dtype(dtype)
    S = 1 << L
    shape = shape or (instants(L), S, S)
    T, R, Cc = shape
    rng = rng or np.random.default_rng(1000 + L)
    good = (rng.integers(-400, 400, size=shape) / 8.0).astype(dtype)
    at = (T - 2 if T > 1 else 0, R // 2, (2 * Cc) // 3)
    for name, value, code in (("precision", 5.0 + 1.0 / 64.0, ERR_PRECISION), ("infinity", -np.inf, ERR_NONFINITE),
                              ("beyond_i64", 1e30, ERR_OVERFLOW)):
        x = good.copy()
        x[at] = value
        yield name, x, 3, False, code


# ---- the matrix: every view x every content kind, each in a buffer of its own ------------------------------------------------

def aligned_buffer(nbytes, dtype):
    """A zeroed 1-D array of `dtype` holding at least nbytes, its first element 64-byte aligned."""
    esz = np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 64 + esz, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 64
    return raw[skip:skip + (nbytes + esz - 1) // esz * esz].view(dtype)


class Case:
    """One tile: `view` (numpy, inside `buffer` at byte_offset with `strides` in elements) holds the contents."""

    def __init__(self, L, dtype, view_name, kind, expected, make, array, bits, round_):
        self.L, self.dtype, self.view_name, self.kind, self.expected = L, np.dtype(dtype), view_name, kind, tuple(expected)
        self.name = "L%d-%s-%s-%s" % (L, self.dtype.name, view_name, kind)
        self.buffer = aligned_buffer(make.nbytes, dtype)
        self.byte_offset, self.strides, self.shape = make(self.buffer)
        self.view = as_view(self.buffer, self.byte_offset, self.strides, self.shape)
        self.view[...] = array  # (a broadcast view keeps the last instant: references are computed from the view)
        self.bits, self.round = bits, round_


def seeded(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def cases(L, dtype, only_kinds=None, only_views=None, map_fn=map):
    """Every view of views(L, dtype) x every content kind of kinds(dtype), deterministic.  map_fn: a thread pool's map, to
    fill the tiles in parallel."""
    todo = []
    for vname, expected, make in views(L, dtype):
        if only_views is not None and vname not in only_views:
            continue
        for kind in kinds(dtype):
            if only_kinds is None or kind in only_kinds:
                todo.append((vname, expected, make, kind))

    def one(spec):
        vname, expected, make, kind = spec
        shape = make(aligned_buffer(make.nbytes, dtype))[2]
        a, bits, rnd = contents(kind, shape, dtype, seeded(L, np.dtype(dtype).name, vname, kind))
        return Case(L, dtype, vname, kind, expected, make, a, bits, rnd)
    return list(map_fn(one, todo))
