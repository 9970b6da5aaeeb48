"""The case table of the superchunk assembly's tests (dcdf_superchunk_build = Superchunk::build, superchunk.rs:88-270): rasters
named for what they are there to hit, each inside a buffer of its own as a strided view.  Pure numpy: imports neither the GPU
nor the library, so the host test (tests/test_superchunk_cases_host.py: the table keeps its promises in the oracle) and the GPU
test (tests/test_gpu_superchunk_cases.py: host and device views against the oracle) walk the same table.  The vocabulary of
views (aligned_buffer, extent, as_view, seeded) is that of tests/encode_cases.py.

  cases()          -> [Case], deterministic, built once per process
  Case             .name .tags .hits  .buffer .byte_offset .strides .shape .view  .levels .k .bits .round
                   .code     0, an error code of the library (ERR_*), or BAD_ARG (the oracle raises ValueError)
                   .expect   promises about the oracle's result: elided / links / references / chunk_bits (sorted byte 1 of
                             every stored chunk) / codes (a case with two causes: the codes an implementation may report)
                   .exact    every value is stored without loss (a rebuilt raster equals the source)
                   .good     an error case: the name of a good case of the same shape
  nan_layouts(n)   -> the NaN-order layouts for a tile of n cells; nan_behind(flat) -> the rule of min_max_float restated
"""
import numpy as np

import encode_cases as E

ERR_BAD_ARG, ERR_NONFINITE, ERR_PRECISION, ERR_OVERFLOW = -1, -2, -3, -4


# ---- views of a [T, R, C] raster: every one has the raster's shape, so one raster gives one oracle result under all of them ----

def views(shape, dtype):
    """(name, byte_offset, strides in elements, bytes of buffer needed)."""
    T, R, Cc = shape
    esz = np.dtype(dtype).itemsize
    W = Cc + 7  # the row of a wider array

    def one(name, byte_offset, strides):
        lo, hi = E.extent(byte_offset, strides, shape, esz)
        assert lo >= 0
        return name, byte_offset, tuple(strides), hi

    yield one("dense", 0, (R * Cc, Cc, 1))
    yield one("window", esz, (R * W + 3, W, 1))                  # a crop: row pitch, base one element in
    yield one("transposed", 0, (R * Cc, 1, R))                   # the transpose of a dense [T, C, R] array
    yield one("reversed_rows", (R - 1) * Cc * esz, (R * Cc, -Cc, 1))
    yield one("col_step_2", 0, (2 * R * Cc, 2 * Cc, 2))
    yield one("broadcast_instants", 0, (0, Cc, 1))               # one instant read T times (it keeps the last one written)


VIEW_NAMES = ("dense", "window", "transposed", "reversed_rows", "col_step_2", "broadcast_instants")


class Case:
    def __init__(self, name, array, levels, k=2, bits=0, round_=False, hits="", tags=(), view="dense", code=0, expect=None,
                 exact=True, good=None):
        array = np.asarray(array)
        assert array.ndim == 3
        self.name, self.levels, self.k, self.bits, self.round = name, list(levels), int(k), int(bits), bool(round_)
        self.hits, self.tags, self.view_name, self.code = hits, frozenset(tags), view, code
        self.expect, self.exact = dict(expect or {}), exact
        self.good = good  # an error case: the name of a good case of the same shape, to build right after it
        self.dtype = array.dtype
        _, off, strides, nbytes = next(v for v in views(array.shape, array.dtype) if v[0] == view)
        self.buffer = E.aligned_buffer(nbytes, array.dtype)
        self.byte_offset, self.strides, self.shape = off, strides, tuple(array.shape)
        self.view = E.as_view(self.buffer, off, strides, self.shape)
        self.view[...] = array  # (a broadcast view keeps the last instant: references are computed from the view)
        self.buffer.flags.writeable = False
        self.view.flags.writeable = False

    def tile_rows(self):
        """Rows of the top level's grid that hold cells of the raster."""
        side = self.k ** sum(self.levels) // self.k ** self.levels[0]
        return -(-self.shape[1] // side)

    def __repr__(self):
        return "Case(%s)" % self.name


# ---- NaN order (min_max_float, mmbuffer.rs:465-499) ---------------------------------------------------------------------------

def nan_layouts(n):
    """(name, NaN positions) in row-major positions of a tile of n cells.  A 32 x 32 tile (1024 cells: four strides of a
    256-thread loop) takes the positions as they are named; a smaller one (the ragged 8 x 5 tile has 40 cells: most threads
    idle) takes the same layouts with the first number at 30 instead of 300, and its middle cells for 255 / 256.  A cell is a
    NaN or a number, so "a NaN behind the first number" has no case of equality: the NaN directly before the first number and
    the one directly behind it are the closest a layout can come to the rule's edge."""
    big = n > 302
    lead = 300 if big else 30
    assert n > lead + 2
    return [
        ("nan_at_0", [0]),
        ("nan_at_0_to_2", [0, 1, 2]),
        ("leading_nans_first_number_at_%d" % lead, list(range(lead))),               # NaN next to the first number, before it
        ("number_at_0_nan_at_1", [1]),                                                # NaN next to the first number, behind it
        ("first_number_at_%d_nan_at_%d" % (lead, lead + 1), list(range(lead)) + [lead + 1]),
        ("nan_at_255", [255 if big else n // 2 - 1]),                                 # the last cell of the loop's first stride
        ("nan_at_256", [256 if big else n // 2]),                                     # the first cell of the second: thread 0 again
        ("nan_at_last_cell", [n - 1]),
        ("all_nan", list(range(n))),
    ]


LAYOUT_NAMES = [name for name, _ in nan_layouts(1024)]


def nan_behind(flat):
    """min_max_float's rule, restated without its loop: (all NaN, a NaN lies behind the first number)."""
    isn = np.isnan(flat)
    if isn.all():
        return True, False
    first = int(np.argmin(isn))
    return False, bool(isn[first + 1:].any())


def tiles_of(shape, side):
    """(top, bottom, left, right) of every tile of the top level's grid that holds cells, row-major."""
    _, R, Cc = shape
    return [(t, min(t + side, R), l, min(l + side, Cc)) for t in range(0, R, side) for l in range(0, Cc, side)]


def _eighths(rng, shape, dtype, lo=-400, hi=400):
    return (rng.integers(lo, hi, size=shape) / 8.0).astype(dtype)


def nan_order_rasters(dtype):
    """Two [.., 40, 37] rasters, levels [1, 5]: a 32 x 32 tile, 32 x 5, 8 x 32 and the ragged 8 x 5 tile, every tile of every
    instant in one layout of nan_layouts (the same layout name for the four tiles of an instant).  Returns [(array, [layout
    name per instant])]."""
    out = []
    for part, names in enumerate((LAYOUT_NAMES[:5], LAYOUT_NAMES[5:])):
        shape = (len(names), 40, 37)
        a = _eighths(E.seeded("superchunk", "nan_order", np.dtype(dtype).name, part), shape, dtype)
        for t, l in enumerate(names):
            i = LAYOUT_NAMES.index(l)
            for top, bottom, left, right in tiles_of(shape, 32):
                tile = a[t, top:bottom, left:right]
                flat = tile.reshape(-1).copy()
                flat[nan_layouts(flat.size)[i][1]] = np.nan
                tile[...] = flat.reshape(tile.shape)
        out.append((a, list(names)))
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------------

def _ints(key, shape, dtype=np.int32, lo=-1000, hi=1000):
    return E.seeded("superchunk", key).integers(lo, hi, size=shape).astype(dtype)


def base_raster(dtype):
    """The raster the views and the error cases are made of: [4, 40, 52] under levels [2, 4], a 4 x 4 grid of 16-tiles whose
    last tile row lies outside (elided), its third ragged below; floats are multiples of 1/8 with two NaNs."""
    shape = (4, 40, 52)
    if np.dtype(dtype).kind == "i":
        return _ints(("base", np.dtype(dtype).name), shape, dtype)
    a = _eighths(E.seeded("superchunk", "base", np.dtype(dtype).name), shape, dtype)
    a[1, 5, 5] = np.nan
    a[2, 33, 50] = np.nan
    return a


BASE_LEVELS = [2, 4]


def fraction_raster(with_tenth):
    """float64 [3, 72, 40] under levels [2, 5]: a 3 x 2 grid of 32-tiles, ragged bottom and right, tile contents multiples of
    1/2, 1/32, 1/8, 1, 1/4, 1/16 -- each tile holds odd multiples, so it needs exactly its bits.  with_tenth: one cell of the
    1/8 tile holds 0.1 (Precise with some 56 bits: not a multiple of any 2^-n a raster would ask for)."""
    shape = (3, 72, 40)
    rng = E.seeded("superchunk", "fractions")
    a = np.zeros(shape, dtype=np.float64)
    for (top, bottom, left, right), den in zip(tiles_of(shape, 32), (2, 32, 8, 1, 4, 16)):
        n = rng.integers(-3000, 3000, size=(3, bottom - top, right - left))
        n[:, 0, 0] |= 1  # an odd multiple in every instant
        a[:, top:bottom, left:right] = n / float(den)
    if with_tenth:
        a[1, 40, 7] = 0.1  # (tile 2, the 1/8 tile)
    return a


def round_verdict_raster():
    """float64 [2, 32, 32] under levels [1, 4] (four 16-tiles), multiples of 1/4 in +-100, and in tile 0 one 2^-60 that is neither
    the minimum nor the maximum of its instant: to_fixed of every (min, max) is exact at 2 bits, suggest_fraction says Round(55)
    for tile 0 (7 whole bits leave 55; 2^-60 does not fit them)."""
    a = (E.seeded("superchunk", "round_verdict").integers(-400, 400, size=(2, 32, 32)) / 4.0).astype(np.float64)
    a[:, 0, 0], a[:, 0, 1] = -100.0, 100.0
    a[1, 3, 3] = 2.0 ** -60
    return a


def _build():
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))

    # -- arity: ref_levels' f64 formula, the tile grid and the universal encoder under the assembly, k = 3, 4, 5, 16
    a27 = _ints("k3_27", (5, 27, 27))
    add("k3-27-levels_1_2", a27, [1, 2], k=3, tags={"arity"}, hits="3 x 3 tiles of 9", expect={"elided": 0, "references": 9, "links": 9})
    add("k3-27-levels_2_1", a27, [2, 1], k=3, tags={"arity"}, hits="9 x 9 tiles of 3", expect={"elided": 0, "references": 81})
    add("k3-27-levels_1_1_1", a27, [1, 1, 1], k=3, tags={"arity", "nested"}, hits="nested: 9 Superchunk children",
        expect={"elided": 0, "references": 9, "links": 9, "children": 9})
    add("k3-ragged_20x25-levels_1_2", _ints("k3_ragged", (5, 30, 30))[:, 3:23, 2:27].copy(), [1, 2], k=3, tags={"arity"},
        hits="ragged tiles 2 rows / 7 cols", expect={"elided": 0, "references": 9})
    f27 = (_ints("k3_f32", (5, 27, 27)) / 4.0).astype(np.float32)
    f27[2, 10, 10] = np.nan
    f27[3, 0, 0] = np.nan
    add("k3-27-float32-nan", f27, [1, 2], k=3, bits=2, tags={"arity", "float"}, hits="float tiles at k = 3, a NaN behind and a leading NaN",
        expect={"elided": 0, "references": 9})
    add("k4-64-int64-levels_1_2", _ints("k4_64", (3, 64, 64), np.int64, -(1 << 40), 1 << 40), [1, 2], k=4, tags={"arity"},
        hits="4 x 4 tiles of 16, int64", expect={"elided": 0, "references": 16})
    add("k4-50x33-levels_2_1", _ints("k4_50", (3, 50, 33)), [2, 1], k=4, tags={"arity"}, hits="16 x 16 tiles of 4, 139 outside",
        expect={"elided": 139, "references": 117})
    a125 = _ints("k5_125", (2, 125, 100))
    add("k5-125x100-levels_1_3", a125, [1, 3], k=5, tags={"arity", "k5"}, hits="ceil(log(125) / log(5)) = 4 in f64: sidelen 625, 24 of 25 tiles outside",
        expect={"elided": 24, "references": 1, "sidelen": 625})
    add("k5-125x100-levels_2_2", a125, [2, 2], k=5, tags={"arity", "k5"}, hits="sidelen 625, 25 x 25 tiles of 25", expect={"elided": 605, "references": 20, "sidelen": 625})
    add("k5-125x100-levels_3_1", a125, [3, 1], k=5, tags={"arity", "k5"}, hits="sidelen 625, 125 x 125 tiles of 5", expect={"elided": 15125, "references": 500, "sidelen": 625})
    add("k5-125x100-levels_1_2-refused", a125, [1, 2], k=5, tags={"arity", "k5", "error"}, code=ERR_BAD_ARG, good="k5-125x100-levels_1_3",
        hits="three levels would do for integers; the reference's f64 formula needs four")
    add("k16-200x256-levels_1_1", _ints("k16", (2, 200, 256)), [1, 1], k=16, tags={"arity"}, hits="16 x 16 tiles of 16, the last 3 1/2 tile rows outside",
        expect={"elided": 48, "references": 208, "links": 208})

    # -- NaN order
    for dtype in (np.float32, np.float64):
        dn = np.dtype(dtype).name
        for part, (a, names) in enumerate(nan_order_rasters(dtype)):
            add("nan_order-%s-%d" % (dn, part), a, [1, 5], bits=3, tags={"nan", "nan_order", "float"}, hits="instants: " + ", ".join(names),
                expect={"layouts": names})
        a = _eighths(E.seeded("superchunk", "nan_tiles", dn), (4, 40, 37), dtype, 8, 400)
        a[:, :32, 32:] = np.nan            # tile 1: NaN in every instant -- stored 0, min == max: elided
        a[:, 32:, :32] = np.nan            # tile 2: every instant NaN but one
        a[2, 32:, :32] = _eighths(E.seeded("superchunk", "nan_tiles_one", dn), (8, 32), dtype)
        a[0, 3, 4], a[0, 20, 9] = -0.0, 0.0  # tile 0: the zeros are the only candidates for the minimum, -0.0 met first ...
        a[1, 3, 4], a[1, 20, 9] = 0.0, -0.0  # ... and +0.0 met first: both are stored as 1
        add("nan_tiles-%s" % dn, a, [1, 5], bits=3, tags={"nan", "float"}, hits="a tile NaN in every instant (elided), one NaN in all but one, signed zeros as minimum",
            expect={"elided": 1, "references": 3})

    # -- per-tile fractional bits
    add("fractions-round_4", fraction_raster(True), [2, 5], bits=4, round_=True, tags={"fractions", "float"}, exact=False,
        hits="per-tile bits min(suggested, 4)", expect={"chunk_bits": [0, 1, 2, 4, 4, 4], "elided": 10})
    add("fractions-round_30", fraction_raster(True), [2, 5], bits=30, round_=True, tags={"fractions", "float"}, exact=False,
        hits="per-tile bits min(suggested, 30): 0.1 takes all 30", expect={"chunk_bits": [0, 1, 2, 4, 5, 30], "elided": 10})
    add("fractions-exact_5", fraction_raster(False), [2, 5], bits=5, tags={"fractions", "float"},
        hits="per-tile bits as suggested, round = False", expect={"chunk_bits": [0, 1, 2, 3, 4, 5], "elided": 10})
    add("round_verdict-rounded", round_verdict_raster(), [1, 4], bits=2, round_=True, tags={"fractions", "float"}, exact=False,
        hits="suggest_fraction says Round(55) for tile 0; round = True takes min(55, 2)", expect={"chunk_bits": [2, 2, 2, 2]})
    add("round_verdict-refused", round_verdict_raster(), [1, 4], bits=2, tags={"fractions", "float", "error"}, code=ERR_PRECISION, good="round_verdict-rounded",
        hits="the same with round = False: panic 'loss of precision' (mmbuffer.rs:607) though every (min, max) converts")

    # -- wide integers: eight byte planes in the min / max Dacs
    w = E.seeded("superchunk", "wide").integers(-(1 << 62), 1 << 62, size=(3, 16, 16), dtype=np.int64)
    w[0, 0, 0], w[1, 15, 15] = -(1 << 62), (1 << 62) - 1
    add("wide_int64", w, [1, 3], tags={"wide"}, hits="int64 over +-2^62: (min, max) with eight Dac planes", expect={"elided": 0, "references": 4})
    w2 = w.copy()
    w2[:, 8:, :8] = -(1 << 62)
    add("wide_int64-elided_tile", w2, [1, 3], tags={"wide"}, hits="a tile constant at -2^62: elided, its value lives in the Dacs alone",
        expect={"elided": 1, "references": 3})

    # -- de-duplication of equal sub-chunks and of equal nested superchunks
    q = _ints("dedup", (3, 32, 32))
    q[:, 16:, 16:] = q[:, :16, :16]
    q[:, 16:, :16] = q[:, :16, 16:]
    add("dedup-chunks", q, [1, 4], tags={"dedup"}, hits="four tiles pairwise equal", expect={"elided": 0, "references": 4, "links": 2})
    add("dedup-nested", np.tile(q, (1, 2, 2)), [1, 1, 4], tags={"dedup", "nested"}, hits="four equal Superchunk children, each with two distinct chunks",
        expect={"elided": 0, "references": 4, "links": 1, "children": 1})

    # -- views of the integer and the float base raster
    for dtype, bits in ((np.int32, 0), (np.float32, 3)):
        for v in VIEW_NAMES:
            add("view-%s-%s" % (np.dtype(dtype).name, v), base_raster(dtype), BASE_LEVELS, bits=bits, view=v,
                tags={"views", "float"} if bits else {"views"}, hits="4 x 4 grid of 16-tiles, one tile row outside, through a %s view" % v,
                expect={"elided": 4, "references": 12})

    # -- three bands of one tile row each when a host view is uploaded with K2R_SC_BAND_MB=1 (a tile row of every instant is 1 MiB)
    big = _ints("banded", (8, 192, 256), np.int64, -(1 << 20), 1 << 20)
    add("banded-int64", big, [2, 6], tags={"banded"}, hits="4 x 4 grid of 64-tiles, three tile rows inside: 1 MiB per tile row",
        expect={"elided": 4, "references": 12})

    # -- errors: one cause per raster, in the last tile that holds cells
    f = base_raster(np.float32)
    last = (3, 39, 51)
    g = f.copy(); g[last] = np.inf
    add("error-infinity", g, BASE_LEVELS, bits=3, tags={"error", "float"}, code=ERR_NONFINITE, good="view-float32-dense", hits="to_fixed of a tile's max (fixed.rs:39-41)")
    g = np.round(f * 4) / 4; g[last] = 60.125  # (every other (min, max) is a multiple of 1/4)
    add("error-minmax_precision", g, BASE_LEVELS, bits=2, tags={"error", "float"}, code=ERR_PRECISION, good="view-float32-dense",
        hits="a tile's max is an odd multiple of 1/8 under 2 bits, round = False (fixed.rs:47-58)")
    g = f / 16; g[last] = 200.0  # (every other value lies within +-4: 60 bits hold it)
    add("error-to_fixed_overflow", g, BASE_LEVELS, bits=60, tags={"error", "float"}, code=ERR_OVERFLOW, good="view-float32-dense", hits="200 * 2^61 is no i64 (fixed.rs:64-70); the other tiles stay within +-3.2")
    g = f.astype(np.float64); g[last] = 1e300
    add("error-beyond_62_bits", g, BASE_LEVELS, bits=3, round_=True, tags={"error", "float"}, code=ERR_OVERFLOW, good="view-float32-dense",
        hits="1e300: to_fixed of the tile's max overflows before suggest_fraction can (a value with more than 62 whole bits is "
             "always its instant's max, so suggest_fraction's own overflow, fixed.rs:129, cannot be reached first)")
    fb = _eighths(E.seeded("superchunk", "banded_error"), (8, 192, 256), np.float64)
    add("banded-float64", fb, [2, 6], bits=3, tags={"banded", "float"}, hits="the same grid in float64: fractional bits band by band",
        expect={"elided": 4, "references": 12})
    fb = fb.copy()
    fb[7, 191, 255] = -np.inf
    add("error-infinity-last_band", fb, [2, 6], bits=3, tags={"error", "float", "banded"}, code=ERR_NONFINITE, good="banded-float64",
        hits="the last tile of the third band, earlier bands' sessions in flight")
    two = round_verdict_raster()
    two[0, 31, 31] = np.inf
    add("error-two_causes", two, [1, 4], bits=2, tags={"error", "float", "two_causes"}, code=ERR_PRECISION, good="round_verdict-rounded",
        hits="tile 0: Round verdict with round = False; tile 3: an infinity", expect={"codes": [ERR_PRECISION, ERR_NONFINITE]})
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert (c.good is None) == (c.code == 0)
        if c.good:
            g = next(x for x in out if x.name == c.good)
            assert g.code == 0 and g.shape == c.shape and g.k == c.k
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def by_name(name):
    return next(c for c in cases() if c.name == name)


def good_cases():
    return [c for c in cases() if c.code == 0]


def error_cases():
    return [c for c in cases() if c.code != 0]
