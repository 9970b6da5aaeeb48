"""dcdf_superchunk_build on the card over the case table of tests/superchunk_cases.py, from HOST views (Superchunk.build: the
upload re-densifies the view) and from DEVICE views (Superchunk.build_device: the caller's strides reach k_tile_minmax,
k_suggest and the encoder's loaders as they are), for k = 2, 3, 4, 5 and 16, against the oracle: root CID, every stored object
byte for byte, the same object set, the six counters.  Error cases report the oracle's code and leave the pools and rings as
the next call expects them; the k = 2 objects are decoded on the card and give the source raster back.
tests/test_superchunk_cases_host.py checks the table itself without a GPU.

One family at a time:  pytest tests/test_gpu_superchunk_cases.py -k nan_order"""
import numpy as np
import pytest

import encode_cases as E
import oracle_lib as O
import oracle_superchunk as OS
import superchunk_cases as SC
from raster_rebuild import rebuild_from

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


class Ref:
    """What the oracle makes of a case's view: code (0, the reference's panic, or BAD_ARG for levels it refuses), the store, the
    root CID, the node, the stats."""

    def __init__(self, case):
        self.store, self.root, self.obj, self.stats = OS.Store(), None, None, None
        try:
            self.obj, self.stats = OS.superchunk_build(case.view, list(case.levels), case.k, self.store, case.bits, case.round)
            self.root = self.store.save(self.obj)
            self.code = 0
        except O.OracleError as e:
            self.code = e.code
        except ValueError:
            self.code = SC.ERR_BAD_ARG


REFS = {}


def ref_of(case):
    if case.name not in REFS:
        REFS[case.name] = Ref(case)
    return REFS[case.name]


def same_as_oracle(b, case):
    """tests/test_gpu_superchunk.py check(), against the case's oracle result."""
    r = ref_of(case)
    assert r.code == 0
    st = r.stats
    assert b.cid == r.root and bytes(b.data) == r.obj, case.name
    assert set(b.objects) == set(r.store), (case.name, len(b.objects), len(r.store))
    for cid, o in r.store.items():
        assert bytes(b.objects[cid]) == o, case.name
    assert (b.size, b.elided, b.local, b.external, b.snapshots, b.logs) == (st["size"], st["elided"], 0, st["external"], st["snapshots"], st["logs"]), case.name


def build_host(dc, c):
    return dc.Superchunk.build(c.view, c.levels, k=c.k, fractional_bits=c.bits, round=c.round)


def build_device(dc, c):
    """The case's buffer in a device allocation of its size, its view handed over as pointer, strides and shape."""
    from dcdf_amd.encoder import DeviceBuffer
    lo, hi = E.extent(c.byte_offset, c.strides, c.shape, c.dtype.itemsize)
    assert 0 <= lo and hi <= c.buffer.nbytes  # what the kernels may read lies inside the allocation
    buf = DeviceBuffer(c.buffer.nbytes)
    try:
        buf.write(0, c.buffer)
        return dc.Superchunk.build_device(buf.ptr + c.byte_offset, c.dtype, c.strides, c.shape, c.levels, k=c.k, fractional_bits=c.bits, round=c.round)
    finally:
        buf.free()


BUILDERS = {"host": build_host, "device": build_device}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", SC.good_cases(), ids=lambda c: c.name)
def test_every_case_matches_the_oracle(dc, case, where):
    same_as_oracle(BUILDERS[where](dc, case), case)


@pytest.mark.parametrize("band_mb", ["0", "1"])
def test_host_views_with_and_without_bands(dc, band_mb, monkeypatch):
    """Every case with two or more tile rows as a host view with the bands switched off (K2R_SC_BAND_MB=0) and at 1 MiB a band:
    the `banded` rasters hold exactly 1 MiB per tile row and go up in three bands of one tile row each, their chunks encoded and
    fetched by the thread of their own; the smaller ones fit one band either way."""
    monkeypatch.setenv("K2R_SC_BAND_MB", band_mb)
    picked = [c for c in SC.good_cases() if c.tile_rows() >= 2]
    assert sum("banded" in c.tags for c in picked) == 2 and {c.view_name for c in picked} == set(SC.VIEW_NAMES)
    for c in picked:
        same_as_oracle(build_host(dc, c), c)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", [c for c in SC.error_cases() if "two_causes" not in c.tags], ids=lambda c: c.name)
def test_single_cause_errors(dc, case, where, monkeypatch):
    """One cause per raster, in its last tile (of the last band, when the raster goes up in bands): the call reports the
    reference's panic as the oracle's code, and a good build of the same shape right after matches the oracle."""
    if "banded" in case.tags:
        monkeypatch.setenv("K2R_SC_BAND_MB", "1")
    assert ref_of(case).code == case.code != 0
    with pytest.raises(dc.DcdfError) as e:
        BUILDERS[where](dc, case)
    assert e.value.code == case.code, case.hits
    good = SC.by_name(case.good)
    same_as_oracle(BUILDERS[where](dc, good), good)


@pytest.mark.parametrize("where", ["host", "device"])
def test_two_causes_in_one_raster(dc, where):
    """Tile 0 gets a Round verdict under round = False (-3, DCDF_ERR_PRECISION), tile 3 holds an infinity (-2,
    DCDF_ERR_NONFINITE).  The reference builds tile by tile -- (min, max), fractional bits, Chunk::build of tile 0 before it looks
    at tile 1 -- so its first panic is tile 0's "loss of precision" (the oracle: -3).  The library computes (min, max) of all
    tiles of a band, then all fractions, then builds: it meets tile 3's infinity in the first step and returns -2
    (DCDF_ERR_NONFINITE).  Both are panics in the reference; which of two causes is reported is not part of the contract, that
    one of them is and that the next call works, is."""
    case = SC.by_name("error-two_causes")
    assert ref_of(case).code == SC.ERR_PRECISION
    with pytest.raises(dc.DcdfError) as e:
        BUILDERS[where](dc, case)
    print("two causes, %s view: the library reports %d, the oracle %d" % (where, e.value.code, ref_of(case).code))
    assert e.value.code in case.expect["codes"]
    good = SC.by_name(case.good)
    same_as_oracle(BUILDERS[where](dc, good), good)


def test_argument_checks(dc):
    """DCDF_ERR_BAD_ARG: fewer than two levels, k outside 2..16, levels whose sum is not what the raster needs (k = 3; k = 5
    and 125 wide with three levels, where the f64 formula asks for four)."""
    a27 = SC.by_name("k3-27-levels_1_2")
    a125 = SC.by_name("k5-125x100-levels_1_2-refused")
    bad = [(a27, [3], 3), (a27, [1, 2], 1), (a27, [1, 2], 17), (a27, [1, 1], 3), (a27, [2, 2], 3), (a125, [1, 2], 5), (a125, [3], 5)]
    for c, levels, k in bad:
        with pytest.raises(dc.DcdfError) as e:
            dc.Superchunk.build(c.view, levels, k=k)
        assert e.value.code == SC.ERR_BAD_ARG, (c.name, levels, k)
    same_as_oracle(build_host(dc, a27), a27)


ROUND_TRIPS = ["nan_tiles-float32", "view-int32-window", "fractions-round_4", "dedup-nested"]


@pytest.mark.parametrize("name", ROUND_TRIPS)
def test_k2_objects_decode_to_the_source_on_the_card(dc, name):
    """The objects the card built, flattened by leaf_grid into the leaves of a raster (dcdf_raster_create_tiles, as
    Variable.raster() does) and decoded on the card: the source raster, NaN for NaN -- a float raster with an elided all-NaN
    tile, a ragged integer one, a nested one; the rounded one gives what the oracle reads out of the same objects."""
    from dcdf_amd.chunk import Chunk
    from dcdf_amd.dataset import leaf_grid
    from dcdf_amd.raster import EncodedRaster, RasterTile
    c = SC.by_name(name)
    assert c.k == 2 and c.code == 0
    b = build_host(dc, c)
    same_as_oracle(b, c)
    a = np.array(c.view)
    T = c.shape[0]
    leaf, grid = leaf_grid(b.objects, [b.cid], c.levels, c.round)
    opened = {}

    def chunk(cid):
        if cid not in opened:
            opened[cid] = Chunk(bytes(b.objects[cid][8:]))
        return opened[cid]

    tiles = [RasterTile(None if lf.cid is None else chunk(lf.cid), lf.row0, lf.col0, lf.values, lf.minmax, lf.encoding, lf.fractional_bits,
                        lf.exact) for lf in grid[0]]
    assert any(t.chunk is None for t in tiles) == (name in ("nan_tiles-float32",))
    r = EncodedRaster.from_tiles(c.shape, tiles, leaf, T)
    got = r.decode(0, T, dtype=a.dtype)
    r.close()
    want, _ = rebuild_from(b.objects, [b.cid], a, c.levels, T, c.round)
    np.testing.assert_array_equal(got, want)
    if c.exact:
        np.testing.assert_array_equal(got, a)
    else:
        assert (got != a).any()
