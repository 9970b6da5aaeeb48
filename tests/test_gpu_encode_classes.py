"""Every fused encoder kernel k_encode<L, PADDED, VEC> (L = 4..8; P0_V0, P1_V0, P0_V1..V4) run on the card from device views,
for every element type it serves, against the CPU oracle, bit for bit.  The cases are the table of tests/encode_cases.py
(tests/test_encode_cases_host.py checks the table itself and runs it through the host simulator); which kernel a tile took
is asked of the library (dcdf_encoder_tile_kernel), never restated here.

One L at a time:  pytest tests/test_gpu_encode_classes.py -k L6"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import encode_cases as E
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


def code_of(dtype):
    return O.ENC[np.dtype(dtype)]


def pool_map(fn, items):
    nthr = max(1, min(16, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(nthr) as ex:
        return list(ex.map(fn, items))


class Ref:
    """What the oracle makes of a case's view: code (0 or the reference's panic), bytes, counters, per-instant stored
    (min, max) -- of the integers themselves, for floats of the oracle chunk's stored fixed-point values (NaN = 0 takes part)."""

    def __init__(self, case):
        T, R, Cc = case.shape
        self.data, self.ns, self.nl, self.mm = None, 0, 0, None
        try:
            self.data, self.ns, self.nl, _ = O.chunk_build(case.view, fractional_bits=case.bits, round_=case.round, want_snapshots=True)
            self.code = 0
        except O.OracleError as e:
            self.code = e.code
            return
        if E.is_float(case.dtype):
            stored = O.Chunk(self.data).fill_window(0, T, 0, R, 0, Cc, dtype=np.int64)
        else:
            stored = np.asarray(case.view)
        flat = stored.reshape(T, -1)
        self.mm = np.stack([flat.min(1), flat.max(1)], axis=1).astype(np.int64)


VIEWS_WITH_EXTRAS = ("dense", "subtile", "base_plus_1", "padded_subtile")


def padded_subtile_name(L):
    return "padded_%dx%d_subtile" % ((1 << L) - 1, 1 << L)


class Table:
    """The matrix of one L: cases[dtype] = every view x content kind; extras[(dtype, view)] = the three error tiles and an
    all-NaN tile in that view (floats).  Every case carries its oracle result as .ref, computed once."""

    def __init__(self, L):
        self.L = L
        self.cases = {np.dtype(d): E.cases(L, d, map_fn=pool_map) for d in E.DTYPES}
        self.extras = {}
        for d in (np.float32, np.float64):
            for vname, expected, make in E.views(L, d):
                key = "padded_subtile" if vname == padded_subtile_name(L) else vname
                if key not in VIEWS_WITH_EXTRAS:
                    continue
                shape = make(E.aligned_buffer(make.nbytes, d))[2]
                lst = []
                for name, x, bits, rnd, code in E.error_tiles(L, d, shape=shape):
                    c = E.Case(L, d, vname, "error_" + name, expected, make, x, bits, rnd)
                    c.want_code = code
                    lst.append(c)
                lst.append(E.Case(L, d, vname, "all_nan", expected, make, np.full(shape, np.nan, dtype=d), 3, False))
                self.extras[(np.dtype(d), key)] = lst
        everything = [c for lst in self.cases.values() for c in lst] + [c for lst in self.extras.values() for c in lst]
        for c, r in zip(everything, pool_map(Ref, everything)):
            c.ref = r

    def pick(self, dtype, view, kind):
        view = padded_subtile_name(self.L) if view == "padded_subtile" else view
        hit = [c for c in self.cases[np.dtype(dtype)] if c.view_name == view and c.kind == kind]
        assert len(hit) == 1, (dtype, view, kind)
        return hit[0]


@pytest.fixture(scope="module", params=E.LEVELS, ids=lambda L: "L%d" % L)
def table(request):
    return Table(request.param)


class Session:
    """The cases' buffers in one device allocation (each at a 256-byte aligned offset, so a view keeps its alignment), their
    views as the tile descs of one Encoder session."""

    def __init__(self, cases):
        from dcdf_amd.encoder import DeviceBuffer, Encoder
        self.cases = cases
        offs, total = [], 0
        for c in cases:
            offs.append(total)
            total += (c.buffer.nbytes + 255) & ~255
        self.buf = DeviceBuffer(total)
        assert self.buf.ptr % 256 == 0
        descs = []
        for c, o in zip(cases, offs):
            lo, hi = E.extent(c.byte_offset, c.strides, c.shape, c.dtype.itemsize)
            assert 0 <= lo and hi <= c.buffer.nbytes and o + hi <= total  # what the kernel may read lies inside the allocation
            self.buf.write(o, c.buffer)
            descs.append((self.buf.ptr + o + c.byte_offset, code_of(c.dtype), c.strides, c.shape, c.bits, c.round))
        self.enc = Encoder(descs, k=2)
        self.ms = self.enc.run()
        self.packed, self.goffs, self.glens, self.mm = self.enc.gather()
        self.mmoff = np.concatenate([[0], np.cumsum([c.shape[0] for c in cases])])

    def outcome(self, i):
        """(status, bytes, snapshots, logs, minmax bytes) of tile i."""
        st, ln, ns, nl = self.enc.result(i)
        if st != 0:
            return st, None, 0, 0, None
        return st, self.enc.fetch(i), ns, nl, self.mm[self.mmoff[i]:self.mmoff[i + 1]].tobytes()

    def problems(self, i, expect_kernel=True):
        """What differs from the oracle (and, between themselves, the session's ways of handing a result out) for tile i."""
        c, out = self.cases[i], []
        if expect_kernel and self.enc.tile_kernel(i) != (c.L,) + c.expected + (0,):
            out.append("kernel %s, expected %s" % (self.enc.tile_kernel(i), (c.L,) + c.expected))
        st, data, ns, nl, mm = self.outcome(i)
        if st != c.ref.code:
            return out + ["status %d, oracle %d" % (st, c.ref.code)]
        if st != 0:
            if self.glens[i] != 0:
                out.append("a failed tile with gathered bytes")
            return out
        if data != c.ref.data:
            n = min(len(data), len(c.ref.data))
            first = next((j for j in range(n) if data[j] != c.ref.data[j]), n)
            out.append("bytes differ: len %d vs %d, first diff at %d" % (len(data), len(c.ref.data), first))
        if (ns, nl) != (c.ref.ns, c.ref.nl):
            out.append("snapshots, logs %s, oracle %s" % ((ns, nl), (c.ref.ns, c.ref.nl)))
        o, ln = int(self.goffs[i]), int(self.glens[i])
        if o % 16 != 0 or ln != len(data) or self.packed[o:o + ln].tobytes() != data:
            out.append("gather() disagrees with fetch()")
        if mm != c.ref.mm.tobytes():
            out.append("minmax differs from the stored integers' (min, max)")
        return out

    def close(self):
        self.enc.close()
        self.buf.free()


def report(bad):
    assert not bad, "%d tiles wrong, the first: %s" % (len(bad), bad[:8])


def test_every_class_every_dtype(dc, table):
    """Every view x content kind of the table as the tiles of one session per element type: the kernel the library says it chose
    is the expected one, status 0, the oracle's bytes and counters, gather() == fetch(), per-instant (min, max) of the stored
    integers.  (A tile with a stored value beyond 2^30 is declined by its fused kernel and comes back from the universal one.)"""
    seen = set()
    for dtype, cases in table.cases.items():
        s = Session(cases)
        bad = [(c.name, p) for i, c in enumerate(cases) for p in s.problems(i)]
        seen |= {s.enc.tile_kernel(i)[:3] + (dtype.name,) for i in range(len(cases))}
        s.close()
        report(bad)
        assert all(c.ref.code == 0 for c in cases)
    L = table.L
    want = {(L, p, v, np.dtype(d).name) for d in E.DTYPES for p, v in ((0, 0), (1, 0), (0, E.LOADER[np.dtype(d)]))}
    assert seen == want  # the six kernels of this L, each with every element type it serves


def test_host_arrays_take_the_vector_loader(dc, table):
    """The same strided views as HOST arrays through build_batch: the batch packs every host tile dense at an aligned staging
    offset, so a full tile takes its type's row loader whatever its strides were and a padded one P1_V0; the bytes are the
    oracle's of the strided view."""
    L = table.L
    for dtype, cases in table.cases.items():
        picked = [c for c in cases if c.kind in ("sparse", "neg_fractions")]
        assert {c.view_name for c in picked} == {v[0] for v in E.views(L, dtype)}
        assert not any(c.round for c in picked)
        res = dc.build_batch([c.view for c in picked], fractional_bits=[c.bits for c in picked])
        bad = []
        for c, r in zip(picked, res):
            if isinstance(r, Exception):
                bad.append((c.name, repr(r)))
                continue
            padded = c.expected[0]
            if r.kernel != (L, padded, 0 if padded else E.LOADER[dtype], 0):
                bad.append((c.name, "kernel %s" % (r.kernel,)))
            if r.data.write_to() != c.ref.data or (r.snapshots, r.logs) != (c.ref.ns, c.ref.nl):
                bad.append((c.name, "bytes or counters differ from the oracle's"))
            if r.minmax.tobytes() != c.ref.mm.tobytes():
                bad.append((c.name, "minmax"))
            r.data.close()
        report(bad)


def test_float_errors_per_loader(dc, table):
    """Tiles the reference panics on (one precision loss, one infinity, one value beyond i64; one kind per tile) under the
    generic loader, the padded loader and the float row loaders, between good tiles of the same session: each reports the
    oracle's code, every good neighbour still matches the oracle, and the tile with a stored 2^30 + 1 comes back from the
    universal kernel with the oracle's bytes."""
    for dtype in (np.dtype(np.float32), np.dtype(np.float64)):
        queue = []
        for view in ("base_plus_1", "padded_subtile", "dense"):
            errs = [c for c in table.extras[(dtype, view)] if c.kind.startswith("error_")]
            good = [table.pick(dtype, view, k) for k in ("sparse", "nan_blocks", "neg_fractions", "round_ties")]
            assert [c.want_code for c in errs] == [E.ERR_PRECISION, E.ERR_NONFINITE, E.ERR_OVERFLOW]
            assert [c.ref.code for c in errs] == [c.want_code for c in errs]
            queue += [good[0], errs[0], good[1], errs[1], good[2], errs[2], good[3], table.pick(dtype, view, "edge29_over")]
        s = Session(queue)
        bad = [(c.name, p) for i, c in enumerate(queue) for p in s.problems(i)]
        kernels = {s.enc.tile_kernel(i)[1:3] for i in range(len(queue))}
        s.close()
        report(bad)
        assert kernels == {(0, 0), (1, 0), (0, E.LOADER[dtype])}


MIXED_CLASSES = [(np.int32, "dense"), (np.float32, "dense"), (np.int64, "subtile"), (np.float64, "subtile"),
                 (np.float64, "base_plus_1"), (np.float32, "padded_subtile"), (np.int32, "padded_subtile")]


def test_one_workgroup_encodes_a_mixed_queue(dc, table, monkeypatch):
    """The workgroups are persistent and pop tiles from a queue.  With K2R_MAX_WGS=1 a single workgroup encodes a queue of one
    class that alternates the extremes (wide, constant, all NaN, a failing tile, small, noise, ...): whatever a tile leaves in
    LDS, the error flag, the stash or the compact copy must not reach the next.  Every tile gives what it gives in a session
    with a workgroup per tile, and what the oracle gives."""
    L = table.L
    for dtype, view in MIXED_CLASSES:
        dtype = np.dtype(dtype)
        if E.is_float(dtype):
            ex = {c.kind: c for c in table.extras[(dtype, view)]}
            order = ["wide", "const", ex["all_nan"], ex["error_precision"], "small", "noise", "sparse", "nan_blocks",
                     ex["error_infinity"], "neg_fractions", "round_ties", "edge29", ex["error_beyond_i64"], "subnormal", "wide",
                     "edge29_over", "const"]
            queue = [table.pick(dtype, view, k) if isinstance(k, str) else k for k in order]
        else:
            other = "dense" if view != "dense" else "subtile"  # the same class (or, padded, the same kernel): more tiles
            other = padded_subtile_name(L)[:-len("_subtile")] if view == "padded_subtile" else other
            queue = []
            for k in ("wide", "const", "noise", "small", "sparse", "wide"):
                queue += [table.pick(dtype, view, k), table.pick(dtype, other, "const" if k == "wide" else "wide")]
        assert len(queue) >= 12
        monkeypatch.delenv("K2R_MAX_WGS", raising=False)
        s = Session(queue)
        alone = [s.outcome(i) for i in range(len(queue))]
        kernels = {s.enc.tile_kernel(i) for i in range(len(queue))}
        s.close()
        assert len(kernels) == 1, kernels  # one class: one launch, one queue
        monkeypatch.setenv("K2R_MAX_WGS", "1")
        s = Session(queue)
        bad = [(c.name, p) for i, c in enumerate(queue) for p in s.problems(i)]
        bad += [(c.name, "differs from the session with a workgroup per tile") for i, c in enumerate(queue) if s.outcome(i) != alone[i]]
        assert {s.enc.tile_kernel(i) for i in range(len(queue))} == kernels
        s.close()
        monkeypatch.delenv("K2R_MAX_WGS")
        report(bad)


def test_row_offset_limit_of_the_vector_loader(dc):
    """The row loaders address a row by a 32-bit byte offset inside its instant; the library takes them only while
    ((rows - 1) * stride_r + cols) * 8 < 2^31.  One 256 x 256 instant of int64 / float64 rows 8.4 MB apart in a 2.2 GB device
    buffer (only the rows are written): the largest even row stride below the limit takes V3 / V4, the next one that crosses
    it the generic loader, and both give the oracle's bytes."""
    from dcdf_amd.encoder import DeviceBuffer, Encoder
    S, esz = 256, 8
    below = (((1 << 31) // esz - 1 - S) // (S - 1)) & ~1  # even: a row stride of 16-byte multiples
    above = below + 2
    assert (below, above) == (1052686, 1052688)
    assert ((S - 1) * below + S) * esz < 1 << 31 <= ((S - 1) * above + S) * esz
    base_above = 4096  # (the rows of the two tiles interleave without touching: 32 * r + 4096 bytes apart)
    nbytes = 2_200_000_000
    assert base_above + ((S - 1) * above + S) * esz <= nbytes
    buf = DeviceBuffer(nbytes)
    try:
        for dtype in (np.int64, np.float64):
            rng = np.random.default_rng(62)
            tiles = []
            for kind in ("sparse", "wide"):
                a, bits, rnd = E.contents(kind, (1, S, S), dtype, rng)
                tiles.append((a, bits, rnd))
            descs, refs = [], []
            for (a, bits, rnd), (stride, base) in zip(tiles, ((below, 0), (above, base_above))):
                for r in range(S):
                    o = base + r * stride * esz
                    assert 0 <= o and o + S * esz <= nbytes
                    buf.write(o, a[0, r])
                descs.append((buf.ptr + base, code_of(dtype), (0, stride, 1), (1, S, S), bits, rnd))
                refs.append(O.chunk_build(a, fractional_bits=bits, round_=rnd))
            enc = Encoder(descs, k=2)
            enc.run()
            assert enc.tile_kernel(0) == (8, 0, E.LOADER[np.dtype(dtype)], 0)
            assert enc.tile_kernel(1) == (8, 0, 0, 0)
            for i in range(2):
                assert enc.result(i)[0] == 0
                assert enc.fetch(i) == refs[i], (np.dtype(dtype).name, i)
            enc.close()
    finally:
        buf.free()
