"""A tiled, time-segmented raster of encoded chunks: the callers either side of the chunk path, reduced to routing.

The reference cuts a [instants, rows, cols] variable into time segments of `chunk_size` instants
(`Variable::append`, dataset.rs:838; queried through `Span::fill_window` / `Span::search`, span.rs:183-275) and each
segment into `tile` x `tile` sub-arrays (`Superchunk::build`, superchunk.rs:127-181; queried through
`Superchunk::subchunks_for`, superchunk.rs:589-633).  Every (segment, tile row, tile col) is one `Chunk`.  This module
does that routing on the host -- vectorised over a whole batch of queries -- and sends the chunk-level sub-queries
through the batched C-ABI entry points (dcdf_query_fill_window_batch / dcdf_query_search_batch); the decoding itself is
on the GPU.  BASELINE configs[4] is exactly this with tile = 256, chunk_size = 32.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib as L
from .chunk import _ENC

# One leaf of a raster over stored Superchunks (dcdf_raster_tile): chunk = an opened dcdf_amd.Chunk, or None for an elided leaf
# whose value per instant is `values`; (row0, col0) = where the leaf starts inside its chunk; minmax = [instants, 2] stored
# (min, max) of the node tile that holds the leaf (or None); encoding / fractional_bits = the node's (of values and minmax);
# minmax_exact = minmax are exact values of the chunk's stored integers (value search may prune with them).
RasterTile = collections.namedtuple("RasterTile", "chunk row0 col0 values minmax encoding fractional_bits minmax_exact",
                                    defaults=(0, 0, None, None, L.DCDF_I64, 0, False))


class EncodedRaster:
    def __init__(self, shape, chunks, tile=256, chunk_size=32):
        """shape = (instants, rows, cols); chunks[(seg * nti + ti) * ntj + tj] = dcdf_amd.Chunk (opened or lazy)."""
        self.shape = tuple(int(x) for x in shape)
        self.tile, self.chunk_size = int(tile), int(chunk_size)
        self.nseg = -(-self.shape[0] // self.chunk_size)
        self.nti = -(-self.shape[1] // self.tile)
        self.ntj = -(-self.shape[2] // self.tile)
        if len(chunks) != self.nseg * self.nti * self.ntj:
            raise ValueError("expected %d chunks" % (self.nseg * self.nti * self.ntj))
        self.chunks = list(chunks)
        self.tiles = None  # from_tiles: the RasterTile of every leaf
        self._native = None

    @classmethod
    def from_tiles(cls, shape, tiles, tile, chunk_size):
        """A raster over stored Superchunks (dcdf_raster_create_tiles): tiles[(seg * nti + ti) * ntj + tj] = RasterTile, leaf size
        `tile`.  The native queries (fill_windows_flat, decode_flat, search_flat, search_values_flat, get_flat, fill_cells_flat) take it; the
        host-routed helpers (split and the methods built on it) refuse a raster with elided or offset leaves."""
        r = cls(shape, list(tiles), tile, chunk_size)
        r.tiles = [t if isinstance(t, RasterTile) else RasterTile(*t) for t in tiles]
        r.chunks = [t.chunk for t in r.tiles]
        r._handle()  # (bad tile tables fail here)
        return r

    # ---- the same routing natively (dcdf_raster_*: split in C++, every piece decoded into its place by one launch) ---------
    def _handle(self):
        if self._native is None:
            shp = (C.c_uint32 * 3)(*self.shape)
            h = C.c_void_p()
            if self.tiles is None:
                hs = (C.c_void_p * len(self.chunks))(*[c._h for c in self.chunks])
                L.check(L.lib().dcdf_raster_create(hs, C.c_size_t(len(self.chunks)), shp, self.tile, self.chunk_size, C.byref(h)), "raster_create")
            else:
                desc = (L.RasterTile * len(self.tiles))()
                keep = []  # (values and minmax are copied by the call)
                for d, t in zip(desc, self.tiles):
                    d.chunk = t.chunk._h if t.chunk is not None else None
                    d.row0, d.col0 = int(t.row0), int(t.col0)
                    for name in ("values", "minmax"):
                        a = getattr(t, name)
                        if a is not None:
                            a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
                            keep.append(a)
                            setattr(d, name, a.ctypes.data)
                    d.encoding, d.fractional_bits, d.minmax_exact = int(t.encoding), int(t.fractional_bits), 1 if t.minmax_exact else 0
                L.check(L.lib().dcdf_raster_create_tiles(desc, C.c_size_t(len(desc)), shp, self.tile, self.chunk_size, C.byref(h)),
                        "raster_create_tiles")
            self._native = h
        return self._native

    def close(self):
        if getattr(self, "_native", None):
            L.lib().dcdf_raster_destroy(self._native)
            self._native = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the region calls (dcdf_raster_*_batch over whole cubes) ----------------------------------------------------------------
    @staticmethod
    def _cubes(cubes):
        return np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))

    @staticmethod
    def _extent(q, lo):
        """|q[:, lo + 1] - q[:, lo]| as int64 (reversed bounds are reordered, geom.rs:83-103)"""
        return np.abs(q[:, lo + 1].astype(np.int64) - q[:, lo])

    def _region_call(self, name, q, counts, dtype, args, zeroed=False, stats=True, out_device_ptr=None, out_offset=None):
        """dcdf_raster_<name>_batch over the cubes q, in either form.  Host form (out_device_ptr None): cube i gets counts()[i]
        elements of dtype, one cube after the other; returns (flat array, offsets uint64[n], kernel ms, stats).  Device form: the
        caller's out_offset; returns (kernel ms, stats).  args(n, out, mem, off, stats): the call's arguments between the cubes and
        the kernel ms, in its own order.  stats = False: the call has none, and none is returned."""
        ms = C.c_float()
        st = np.zeros(3, dtype=np.uint64) if stats else None
        if out_device_ptr is None:
            vol = counts().astype(np.uint64)
            off = np.zeros(len(q), dtype=np.uint64)
            if len(q) > 1:
                off[1:] = np.cumsum(vol)[:-1]
            out = (np.zeros if zeroed else np.empty)(max(1, int(vol.sum())), dtype=dtype)
            ptr, mem = out.ctypes.data, L.MEM_HOST
        else:
            off = np.ascontiguousarray(np.asarray(out_offset, dtype=np.uint64))
            out, ptr, mem = None, out_device_ptr, L.MEM_DEVICE
        entry = "raster_%s_batch" % name
        own = args(C.c_size_t(len(q)), C.c_void_p(ptr), mem, C.c_void_p(off.ctypes.data), None if st is None else C.c_void_p(st.ctypes.data))
        L.check(getattr(L.lib(), "dcdf_" + entry)(self._handle(), C.c_void_p(q.ctypes.data), *own, C.byref(ms)), entry)
        tail = (ms.value,) if st is None else (ms.value, st)
        return tail if out is None else (out, off) + tail

    def _window_args(self, start, stop, window):
        """(start, stop, top, bottom, left, right) of a whole-raster method: stop defaults to the last instant, window = (top,
        bottom, left, right) to all cells; both inside the raster."""
        T, R, Cc = self.shape
        stop = T if stop is None else int(stop)
        start = int(start)
        if not 0 <= start <= stop <= T:
            raise ValueError("instants [%d, %d) outside [0, %d)" % (start, stop, T))
        top, bottom, left, right = (0, R, 0, Cc) if window is None else (int(x) for x in window)
        if not (0 <= top <= bottom <= R and 0 <= left <= right <= Cc):
            raise ValueError("window (%d:%d, %d:%d) outside the raster's %d x %d cells" % (top, bottom, left, right, R, Cc))
        return start, stop, top, bottom, left, right

    def fill_windows_flat(self, cubes, dtype=np.int64, out_device_ptr=None, out_offset=None):
        """fill_window of dataset-level cubes [n, 6] through dcdf_raster_fill_window_batch.  Host form: returns (flat array of
        dtype, offsets uint64[n], kernel ms): window q is flat[offsets[q]:] shaped (t, r, c).  Device form (out_device_ptr +
        out_offset in elements): the windows are written there, returns kernel ms."""
        q = self._cubes(cubes)
        dtype = np.dtype(dtype)
        res = self._region_call("fill_window", q, lambda: self._extent(q, 0) * self._extent(q, 2) * self._extent(q, 4), dtype,
                                lambda n, out, mem, off, stats: (n, out, _ENC[dtype], mem, off), stats=False, out_device_ptr=out_device_ptr,
                                out_offset=out_offset)
        return res[0] if out_device_ptr is not None else res

    def decode_flat(self, cubes, dtype=np.int64, out_device_ptr=None, out_offset=None):
        """Decompress dataset-level cubes [n, 6] through dcdf_raster_decode_batch: the values fill_windows_flat returns, bit for
        bit, decoded block by block (meant for whole tiles and long time ranges).  Host form: returns (flat array of dtype,
        offsets uint64[n], kernel ms, stats); device form (out_device_ptr + out_offset in elements): returns (kernel ms, stats).
        stats = uint64[3]: cells written by the bulk kernel, by the fallback walk, by the elided fill."""
        q = self._cubes(cubes)
        dtype = np.dtype(dtype)
        return self._region_call("decode", q, lambda: self._extent(q, 0) * self._extent(q, 2) * self._extent(q, 4), dtype,
                                 lambda n, out, mem, off, stats: (n, out, _ENC[dtype], mem, off, stats), out_device_ptr=out_device_ptr,
                                 out_offset=out_offset)

    def decode(self, start=0, stop=None, dtype=np.int64):
        """The instants [start, stop) of the whole raster, decompressed: ndarray [stop - start, rows, cols] of dtype."""
        start, stop, _, R, _, Cc = self._window_args(start, stop, None)
        if start == stop:
            return np.empty((0, R, Cc), dtype=np.dtype(dtype))
        out, _, _, _ = self.decode_flat([[start, stop, 0, R, 0, Cc]], dtype)
        return out[:(stop - start) * R * Cc].reshape(stop - start, R, Cc)

    # ---- the region statistics: what each one is stands once, in its description below this class; these are the drivers ---------
    def _flat(self, S, cubes, *arrays, out_device_ptr=None, out_offset=None):
        """The flat form of every region statistic.  S: its description, holding the call's own arguments; arrays: what it takes
        per cube (labels, masks, bounds), staged against the cubes by S.flat.  Returns what _region_call returns, in either form."""
        q = S.flat(cubes, *arrays)
        return self._region_call(S.name, q, lambda: S.count(q), S.dtype, S.args, zeroed=S.zeroed, out_device_ptr=out_device_ptr,
                                 out_offset=out_offset)

    def _whole(self, stat, own, arrays, start, stop, window):
        """The whole-raster form of every region statistic: the instants and the window (_window_args), the statistic's own
        arguments (stat(*own)), its arrays against the window (window()); then its fill where there is nothing to read -- no
        instant, or for a statistic over time no cell --, else the flat form over one cube, cut into the result's arrays."""
        start, stop, top, bottom, left, right = self._window_args(start, stop, window)
        S = stat(*own)
        nt, rows, cols = stop - start, bottom - top, right - left
        arrays = S.window(nt, rows, cols, *arrays)
        shape = S.shape(nt, rows, cols)
        if nt == 0 or (S.over_time and rows * cols == 0):
            return S.nothing(shape)
        return S.cut(self._flat(S, [[start, stop, top, bottom, left, right]], *arrays)[0], shape)

    @staticmethod
    def _ops(ops, table, what):
        """reduce_ops / spell_ops over their table of {name: bit}"""
        if isinstance(ops, (int, np.integer)):
            mask = int(ops)
        else:
            mask = 0
            for name in ([ops] if isinstance(ops, str) else ops):
                if name not in table:
                    raise ValueError("%s: unknown statistic %r (one of %s)" % (what, name, ", ".join(table)))
                mask |= table[name]
        if not 0 < mask < 32:
            raise ValueError("%s: ops %r is not a set of %s" % (what, ops, ", ".join(table)))
        return mask, [n for n, b in table.items() if mask & b]

    @staticmethod
    def reduce_ops(ops):
        """ops of reduce_time / reduce_time_flat as (bitmask, names in plane order): a DCDF_REDUCE_* bitmask, one name or an
        iterable of "min" / "max" / "sum" / "count" / "mean"."""
        return EncodedRaster._ops(ops, L.REDUCE_OPS, "reduce_time")

    def reduce_time_flat(self, cubes, ops, out_device_ptr=None, out_offset=None):
        """Per-cell statistics over time of dataset-level cubes [n, 6] through dcdf_raster_reduce_time_batch: cube q yields one
        [rows, cols] float64 plane per statistic of `ops` (reduce_ops), in the order min, max, sum, count, mean, over the values
        decode_flat returns for it in the leaves' own dtype; the sum is sequential in instant order.  Host form: returns (flat
        float64 array, offsets uint64[n], kernel ms, stats): cube q's planes are flat[offsets[q]:] shaped (planes, r, c).  Device
        form (out_device_ptr + out_offset in elements): returns (kernel ms, stats).  stats = uint64[3]: cells read by the bulk
        kernel, by the fallback walk, from elided leaves."""
        return self._flat(_ReduceTime(ops), cubes, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def reduce_time(self, ops, start=0, stop=None, window=None):
        """{statistic: ndarray [rows, cols] float64} over the instants [start, stop) of the whole raster, or of `window` =
        (top, bottom, left, right).  Without instants: NaN planes, count 0 and sum 0."""
        return self._whole(_ReduceTime, (ops,), (), start, stop, window)

    def reduce_time_groups_flat(self, cubes, ops, labels, n_groups, out_device_ptr=None, out_offset=None):
        """reduce_time_flat's statistics per cell and group of instants, of dataset-level cubes [n, 6] through
        dcdf_raster_reduce_time_groups_batch: one walk of the encoded bytes whatever the number of groups.  labels: one uint16 array
        [instants] per (normalised) cube -- instant i, counted from the cube's first, belongs to group labels[i] when that is <
        n_groups; GROUP_NONE (0xffff) and every other value >= n_groups belong to no group.  Cube q yields one [n_groups, rows, cols]
        float64 array per statistic of `ops` (reduce_ops), in the order min, max, sum, count, mean: group g is reduce_time of the
        instants labelled g, the sum sequential in instant order; a group without a non-NaN value gets NaN, NaN, +0.0, 0, NaN.  Host
        form: returns (flat float64 array, offsets uint64[n], kernel ms, stats): cube q's part is flat[offsets[q]:] shaped
        (statistics, n_groups, r, c).  Device form (out_device_ptr + out_offset in elements): returns (kernel ms, stats).  stats =
        uint64[3]: cells read by the bulk kernel, by the fallback walk, from elided leaves."""
        return self._flat(_ReduceTimeGroups(ops), cubes, labels, n_groups, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def reduce_time_groups(self, ops, labels, start=0, stop=None, window=None, n_groups=None):
        """{statistic: ndarray [n_groups, rows, cols] float64}: reduce_time over the instants [start, stop) of the whole raster, or
        of `window` = (top, bottom, left, right), separately for every group of `labels` -- uint16 [stop - start], GROUP_NONE and
        labels >= n_groups are in no group.  n_groups defaults to the largest label present, GROUP_NONE apart, plus 1 (at least
        1).  Without instants or cells: NaN planes, count 0 and sum 0, of that shape."""
        return self._whole(_ReduceTimeGroups, (ops,), (labels, n_groups), start, stop, window)

    @staticmethod
    def moment_ops(ops):
        """ops of moments_time / moments_time_groups as (bitmask, names in plane order): a DCDF_MOMENT_* bitmask, one name or an
        iterable of "count" / "mean" / "var" / "std"."""
        mask, names = EncodedRaster._ops(ops, L.MOMENT_OPS, "moments_time")
        if mask >= 16:
            raise ValueError("moments_time: ops %r is not a set of %s" % (ops, ", ".join(L.MOMENT_OPS)))
        return mask, names

    def moments_time_flat(self, cubes, ops, ddof=0, out_device_ptr=None, out_offset=None):
        """Per-cell count, mean, variance and standard deviation over time of dataset-level cubes [n, 6] through
        dcdf_raster_moments_time_batch: cube q yields one [rows, cols] float64 plane per statistic of `ops` (moment_ops), in the
        order count, mean, var, std, over the values decode_flat returns for it in the leaves' own dtype, NaN skipped.  The sums
        are taken of x - K, K the cell's first value, sequentially in instant order (include/dcdf_k2r.h): mean = K + s1 / count,
        var = (s2 - s1 * s1 / count) / (count - ddof), std = sqrt(var) correctly rounded; ddof is 0 or 1.  A cell without a value
        gets 0, NaN, NaN, NaN; a constant cell has var exactly 0.  Host form: returns (flat float64 array, offsets uint64[n],
        kernel ms, stats): cube q's planes are flat[offsets[q]:] shaped (planes, r, c).  Device form (out_device_ptr + out_offset
        in elements): returns (kernel ms, stats).  stats = uint64[3]: cells read by the bulk kernel, by the fallback walk, from
        elided leaves."""
        return self._flat(_MomentsTime(ops, ddof), cubes, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def moments_time(self, ops=("mean", "std"), start=0, stop=None, window=None, ddof=0):
        """{statistic: ndarray [rows, cols] float64} of moments_time_flat over the instants [start, stop) of the whole raster, or
        of `window` = (top, bottom, left, right).  Without instants or cells: count 0, NaN elsewhere."""
        return self._whole(_MomentsTime, (ops, ddof), (), start, stop, window)

    def moments_time_groups_flat(self, cubes, ops, labels, n_groups, ddof=0, out_device_ptr=None, out_offset=None):
        """moments_time_flat's statistics per cell and group of instants through dcdf_raster_moments_time_groups_batch: one walk of
        the encoded bytes whatever the number of groups.  labels and n_groups are reduce_time_groups_flat's: one uint16 array
        [instants] per (normalised) cube, GROUP_NONE (0xffff) and every other value >= n_groups in no group.  Cube q yields one
        [n_groups, rows, cols] float64 array per statistic of `ops`, in the order count, mean, var, std: group g is moments_time of
        the instants labelled g, in order (its K is the group's first value); a group without a value gets 0, NaN, NaN, NaN.
        Returns what moments_time_flat returns, cube q's part shaped (statistics, n_groups, r, c)."""
        return self._flat(_MomentsTimeGroups(ops, ddof), cubes, labels, n_groups, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def moments_time_groups(self, ops, labels, start=0, stop=None, window=None, n_groups=None, ddof=0):
        """{statistic: ndarray [n_groups, rows, cols] float64}: moments_time over the instants [start, stop) of the whole raster, or
        of `window`, separately for every group of `labels` -- uint16 [stop - start], GROUP_NONE and labels >= n_groups are in no
        group.  n_groups defaults to the largest label present, GROUP_NONE apart, plus 1 (at least 1).  With one group and all
        labels 0 it is moments_time bit for bit.  Without instants or cells: count 0, NaN elsewhere, of that shape."""
        return self._whole(_MomentsTimeGroups, (ops, ddof), (labels, n_groups), start, stop, window)

    @staticmethod
    def spell_ops(ops):
        """ops of spells / spells_flat as (bitmask, names in plane order): a DCDF_SPELL_* bitmask, one name or an iterable of
        "count" / "longest" / "longest_start" / "first" / "last"."""
        return EncodedRaster._ops(ops, L.SPELL_OPS, "spells")

    def spells_flat(self, cubes, lower, upper, ops, out_device_ptr=None, out_offset=None):
        """Per-cell spell statistics of dataset-level cubes [n, 6] through dcdf_raster_spells_batch: instant i of a cell (counted
        from the cube's first) is a hit when its value lies in [lower[q], upper[q]] by value search's rule (search_values_flat:
        NaN never hits, integer leaves compare exactly, +-inf is unbounded); cube q yields one [rows, cols] uint32 plane per
        statistic of `ops` (spell_ops), in the order count, longest, longest_start, first, last; SPELL_NONE where there is no hit.
        lower / upper: one value per cube, or a scalar for all.  Host form: returns (flat uint32 array, offsets uint64[n], kernel
        ms, stats): cube q's planes are flat[offsets[q]:] shaped (planes, r, c).  Device form (out_device_ptr + out_offset in
        elements): returns (kernel ms, stats).  stats = uint64[3]: cells read by the bulk kernel, by the fallback walk, from elided
        leaves."""
        return self._flat(_Spells(ops), cubes, lower, upper, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def spells(self, lower, upper, ops=("count", "longest"), start=0, stop=None, window=None):
        """{statistic: ndarray [rows, cols] uint32} of the hits of [lower, upper] over the instants [start, stop) of the whole
        raster, or of `window` = (top, bottom, left, right); instants are counted from `start`.  Without instants: zeros for count
        and longest, SPELL_NONE for the others."""
        return self._whole(_Spells, (ops,), (lower, upper), start, stop, window)

    def quantile_time_flat(self, cubes, probs, method="linear", out_device_ptr=None, out_offset=None):
        """Per-cell quantiles over time of dataset-level cubes [n, 6] through dcdf_raster_quantile_time_batch: cube q yields one
        [rows, cols] float64 plane per probability of `probs` (1 .. 16 values in [0, 1], shared by all cubes), in their order, over
        the values decode_flat returns for it in the leaves' own dtype, NaN skipped: with v the n sorted values of a cell and
        h = (n - 1) * p, "lower" is v[floor(h)], "higher" v[ceil(h)], "nearest" the nearer of the two (the even index at a tie) and
        "linear" the interpolation numpy.nanquantile makes; NaN where n == 0.  The result is exact: the order statistics are selected
        on the device.  Host form: returns (flat float64 array, offsets uint64[n], kernel ms, stats): cube q's planes are
        flat[offsets[q]:] shaped (planes, r, c).  Device form (out_device_ptr + out_offset in elements): returns (kernel ms,
        stats).  stats = uint64[3]: cells read by the bulk kernel, by the fallback walk, from elided leaves."""
        return self._flat(_QuantileTime(probs, method), cubes, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def quantile_time(self, probs, start=0, stop=None, window=None, method="linear"):
        """ndarray [n_probs, rows, cols] float64 ([rows, cols] for a scalar `probs`): the quantiles of every cell's series over the
        instants [start, stop) of the whole raster, or of `window` = (top, bottom, left, right) (quantile_time_flat's rule).  Without
        instants or cells: NaN planes of that shape."""
        return self._whole(_QuantileTime, (probs, method), (), start, stop, window)

    @staticmethod
    def regress_ops(ops):
        """ops of regress_time / regress_time_groups as (bitmask, names in plane order): a DCDF_REGRESS_* bitmask, one name or an
        iterable of "count" / "slope" / "intercept" / "corr"."""
        mask, names = EncodedRaster._ops(ops, L.REGRESS_OPS, "regress_time")
        if mask >= 16:
            raise ValueError("regress_time: ops %r is not a set of %s" % (ops, ", ".join(L.REGRESS_OPS)))
        return mask, names

    def regress_time_flat(self, cubes, ops, regressors=None, out_device_ptr=None, out_offset=None):
        """Per-cell least-squares line over time of dataset-level cubes [n, 6] through dcdf_raster_regress_time_batch: cube q yields
        one [rows, cols] float64 plane per statistic of `ops` (regress_ops), in the order count, slope, intercept, corr, of the
        values decode_flat returns for it in the leaves' own dtype, NaN skipped, against a per-instant regressor.  regressors: None
        -- the instant index counted from each cube's first instant, 0, 1, 2, ... -- or one float64 array [instants] per
        (normalised) cube, finite.  It enters AS GIVEN (include/dcdf_k2r.h): intercept is the fitted value where the regressor is 0,
        and the sums keep their accuracy only for a regressor near zero, so subtract a far-off regressor's first value before the
        call (regress_time does).  The sums are taken of x - K, K the cell's first value, sequentially in instant order; a cell
        with fewer than two values, or whose regressor values are all equal, gets NaN but for count; a constant cell has slope
        exactly 0, intercept its value and corr NaN.  Host form: returns (flat float64 array, offsets uint64[n], kernel ms, stats):
        cube q's planes are flat[offsets[q]:] shaped (planes, r, c).  Device form (out_device_ptr + out_offset in elements):
        returns (kernel ms, stats).  stats = uint64[3]: cells read by the bulk kernel, by the fallback walk, from elided leaves."""
        return self._flat(_RegressTime(ops), cubes, regressors, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def regress_time(self, ops=("slope",), regressor=None, start=0, stop=None, window=None):
        """{statistic: ndarray [rows, cols] float64} of regress_time_flat over the instants [start, stop) of the whole raster, or of
        `window` = (top, bottom, left, right) -- a trend map with regressor=None (per instant), the regression on / correlation
        with an index series otherwise: `regressor` is float64 [stop - start], finite.  What is passed on is regressor -
        regressor[0], so `intercept` is the fitted value at the first instant of [start, stop), whatever the regressor's own zero
        (years, time stamps); for the instant index this changes nothing.  Without instants or cells: count 0, NaN elsewhere."""
        return self._whole(_RegressTime, (ops,), (regressor,), start, stop, window)

    def regress_time_groups_flat(self, cubes, ops, labels, n_groups, regressors=None, out_device_ptr=None, out_offset=None):
        """regress_time_flat's statistics per cell and group of instants through dcdf_raster_regress_time_groups_batch: the cube is
        decoded once whatever the number of groups.  labels and n_groups are reduce_time_groups_flat's: one uint16 array [instants]
        per (normalised) cube, GROUP_NONE (0xffff) and every other value >= n_groups in no group; regressors regress_time_flat's,
        as given.  Cube q yields one [n_groups, rows, cols] float64 array per statistic of `ops`, in the order count, slope,
        intercept, corr: group g is regress_time_flat of the instants labelled g, in order, each with its own regressor value; a
        group without a value gets 0, NaN, NaN, NaN.  Returns what regress_time_flat returns, cube q's part shaped (statistics,
        n_groups, r, c)."""
        return self._flat(_RegressTimeGroups(ops), cubes, labels, n_groups, regressors, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def regress_time_groups(self, ops, labels, regressor=None, start=0, stop=None, window=None, n_groups=None):
        """{statistic: ndarray [n_groups, rows, cols] float64}: regress_time over the instants [start, stop) of the whole raster, or
        of `window`, separately for every group of `labels` -- uint16 [stop - start], GROUP_NONE and labels >= n_groups are in no
        group; a trend per season, say.  n_groups defaults to the largest label present, GROUP_NONE apart, plus 1 (at least 1).
        What is passed on is regressor - regressor[0] for every group alike, so `intercept` is the group's fitted value at the first
        instant of [start, stop); for the instant index (None) this changes nothing.  With one group and all labels 0 it is
        regress_time bit for bit.  Without instants or cells: count 0, NaN elsewhere, of that shape."""
        return self._whole(_RegressTimeGroups, (ops,), (labels, n_groups, regressor), start, stop, window)

    @staticmethod
    def rolling_ops(ops):
        """ops of rolling_time / rolling_time_groups as (bitmask, names in plane order): a DCDF_ROLLING_* bitmask, one name or an
        iterable of "max" / "argmax" / "min" / "argmin" / "count"."""
        return EncodedRaster._ops(ops, L.ROLLING_OPS, "rolling_time")

    def rolling_time_flat(self, cubes, ops, window, min_count=None, mean=False, out_device_ptr=None, out_offset=None):
        """Per-cell extremes of the sums of every `window` consecutive instants of dataset-level cubes [n, 6] through
        dcdf_raster_rolling_time_batch: cube q yields one [rows, cols] float64 plane per statistic of `ops` (rolling_ops), in the
        order max, argmax, min, argmin, count, over the values decode_flat returns for it in the leaves' own dtype.  The window
        that ENDS at instant i, counted from the cube's first, covers [i - window + 1, i] and exists for i >= window - 1; it is valid
        when it holds at least min_count (None: window) values that are not NaN, and its sum is their EXACT sum.  max / min: the
        greatest / least sum over the valid windows, rounded once; mean=True: divided by window (min_count must then be window).
        argmax / argmin: the last instant of the earliest window whose exact sum is the greatest / least -- sums that only round to
        the same double are no tie.  count: the valid windows.  A cell without one gets NaN, NaN, NaN, NaN, 0.  Host form: returns
        (flat float64 array, offsets uint64[n], kernel ms, stats): cube q's planes are flat[offsets[q]:] shaped (planes, r, c).
        Device form (out_device_ptr + out_offset in elements): returns (kernel ms, stats).  stats = uint64[3]: cells read by the
        bulk kernel, by the fallback walk, from elided leaves."""
        return self._flat(_RollingTime(ops, window, min_count, mean), cubes, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def rolling_time(self, ops, window, min_count=None, mean=False, start=0, stop=None, region=None):
        """{statistic: ndarray [rows, cols] float64} of rolling_time_flat over the instants [start, stop) of the whole raster, or of
        `region` = (top, bottom, left, right) -- `window` is the number of instants a sum takes, 1 .. 65535: the greatest 5-day
        total and the instant it ended on are rolling_time(("max", "argmax"), 5), the lowest 7-day mean rolling_time("min", 7,
        mean=True).  Instants are counted from `start`, whose first window - 1 instants end no window: pass an earlier start for
        windows that reach back.  Without instants or cells: count 0, NaN elsewhere."""
        return self._whole(_RollingTime, (ops, window, min_count, mean), (), start, stop, region)

    def rolling_time_groups_flat(self, cubes, ops, labels, n_groups, window, min_count=None, mean=False, out_device_ptr=None, out_offset=None):
        """rolling_time_flat's statistics per cell and group of instants through dcdf_raster_rolling_time_groups_batch: the cube is
        decoded once whatever the number of groups.  labels and n_groups are reduce_time_groups_flat's: one uint16 array [instants]
        per (normalised) cube, GROUP_NONE (0xffff) and every other value >= n_groups in no group.  A window belongs to the group of
        its LAST instant and reaches back over instants of any label or none (the wettest five days of a year may begin in the
        previous December).  Cube q yields one [n_groups, rows, cols] float64 array per statistic of `ops`, in the order max,
        argmax, min, argmin, count: group g is the fold over the valid windows whose last instant is labelled g, argmax / argmin
        still counted from the cube's first instant; a group without a valid window gets NaN, NaN, NaN, NaN, 0.  Consecutive
        instants of a group slide the window; every other window is summed again from its `window` values, so a scattered
        labelling (i % 7) reads that many values per window.  Returns what rolling_time_flat returns, cube q's part shaped
        (statistics, n_groups, r, c)."""
        return self._flat(_RollingTimeGroups(ops, window, min_count, mean), cubes, labels, n_groups, out_device_ptr=out_device_ptr,
                          out_offset=out_offset)

    def rolling_time_groups(self, ops, labels, window, min_count=None, mean=False, start=0, stop=None, region=None, n_groups=None):
        """{statistic: ndarray [n_groups, rows, cols] float64}: rolling_time over the instants [start, stop) of the whole raster, or
        of `region`, for every group of `labels` -- uint16 [stop - start], GROUP_NONE and labels >= n_groups are in no group; a
        window belongs to the group of its last instant: Rx5day per year, say.  n_groups defaults to the largest label present,
        GROUP_NONE apart, plus 1 (at least 1).  With one group and all labels 0 it is rolling_time bit for bit.  Without instants
        or cells: count 0, NaN elsewhere, of that shape."""
        return self._whole(_RollingTimeGroups, (ops, window, min_count, mean), (labels, n_groups), start, stop, region)

    @staticmethod
    def _device_arrays(q, arrays, what, noun):
        """One array per cube (masks, labels) already on the device, given as (device pointer, offsets uint64[n]): (pointer, offsets,
        memory kind, what must stay alive over the call); None when `arrays` is not of that form."""
        if not (isinstance(arrays, tuple) and len(arrays) == 2 and isinstance(arrays[0], (int, np.integer))):
            return None
        keep = np.ascontiguousarray(np.asarray(arrays[1], dtype=np.uint64))
        if keep.shape != (len(q),):
            raise ValueError("%s: %d %s offsets for %d cubes" % (what, keep.size, noun, len(q)))
        return C.c_void_p(int(arrays[0])), C.c_void_p(keep.ctypes.data), L.MEM_DEVICE, keep

    @staticmethod
    def _host_arrays(parts, dtype):
        """The same for host arrays: the cubes' flat parts one after the other, one spare element behind them."""
        off = np.zeros(len(parts), dtype=np.uint64)
        if len(parts) > 1:
            off[1:] = np.cumsum([p.size for p in parts])[:-1]
        flat = np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, dtype=dtype)]))
        return C.c_void_p(flat.ctypes.data), C.c_void_p(off.ctypes.data), L.MEM_HOST, (flat, off)

    @staticmethod
    def _mask_args(q, masks, what):
        """The mask arguments of dcdf_raster_reduce_space_batch / dcdf_raster_histogram_batch for the cubes q: (pointer, offsets,
        memory kind, what must stay alive over the call).  masks as reduce_space_flat documents them."""
        dev = EncodedRaster._device_arrays(q, masks, what, "mask")
        if dev is not None:
            return dev
        if masks is not None:
            masks = list(masks)
            if len(masks) != len(q):
                raise ValueError("%s: %d masks for %d cubes" % (what, len(masks), len(q)))
            if any(m is not None for m in masks):
                rows, cols = EncodedRaster._extent(q, 2), EncodedRaster._extent(q, 4)
                parts = []
                for i, m in enumerate(masks):
                    shape = (int(rows[i]), int(cols[i]))
                    if m is None:
                        parts.append(np.ones(shape[0] * shape[1], dtype=np.uint8))
                        continue
                    m = np.asarray(m)
                    if m.shape != shape:
                        raise ValueError("%s: mask %d has shape %r, its cube %r" % (what, i, m.shape, shape))
                    parts.append((m != 0).astype(np.uint8).ravel())
                return EncodedRaster._host_arrays(parts, np.uint8)
        return None, None, L.MEM_HOST, None

    def reduce_space_flat(self, cubes, ops, masks=None, out_device_ptr=None, out_offset=None):
        """Per-instant statistics over the selected cells of dataset-level cubes [n, 6] through dcdf_raster_reduce_space_batch: cube
        q yields one [instants] float64 series per statistic of `ops` (reduce_ops), in the order min, max, sum, count, mean, over
        the values decode_flat returns for it in the leaves' own dtype; the sum is exact, rounded once (math.fsum).  masks: None,
        or one entry per cube -- a boolean / uint8 array [rows, cols] of the (normalised) cube whose non-zero cells are selected,
        or None for all cells -- or (device pointer, offsets uint64[n] in bytes) of masks already on the device.  Host form:
        returns (flat float64 array, offsets uint64[n], kernel ms, stats): cube q's series are flat[offsets[q]:] shaped (series,
        instants).  Device form (out_device_ptr + out_offset in elements): returns (kernel ms, stats).  stats = uint64[3]: cells
        read by the bulk kernel, by the fallback walk, from elided leaves."""
        return self._flat(_ReduceSpace(ops), cubes, masks, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def reduce_space(self, ops, start=0, stop=None, window=None, mask=None):
        """{statistic: ndarray [stop - start] float64} over the cells of the whole raster, or of `window` = (top, bottom, left,
        right), at every instant of [start, stop); mask: [rows, cols] of the window, non-zero = the cell is selected.  Without
        instants: empty arrays."""
        return self._whole(_ReduceSpace, (ops,), (mask,), start, stop, window)

    @staticmethod
    def _label_args(q, labels, what):
        """The label arguments of dcdf_raster_zonal_batch for the cubes q: (pointer, offsets, memory kind, what must stay alive over
        the call, the largest label below ZONE_NONE or -1 when unknown).  labels as zonal_flat documents them."""
        dev = EncodedRaster._device_arrays(q, labels, what, "label")
        if dev is not None:
            return dev + (-1,)
        labels = list(labels)
        if len(labels) != len(q):
            raise ValueError("%s: %d label arrays for %d cubes" % (what, len(labels), len(q)))
        rows, cols = EncodedRaster._extent(q, 2), EncodedRaster._extent(q, 4)
        parts = []
        for i, m in enumerate(labels):
            m = np.asarray(m)
            if m.dtype != np.uint16:
                raise ValueError("%s: labels %d are %s, not uint16" % (what, i, m.dtype))
            if m.shape != (int(rows[i]), int(cols[i])):
                raise ValueError("%s: labels %d have shape %r, their cube %r" % (what, i, m.shape, (int(rows[i]), int(cols[i]))))
            parts.append(m.ravel())
        host = EncodedRaster._host_arrays(parts, np.uint16)
        flat = host[3][0]
        named = flat[:-1][flat[:-1] != L.ZONE_NONE]
        return host + (int(named.max()) if named.size else -1,)

    def zonal_flat(self, cubes, ops, labels, n_zones, out_device_ptr=None, out_offset=None):
        """Zonal statistics of dataset-level cubes [n, 6] through dcdf_raster_zonal_batch: reduce_space_flat's statistics for every
        zone of a label raster at once, from one walk of the encoded bytes.  labels: one uint16 array [rows, cols] per (normalised)
        cube -- cell (r, c) belongs to zone labels[r, c] when that is < n_zones; ZONE_NONE (0xffff) and every other value >= n_zones
        belong to no zone -- or (device pointer, offsets uint64[n] in elements) of label arrays already on the device.  Cube q
        yields one [n_zones, instants] float64 matrix per statistic of `ops` (reduce_ops), in the order min, max, sum, count, mean;
        a zone without a non-NaN cell gets NaN, NaN, +0.0, 0, NaN.  Host form: returns (flat float64 array, offsets uint64[n], kernel
        ms, stats): cube q's part is flat[offsets[q]:] shaped (series, n_zones, instants).  Device form (out_device_ptr + out_offset
        in elements): returns (kernel ms, stats).  stats = uint64[3]: cells read by the bulk kernel, by the fallback walk, from elided
        leaves."""
        return self._flat(_Zonal(ops), cubes, labels, n_zones, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def zonal(self, ops, labels, start=0, stop=None, window=None, n_zones=None):
        """{statistic: ndarray [n_zones, stop - start] float64} per zone of `labels` -- uint16 [rows, cols] of the whole raster, or
        of `window` = (top, bottom, left, right); ZONE_NONE and labels >= n_zones are in no zone -- at every instant of [start,
        stop).  n_zones defaults to the largest label present, ZONE_NONE apart, plus 1 (at least 1).  Without instants: empty
        matrices."""
        return self._whole(_Zonal, (ops,), (labels, n_zones), start, stop, window)

    def histogram_flat(self, cubes, edges, masks=None, out_device_ptr=None, out_offset=None):
        """Per-instant value histograms over the selected cells of dataset-level cubes [n, 6] through dcdf_raster_histogram_batch:
        cube q yields a dense [instants, bins] uint64 array of counts over the values decode_flat returns for it in the leaves' own
        dtype, widened to float64 -- edges[b] <= x < edges[b + 1], the last bin closed (numpy.histogram's rule), NaN and values
        outside the edges counted nowhere.  edges: bins + 1 increasing values shared by all cubes.  masks: as reduce_space_flat.
        Host form: returns (flat uint64 array, offsets uint64[n], kernel ms, stats): cube q is flat[offsets[q]:] shaped (instants,
        bins).  Device form (out_device_ptr + out_offset in elements): returns (kernel ms, stats).  stats = uint64[3]: cells read by
        the bulk kernel, by the fallback walk, from elided leaves."""
        return self._flat(_Histogram(edges), cubes, masks, out_device_ptr=out_device_ptr, out_offset=out_offset)

    def histogram(self, edges, start=0, stop=None, window=None, mask=None):
        """ndarray [stop - start, bins] uint64: per instant of [start, stop), how many cells of the whole raster, or of `window` =
        (top, bottom, left, right), fall into every bin of `edges` (histogram_flat's rule); mask: [rows, cols] of the window,
        non-zero = the cell is selected.  Without instants: shape (0, bins)."""
        return self._whole(_Histogram, (edges,), (mask,), start, stop, window)

    def _search(self, entry, cubes, bounds, out_device_ptr, cap):
        """dcdf_<entry> over the cubes [n, 6]; bounds(n) = the (lower, upper) arrays of the entry's type.  Returns (triples uint32[hits,
        3] in raster coordinates -- or None when they stay on the device --, offsets, counts, kernel ms)."""
        q = self._cubes(cubes)
        lo, hi = (np.ascontiguousarray(b) for b in bounds(len(q)))
        counts = np.zeros(len(q), dtype=np.uint64)
        offs = np.zeros(len(q), dtype=np.uint64)
        if cap is None:
            cap = int((self._extent(q, 0) * self._extent(q, 2) * self._extent(q, 4)).sum())
        ms = C.c_float()
        trip = None if out_device_ptr else np.empty((max(cap, 1), 3), dtype=np.uint32)
        L.check(getattr(L.lib(), "dcdf_" + entry)(self._handle(), q.ctypes.data_as(C.POINTER(L.Cube)), C.c_void_p(lo.ctypes.data),
                                                 C.c_void_p(hi.ctypes.data), C.c_size_t(len(q)), C.c_void_p(out_device_ptr or trip.ctypes.data),
                                                 C.c_size_t(cap), L.MEM_DEVICE if out_device_ptr else L.MEM_HOST, C.c_void_p(counts.ctypes.data),
                                                 C.c_void_p(offs.ctypes.data), C.byref(ms)), entry)
        return trip, offs, counts, ms.value

    def search_flat(self, cubes, lower, upper, out_device_ptr=None, cap=None):
        """search of dataset-level cubes through dcdf_raster_search_batch: returns (triples uint32[hits, 3] in raster coordinates
        -- or None when they stay on the device --, offsets, counts, kernel ms)."""
        return self._search("raster_search_batch", cubes, lambda n: (np.asarray(lower, dtype=np.int64), np.asarray(upper, dtype=np.int64)),
                            out_device_ptr, cap)

    def search_values_flat(self, cubes, lower, upper, out_device_ptr=None, cap=None):
        """Value search of dataset-level cubes through dcdf_raster_search_values_batch: real-valued [lower, upper] per cube,
        translated on the device per piece with the piece's chunk's encoding and fractional bits.  Returns what search_flat
        returns (triples uint32[hits, 3] in raster coordinates or None, offsets, counts, kernel ms)."""
        return self._search("raster_search_values_batch", cubes,
                            lambda n: (np.broadcast_to(np.asarray(b, dtype=np.float64), (n,)) for b in (lower, upper)), out_device_ptr, cap)

    def get_flat(self, points, dtype=np.int64, out_device_ptr=None):
        """Dataset-level points [n, 3] of (instant, row, col) through dcdf_raster_get_batch (Superchunk::get, superchunk.rs:313-352),
        typed as fill_windows_flat.  Host form: returns (values of dtype [n], kernel ms); device form (out_device_ptr): value i is
        written at element i there, returns kernel ms."""
        p = np.ascontiguousarray(np.asarray(points, dtype=np.uint32).reshape(-1, 3))
        dtype = np.dtype(dtype)
        ms = C.c_float()
        out = None if out_device_ptr else np.empty(max(1, len(p)), dtype=dtype)
        L.check(L.lib().dcdf_raster_get_batch(self._handle(), C.c_void_p(p.ctypes.data), C.c_size_t(len(p)),
                                              C.c_void_p(out_device_ptr or out.ctypes.data), _ENC[dtype],
                                              L.MEM_DEVICE if out_device_ptr else L.MEM_HOST, C.byref(ms)), "raster_get_batch")
        return ms.value if out_device_ptr else (out[:len(p)], ms.value)

    def fill_cells_flat(self, cells, dtype=np.int64, out_device_ptr=None, out_offset=None):
        """Dataset-level cell series [n, 4] of (start, end, row, col) through dcdf_raster_fill_cell_batch (Superchunk::fill_cell,
        superchunk.rs:356-400).  Host form: returns (flat array of dtype, offsets uint64[n], kernel ms): series i is
        flat[offsets[i]:offsets[i] + |end - start|].  Device form (out_device_ptr; out_offset in elements, None = one after the
        other): returns kernel ms."""
        q = np.ascontiguousarray(np.asarray(cells, dtype=np.uint32).reshape(-1, 4))
        dtype = np.dtype(dtype)
        ms = C.c_float()
        out = None
        if out_device_ptr is None:
            ln = self._extent(q, 0).astype(np.uint64)
            off = np.zeros(len(q), dtype=np.uint64)
            if len(q) > 1:
                off[1:] = np.cumsum(ln)[:-1]
            out = np.empty(max(1, int(ln.sum())), dtype=dtype)
        else:
            off = None if out_offset is None else np.ascontiguousarray(np.asarray(out_offset, dtype=np.uint64))
        L.check(L.lib().dcdf_raster_fill_cell_batch(self._handle(), C.c_void_p(q.ctypes.data), C.c_size_t(len(q)),
                                                    C.c_void_p(out_device_ptr if out is None else out.ctypes.data), _ENC[dtype],
                                                    L.MEM_DEVICE if out is None else L.MEM_HOST, None if off is None else C.c_void_p(off.ctypes.data),
                                                    C.byref(ms)), "raster_fill_cell_batch")
        return ms.value if out is None else (out[:int(ln.sum())], off, ms.value)

    @staticmethod
    def chunk_grid(shape, tile=256, chunk_size=32):
        """[(t0, t1, r0, r1, c0, c1)] of every chunk, in chunk-id order (segment-major, then tile row, tile col)."""
        T, R, Cc = shape
        out = []
        for t0 in range(0, T, chunk_size):
            for r0 in range(0, R, tile):
                for c0 in range(0, Cc, tile):
                    out.append((t0, min(T, t0 + chunk_size), r0, min(R, r0 + tile), c0, min(Cc, c0 + tile)))
        return out

    # ---- routing: dataset-level cubes -> chunk-level sub-queries -------------------------------------------------
    def split(self, cubes):
        """cubes: int array [n, 6] of half-open (t0, t1, r0, r1, c0, c1), already inside the raster.  Returns
        sub[m, 8] = (query, chunk id, local t0, t1, r0, r1, c0, c1), ordered by query, then segment, tile row, tile col
        (span.rs:190-216 over time, superchunk.rs:589-633 over rows/cols).  Only for rasters whose every leaf is a whole chunk: the
        chunk-level calls it feeds know nothing of elided or offset leaves (ValueError)."""
        if self.tiles is not None and any(t.chunk is None or t.row0 or t.col0 for t in self.tiles):
            raise ValueError("this raster has elided or offset leaves: the host-routed helpers cannot answer it; use the *_flat methods")
        q = np.asarray(cubes, dtype=np.int64)
        n = len(q)
        cs, tl = self.chunk_size, self.tile
        s0, s1 = q[:, 0] // cs, (q[:, 1] - 1) // cs
        i0, i1 = q[:, 2] // tl, (q[:, 3] - 1) // tl
        j0, j1 = q[:, 4] // tl, (q[:, 5] - 1) // tl
        empty = (q[:, 1] <= q[:, 0]) | (q[:, 3] <= q[:, 2]) | (q[:, 5] <= q[:, 4])
        ns = np.where(empty, 0, s1 - s0 + 1)
        ni = np.where(empty, 0, i1 - i0 + 1)
        nj = np.where(empty, 0, j1 - j0 + 1)
        cnt = ns * ni * nj
        m = int(cnt.sum())
        qid = np.repeat(np.arange(n), cnt)
        first = np.repeat(np.cumsum(cnt) - cnt, cnt)
        k = np.arange(m) - first  # ordinal of the sub-query inside its query
        nij = (ni * nj)[qid]
        ds, rem = k // nij, k % nij
        di, dj = rem // nj[qid], rem % nj[qid]
        seg, ti, tj = s0[qid] + ds, i0[qid] + di, j0[qid] + dj
        a0, a1 = np.maximum(q[qid, 0], seg * cs), np.minimum(q[qid, 1], seg * cs + cs)
        b0, b1 = np.maximum(q[qid, 2], ti * tl), np.minimum(q[qid, 3], ti * tl + tl)
        d0, d1 = np.maximum(q[qid, 4], tj * tl), np.minimum(q[qid, 5], tj * tl + tl)
        cid = (seg * self.nti + ti) * self.ntj + tj
        return np.stack([qid, cid, a0 - seg * cs, a1 - seg * cs, b0 - ti * tl, b1 - ti * tl, d0 - tj * tl, d1 - tj * tl], axis=1)

    def _origin(self, cid):
        seg, rem = cid // (self.nti * self.ntj), cid % (self.nti * self.ntj)
        return seg * self.chunk_size, (rem // self.ntj) * self.tile, (rem % self.ntj) * self.tile

    def _handles(self, sub):
        return (C.c_void_p * len(sub))(*[self.chunks[int(c)]._h for c in sub[:, 1]])

    # ---- queries ---------------------------------------------------------------------------------------------------
    def window_pieces(self, cubes):
        """fill_window of every cube, as decoded pieces: returns (sub, out int64[total], woff, vol, kernel_ms); the
        piece of sub-query k is out[woff[k]:woff[k]+vol[k]] shaped by its local cube."""
        sub = self.split(cubes)
        m = len(sub)
        vol = ((sub[:, 3] - sub[:, 2]) * (sub[:, 5] - sub[:, 4]) * (sub[:, 7] - sub[:, 6])).astype(np.uint64)
        woff = np.zeros(m, dtype=np.uint64)
        if m > 1:
            woff[1:] = np.cumsum(vol)[:-1]
        total = int(vol.sum())
        out = np.empty(max(total, 1), dtype=np.int64)
        ms = C.c_float()
        if m:
            cub = np.ascontiguousarray(sub[:, 2:8].astype(np.uint32))
            L.check(L.lib().dcdf_query_fill_window_batch(self._handles(sub), cub.ctypes.data_as(C.POINTER(L.Cube)), C.c_size_t(m),
                                                         C.c_void_p(out.ctypes.data), C.c_void_p(woff.ctypes.data), C.byref(ms)),
                    "fill_window_batch")
        return sub, out[:total], woff, vol, ms.value

    def fill_windows(self, cubes):
        """[ndarray[t, r, c] int64 stored values] per cube (mmarray.rs:186 `window` over the whole raster)."""
        q = np.asarray(cubes, dtype=np.int64)
        sub, out, woff, vol, _ = self.window_pieces(q)
        res = [np.zeros((max(0, c[1] - c[0]), max(0, c[3] - c[2]), max(0, c[5] - c[4])), dtype=np.int64) for c in q]
        for k in range(len(sub)):
            qi, cid, a0, a1, b0, b1, d0, d1 = (int(x) for x in sub[k])
            t, r, c = self._origin(cid)
            piece = out[int(woff[k]):int(woff[k]) + int(vol[k])].reshape(a1 - a0, b1 - b0, d1 - d0)
            res[qi][t + a0 - q[qi, 0]:t + a1 - q[qi, 0], r + b0 - q[qi, 2]:r + b1 - q[qi, 2],
                    c + d0 - q[qi, 4]:c + d1 - q[qi, 4]] = piece
        return res

    def search_pieces(self, cubes, lower, upper):
        """search of every cube: returns (sub, triples uint32[hits, 3] local to their chunk, soff, counts, kernel_ms)."""
        sub = self.split(cubes)
        m = len(sub)
        lo = np.ascontiguousarray(np.asarray(lower, dtype=np.int64)[sub[:, 0]])
        hi = np.ascontiguousarray(np.asarray(upper, dtype=np.int64)[sub[:, 0]])
        counts = np.zeros(m, dtype=np.uint64)
        soff = np.zeros(m, dtype=np.uint64)
        cap = int(((sub[:, 3] - sub[:, 2]) * (sub[:, 5] - sub[:, 4]) * (sub[:, 7] - sub[:, 6])).sum())
        trip = np.empty((max(cap, 1), 3), dtype=np.uint32)
        ms = C.c_float()
        if m:
            cub = np.ascontiguousarray(sub[:, 2:8].astype(np.uint32))
            L.check(L.lib().dcdf_query_search_batch(self._handles(sub), cub.ctypes.data_as(C.POINTER(L.Cube)), C.c_void_p(lo.ctypes.data),
                                                    C.c_void_p(hi.ctypes.data), C.c_size_t(m), C.c_void_p(trip.ctypes.data),
                                                    C.c_size_t(cap), C.c_void_p(counts.ctypes.data), C.c_void_p(soff.ctypes.data),
                                                    C.byref(ms)), "search_batch")
        return sub, trip, soff, counts, ms.value

    def search(self, cubes, lower, upper):
        """[int64[hits, 3] (instant, row, col) in raster coordinates] per cube (mmarray.rs:206; span.rs:231-270 adds the
        segment offset, superchunk.rs:516-585 the tile origin)."""
        sub, trip, soff, counts, _ = self.search_pieces(cubes, lower, upper)
        res = [[] for _ in range(len(cubes))]
        for k in range(len(sub)):
            if counts[k]:
                org = np.array(self._origin(int(sub[k, 1])), dtype=np.int64)
                res[int(sub[k, 0])].append(trip[int(soff[k]):int(soff[k]) + int(counts[k])].astype(np.int64) + org)
        return [np.concatenate(r) if r else np.zeros((0, 3), dtype=np.int64) for r in res]


# ---- the region statistics, one description each ---------------------------------------------------------------------------------
def _planes(q, n):
    """elements of n [rows, cols] planes per cube (a cube without instants writes nothing)"""
    return np.where(q[:, 1] == q[:, 0], 0, EncodedRaster._extent(q, 2) * EncodedRaster._extent(q, 4) * n)


class _ReduceTime:
    """reduce_time, and what a region statistic's description holds; the others override what differs.  An instance is one call:
    __init__ checks and normalises the statistic's own arguments that need no cube, in their order (every form begins with them).
    The drivers -- EncodedRaster._flat, EncodedRaster._whole, Variable._statistic -- do the rest from these:
      name, dtype, zeroed     the entry dcdf_raster_<name>_batch, its output's dtype, whether the output must start as zeros
      names, fill             the result's arrays in plane order and {name: its value where nothing was read}; names None: one dense
                              array, `fill` its value
      over_time               a statistic over time: without cells there is nothing to read either (else: only without instants)
      flat(cubes, *arrays)    the flat form's arrays per cube (labels, masks, bounds) staged against the cubes; returns the cubes
      count(q)                elements per cube
      args(n, out, mem, off, stats)  the C arguments between the cubes and the kernel ms, in the entry's own order (_region_call)
      window(nt, rows, cols, *arrays)  the whole-raster form's arrays against the window; returns flat()'s arrays for that one cube
      shape(nt, rows, cols)   of every array of the whole-raster result
      unread(own, arrays, nt, rows, cols)  the description as Variable makes it without instants, where no raster can be built"""
    name, dtype, zeroed, over_time = "reduce_time", np.float64, False, True
    fill = dict(min=np.nan, max=np.nan, sum=0.0, count=0.0, mean=np.nan)

    def __init__(self, ops):
        self.mask, self.names = EncodedRaster.reduce_ops(ops)

    def flat(self, cubes):
        return EncodedRaster._cubes(cubes)

    def count(self, q):
        return _planes(q, len(self.names))

    def args(self, n, out, mem, off, stats):
        return n, C.c_uint32(self.mask), out, mem, off, stats

    def window(self, nt, rows, cols):
        return ()

    def shape(self, nt, rows, cols):
        return rows, cols

    @classmethod
    def unread(cls, own, arrays, nt, rows, cols):
        S = cls(*own)
        S.window(nt, rows, cols, *arrays)
        return S

    def nothing(self, shape):
        """the result of `shape` where nothing was read -- no instant, no cell, no group or zone --, typed as its arrays are"""
        if self.names is None:
            return np.full(shape, self.fill, dtype=self.dtype)
        return {n: np.full(shape, self.fill[n], dtype=self.dtype) for n in self.names}

    def cut(self, out, shape):
        """one cube's flat result as arrays of `shape`, one after the other in the order of `names`"""
        n = int(np.prod(shape, dtype=np.int64))
        if self.names is None:
            return out[:n].reshape(shape)
        return {name: out[i * n:(i + 1) * n].reshape(shape) for i, name in enumerate(self.names)}


class _MomentsTime(_ReduceTime):
    name = "moments_time"
    fill = dict(count=0.0, mean=np.nan, var=np.nan, std=np.nan)

    def __init__(self, ops, ddof):
        self.mask, self.names = EncodedRaster.moment_ops(ops)
        if isinstance(ddof, bool) or not isinstance(ddof, (int, np.integer)) or ddof not in (0, 1):
            raise ValueError("moments_time: ddof %r is neither 0 nor 1" % (ddof,))
        self.ddof = int(ddof)

    def args(self, n, out, mem, off, stats):
        return n, C.c_uint32(self.mask), C.c_uint32(self.ddof), out, mem, off, stats


class _Grouped:
    """A statistic per group of instants or zone of cells: (labels, n) are its arrays, uint16 labels, `none` and every label >= n in
    no group.  noun, extent: "group" of "instants", or "zone" of the "window"; labelled(nt, rows, cols): the shape the labels have."""

    def groups(self, n, lab=None):
        """n_groups / n_zones, 1 .. 65535; None: the largest label of `lab`, `none` apart, plus 1 (at least 1)"""
        if n is None:
            named = lab[lab != self.none]
            n = int(named.max()) + 1 if named.size else 1
        n = int(n)
        if not 1 <= n <= 65535:
            raise ValueError("%s: n_%ss %d outside 1 .. 65535" % (self.name, self.noun, n))
        return n

    def beside(self, nt):
        """the arrays a grouped statistic takes behind (labels, n), checked against nt instants: window()'s tail.  None here."""
        return ()

    def window(self, nt, rows, cols, labels, n):
        lab, shape = np.asarray(labels), self.labelled(nt, rows, cols)
        if lab.dtype != np.uint16 or lab.shape != shape:
            raise ValueError("%s: the labels are %s %r, the %s uint16 %r" % (self.name, lab.dtype, lab.shape, self.extent, shape))
        self.n = self.groups(n, lab)
        return [lab], self.n


class _TimeGroups(_Grouped):
    noun, extent, none = "group", "instants", L.GROUP_NONE

    def flat(self, cubes, labels, n_groups):
        """labels: one uint16 array [instants] per cube, on the host"""
        self.n = self.groups(n_groups)
        q, labels = EncodedRaster._cubes(cubes), list(labels)
        if len(labels) != len(q):
            raise ValueError("%s: %d label arrays for %d cubes" % (self.name, len(labels), len(q)))
        nt = EncodedRaster._extent(q, 0)
        parts = []
        for i, m in enumerate(labels):
            m = np.asarray(m)
            if m.dtype != np.uint16:
                raise ValueError("%s: labels %d are %s, not uint16" % (self.name, i, m.dtype))
            if m.shape != (int(nt[i]),):
                raise ValueError("%s: labels %d have shape %r, their cube %d instants" % (self.name, i, m.shape, int(nt[i])))
            parts.append(m)
        self.labels = EncodedRaster._host_arrays(parts, np.uint16)
        return q

    def count(self, q):
        return _planes(q, len(self.names) * self.n)

    def labelled(self, nt, rows, cols):
        return (nt,)

    def shape(self, nt, rows, cols):
        return self.n, rows, cols


class _ReduceTimeGroups(_TimeGroups, _ReduceTime):
    name = "reduce_time_groups"  # (its statistics are reduce_time's, and so named in their messages)

    def args(self, n, out, mem, off, stats):
        return n, C.c_uint32(self.mask), self.labels[0], self.labels[1], C.c_uint32(self.n), out, mem, off, stats


class _MomentsTimeGroups(_TimeGroups, _MomentsTime):
    name = "moments_time_groups"  # (its statistics and ddof are moments_time's, and so named in their messages)

    def args(self, n, out, mem, off, stats):
        return n, C.c_uint32(self.mask), C.c_uint32(self.ddof), self.labels[0], self.labels[1], C.c_uint32(self.n), out, mem, off, stats


class _Spells(_ReduceTime):
    name, dtype = "spells", np.uint32
    fill = dict(count=0, longest=0, longest_start=L.SPELL_NONE, first=L.SPELL_NONE, last=L.SPELL_NONE)

    def __init__(self, ops):
        self.mask, self.names = EncodedRaster.spell_ops(ops)

    @staticmethod
    def bounds(lower, upper, n):
        """One (lower, upper) pair per cube as float64 arrays; a scalar is shared by all cubes.  NaN is refused."""
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,)))
        if np.isnan(lo).any() or np.isnan(hi).any():
            raise ValueError("spells: a NaN bound")
        return lo, hi

    def flat(self, cubes, lower, upper):
        q = EncodedRaster._cubes(cubes)
        self.lo, self.hi = self.bounds(lower, upper, len(q))
        return q

    def args(self, n, out, mem, off, stats):
        return C.c_void_p(self.lo.ctypes.data), C.c_void_p(self.hi.ctypes.data), n, C.c_uint32(self.mask), out, mem, off, stats

    def window(self, nt, rows, cols, lower, upper):
        self.bounds(lower, upper, 1)
        return lower, upper

    @classmethod
    def unread(cls, own, arrays, nt, rows, cols):  # (Variable.spells without instants looks at the bounds first)
        cls.bounds(*arrays, 1)
        return cls(*own)


class _QuantileTime(_ReduceTime):
    name, names, fill = "quantile_time", None, np.nan

    def __init__(self, probs, method):
        """1 .. 16 probabilities in [0, 1]; method one of "lower", "higher", "nearest", "linear" (or its DCDF_QUANTILE_* code)"""
        p = np.asarray(probs, dtype=np.float64)
        self.scalar = p.ndim == 0
        self.p = p = np.ascontiguousarray(p.reshape(-1))
        if not 1 <= p.size <= L.QUANTILE_MAX_PROBS:
            raise ValueError("quantile_time: %d probabilities, not 1 .. %d" % (p.size, L.QUANTILE_MAX_PROBS))
        if not ((p >= 0) & (p <= 1)).all():  # (a NaN fails both)
            raise ValueError("quantile_time: probabilities must lie in [0, 1]")
        if isinstance(method, str):
            if method not in L.QUANTILE_METHODS:
                raise ValueError("quantile_time: unknown method %r (one of %s)" % (method, ", ".join(L.QUANTILE_METHODS)))
            method = L.QUANTILE_METHODS[method]
        if int(method) not in L.QUANTILE_METHODS.values():
            raise ValueError("quantile_time: unknown method %r" % (method,))
        self.method = int(method)

    def count(self, q):
        return _planes(q, self.p.size)

    def args(self, n, out, mem, off, stats):
        return n, C.c_void_p(self.p.ctypes.data), C.c_uint32(self.p.size), C.c_int32(self.method), out, mem, off, stats

    def shape(self, nt, rows, cols):  # (a scalar `probs` has no axis of its own)
        return (rows, cols) if self.scalar else (self.p.size, rows, cols)


class _Masked:
    """A statistic over the selected cells of every instant: the masks are its arrays (EncodedRaster._mask_args)."""
    over_time = False

    def flat(self, cubes, masks=None):
        q = EncodedRaster._cubes(cubes)
        self.masks = EncodedRaster._mask_args(q, masks, self.name)
        return q

    def window(self, nt, rows, cols, mask):
        if mask is not None and np.asarray(mask).shape != (rows, cols):
            raise ValueError("%s: the mask has shape %r, the window %r" % (self.name, np.asarray(mask).shape, (rows, cols)))
        return (None if mask is None else [mask],)


class _ReduceSpace(_Masked, _ReduceTime):
    name = "reduce_space"  # (its statistics are reduce_time's, and so named in their messages)

    def count(self, q):
        return EncodedRaster._extent(q, 0) * len(self.names)

    def args(self, n, out, mem, off, stats):
        return (n, C.c_uint32(self.mask)) + self.masks[:3] + (out, mem, off, stats)

    def shape(self, nt, rows, cols):
        return (nt,)

    @classmethod
    def unread(cls, own, arrays, nt, rows, cols):  # (Variable.reduce_space without instants does not look at its mask)
        return cls(*own)


class _Zonal(_Grouped, _ReduceTime):
    name, over_time = "zonal", False  # (its statistics are reduce_time's, and so named in their messages)
    noun, extent, none = "zone", "window", L.ZONE_NONE

    def flat(self, cubes, labels, n_zones):
        self.n = self.groups(n_zones)
        q = EncodedRaster._cubes(cubes)
        self.labels = EncodedRaster._label_args(q, labels, "zonal")
        return q

    def count(self, q):
        return EncodedRaster._extent(q, 0) * (len(self.names) * self.n)

    def args(self, n, out, mem, off, stats):
        return (n, C.c_uint32(self.mask)) + self.labels[:3] + (C.c_uint32(self.n), out, mem, off, stats)

    def labelled(self, nt, rows, cols):
        return rows, cols

    def shape(self, nt, rows, cols):
        return self.n, nt


class _Histogram(_Masked, _ReduceTime):
    name, dtype, zeroed, names, fill = "histogram", np.uint64, True, None, 0

    def __init__(self, edges):
        """edges as float64 [bins + 1]: 1 .. 256 bins, no NaN, strictly increasing (-inf first and +inf last are fine)"""
        self.edges = e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
        if e.ndim != 1 or not 2 <= e.size <= L.HIST_MAX_BINS + 1:
            raise ValueError("histogram: edges must be 2 .. %d increasing values" % (L.HIST_MAX_BINS + 1))
        if np.isnan(e).any() or not (e[1:] > e[:-1]).all():
            raise ValueError("histogram: edges must be strictly increasing, without NaN")
        self.bins = e.size - 1

    def count(self, q):
        return EncodedRaster._extent(q, 0) * self.bins

    def args(self, n, out, mem, off, stats):
        return (n, C.c_void_p(self.edges.ctypes.data), C.c_uint32(self.bins)) + self.masks[:3] + (out, mem, off, stats)

    def shape(self, nt, rows, cols):
        return nt, self.bins


class _RegressTime(_ReduceTime):
    """The regressors are its arrays: the flat forms pass them as given, the whole-raster forms less their first value."""
    name = "regress_time"
    fill = dict(count=0.0, slope=np.nan, intercept=np.nan, corr=np.nan)

    def __init__(self, ops):
        self.mask, self.names = EncodedRaster.regress_ops(ops)

    def regressor(self, u, nt, which=""):
        """one regressor as float64 [nt]: real numbers (floats or integers) of that shape, every one finite"""
        u = np.asarray(u)
        if u.dtype.kind not in "fiu" or u.shape != (nt,):
            raise ValueError("%s: the regressor%s is %s %r, the instants real numbers %r" % (self.name, which, u.dtype, u.shape, (nt,)))
        u = u.astype(np.float64)
        if not np.isfinite(u).all():
            raise ValueError("%s: the regressor%s has a value that is not finite" % (self.name, which))
        return u

    def regressors(self, q, regs):
        """the flat form's: None -- the instant index of every cube --, or one regressor per cube, staged as given"""
        self.regs = None, None
        if regs is not None:
            regs = list(regs)
            if len(regs) != len(q):
                raise ValueError("%s: %d regressors for %d cubes" % (self.name, len(regs), len(q)))
            nt = EncodedRaster._extent(q, 0)
            self.regs = EncodedRaster._host_arrays([self.regressor(u, int(nt[i]), " %d" % i) for i, u in enumerate(regs)], np.float64)

    def shifted(self, nt, u):
        """the whole-raster form's regressor for flat(): less its first value, one float64 subtraction each; None stays None"""
        if u is None:
            return None
        u = self.regressor(u, nt)
        return [u - u[0] if nt else u]

    def flat(self, cubes, regressors=None):
        q = EncodedRaster._cubes(cubes)
        self.regressors(q, regressors)
        return q

    def args(self, n, out, mem, off, stats):
        return n, C.c_uint32(self.mask), self.regs[0], self.regs[1], out, mem, off, stats

    def window(self, nt, rows, cols, regressor=None):
        return (self.shifted(nt, regressor),)


class _RegressTimeGroups(_TimeGroups, _RegressTime):
    name = "regress_time_groups"  # (its statistics are regress_time's, and so named in their messages)

    def flat(self, cubes, labels, n_groups, regressors=None):
        q = _TimeGroups.flat(self, cubes, labels, n_groups)
        self.regressors(q, regressors)
        return q

    def args(self, n, out, mem, off, stats):
        return n, C.c_uint32(self.mask), self.regs[0], self.regs[1], self.labels[0], self.labels[1], C.c_uint32(self.n), out, mem, off, stats

    def beside(self, nt, regressor=None):
        return (self.shifted(nt, regressor),)

    def window(self, nt, rows, cols, labels, n, regressor=None):
        return tuple(_TimeGroups.window(self, nt, rows, cols, labels, n)) + self.beside(nt, regressor)


class _RollingTime(_ReduceTime):
    """The window, min_count and the kind are its own arguments; it takes no arrays."""
    name = "rolling_time"
    fill = dict(max=np.nan, argmax=np.nan, min=np.nan, argmin=np.nan, count=0.0)

    def __init__(self, ops, window, min_count, mean):
        """window 1 .. 65535 instants; min_count 1 .. window (None: window); mean: the sums divided by window, whole windows only"""
        self.mask, self.names = EncodedRaster.rolling_ops(ops)
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= L.ROLLING_MAX_WINDOW:
            raise ValueError("rolling_time: window %r outside 1 .. %d" % (window, L.ROLLING_MAX_WINDOW))
        self.w = int(window)
        if min_count is None:
            min_count = self.w
        if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or not 1 <= min_count <= self.w:
            raise ValueError("rolling_time: min_count %r outside 1 .. window %d" % (min_count, self.w))
        self.min_count = int(min_count)
        if mean and self.min_count != self.w:
            raise ValueError("rolling_time: the mean takes whole windows, min_count %d is not window %d" % (self.min_count, self.w))
        self.kind = L.ROLLING_MEAN if mean else L.ROLLING_SUM

    def own(self):
        return C.c_uint32(self.mask), C.c_uint32(self.w), C.c_uint32(self.min_count), C.c_int32(self.kind)

    def args(self, n, out, mem, off, stats):
        return (n,) + self.own() + (out, mem, off, stats)


class _RollingTimeGroups(_TimeGroups, _RollingTime):
    name = "rolling_time_groups"  # (its statistics, window and min_count are rolling_time's, and so named in their messages)

    def args(self, n, out, mem, off, stats):
        return (n,) + self.own() + (self.labels[0], self.labels[1], C.c_uint32(self.n), out, mem, off, stats)
