# The README's example, with its claims as assertions (needs an MI355X: python examples/quickstart.py)

import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repo root: dcdf_amd is used in-tree
import numpy as np, dcdf_amd as dc
from dcdf_amd.raster import EncodedRaster
a = np.random.default_rng(0).integers(0, 1000, size=(32, 256, 256)).astype(np.int32)
built = dc.Chunk.build(a)
data = built.data.write_to()
chunk = dc.Chunk.read_from(data)
assert chunk.get(3, 10, 20) == a[3, 10, 20]
assert (chunk.fill_window(dc.Cube(0, 8, 0, 64, 0, 64)) == a[:8, :64, :64]).all()
hits = chunk.iter_search(dc.Cube(0, 32, 0, 256, 0, 256), 100, 110)
assert len(hits) == int(((a >= 100) & (a <= 110)).sum())
grid = EncodedRaster.chunk_grid(a.shape, tile=128, chunk_size=16)
chunks = [b.data for b in dc.build_batch([np.ascontiguousarray(a[t0:t1, r0:r1, c0:c1]) for t0, t1, r0, r1, c0, c1 in grid])]
R = EncodedRaster(a.shape, chunks, tile=128, chunk_size=16)
flat, offsets, _ = R.fill_windows_flat([(10, 20, 100, 140, 120, 200)], dtype=np.int32)
assert (flat.reshape(10, 40, 80) == a[10:20, 100:140, 120:200]).all()
triples, offs, counts, _ = R.search_flat([(0, 32, 0, 256, 0, 256)], [100], [110])
assert int(counts[0]) == len(hits)
whole = R.decode(dtype=np.int32)
assert whole.shape == a.shape and (whole == a).all()
flat, offsets, _, stats = R.decode_flat([(0, 32, 0, 256, 0, 256)], dtype=np.int32)
assert (flat.reshape(a.shape) == a).all() and int(stats[0]) == a.size
maps = R.reduce_time(("mean", "max", "count"), 8, 24)
assert list(maps) == ["max", "count", "mean"] and (maps["max"] == a[8:24].max(0)).all() and (maps["count"] == 16).all()
assert (maps["mean"] == a[8:24].sum(0) / 16.0).all()
flat, offsets, _, stats = R.reduce_time_flat([(0, 32, 10, 200, 0, 256)], ("min", "sum"))
assert (flat.reshape(2, 190, 256) == np.stack([a[:, 10:200].min(0), a[:, 10:200].sum(0)])).all()
monthly = R.reduce_time_groups(("mean",), (np.arange(32) // 30).astype(np.uint16))
assert monthly["mean"].shape == (2, 256, 256) and (monthly["mean"][0] == a[:30].sum(0) / 30.0).all() and (monthly["mean"][1] == a[30:].sum(0) / 2.0).all()
clim = R.reduce_time_groups(("mean", "max"), (np.arange(32) % 12).astype(np.uint16))
assert list(clim) == ["max", "mean"] and all((clim["max"][g] == a[g::12].max(0)).all() and (clim["mean"][g] == a[g::12].sum(0) / len(a[g::12])).all() for g in range(12))
mom = R.moments_time(("mean", "var", "std"), ddof=1)  # the shifted sums of one walk: var is exactly 0 where a cell never changes
assert np.allclose(mom["std"], a.std(0, ddof=1)) and ((mom["var"] == 0) == (a == a[0]).all(0)).all()
assert (R.moments_time("var", 5, 6)["var"] == 0).all() and (R.moments_time("mean", 5, 6)["mean"] == a[5]).all()  # (one instant: constant cells)
one = R.moments_time_groups(("mean", "var", "std"), np.zeros(32, dtype=np.uint16), ddof=1)  # per group of instants; one group is the plain call
assert all((one[n][0].view(np.uint64) == mom[n].view(np.uint64)).all() for n in mom)
spell = R.spells(500, np.inf, ("count", "longest", "first"), 8, 24)  # instants counted from 8; 0xffffffff where nothing hit
hit = a[8:24] >= 500
cur = np.zeros((256, 256), dtype=np.int64)
best = cur.copy()
for t in range(16):
    cur = np.where(hit[t], cur + 1, 0)
    best = np.maximum(best, cur)
assert list(spell) == ["count", "longest", "first"] and (spell["count"] == hit.sum(0)).all() and (spell["longest"] == best).all()
assert (spell["first"] == np.where(hit.any(0), hit.argmax(0), 0xffffffff)).all()
flat, offsets, _, stats = R.spells_flat([(0, 32, 10, 200, 0, 256)], [99.5], [110.25], ("count", "last"))
band = (a[:, 10:200] >= 100) & (a[:, 10:200] <= 110)
assert (flat.reshape(2, 190, 256)[0] == band.sum(0)).all() and (flat.reshape(2, 190, 256)[1][band[31]] == 31).all()
series = R.reduce_space(("mean", "max", "count"), 8, 24, window=(10, 200, 0, 256))
assert list(series) == ["max", "count", "mean"] and (series["max"] == a[8:24, 10:200].max((1, 2))).all() and (series["count"] == 190 * 256).all()
disc = (np.mgrid[0:256, 0:256][0] - 128) ** 2 + (np.mgrid[0:256, 0:256][1] - 128) ** 2 < 100 ** 2
flat, offsets, _, stats = R.reduce_space_flat([(0, 32, 0, 256, 0, 256)], ("sum", "mean"), masks=[disc])
assert all(flat[t] == math.fsum(a[t][disc].tolist()) and flat[32 + t] == flat[t] / disc.sum() for t in range(32))
counts = R.histogram([0, 250, 500, 750, 1000], 8, 24, mask=disc)
assert counts.shape == (16, 4) and all((counts[t] == np.histogram(a[8 + t][disc], [0, 250, 500, 750, 1000])[0]).all() for t in range(16))
blocks = (np.arange(256)[:, None] // 64 * 4 + np.arange(256)[None, :] // 64).astype(np.uint16)
zones = R.zonal(("mean", "count"), blocks, 8, 24)
assert list(zones) == ["count", "mean"] and zones["mean"].shape == (16, 16) and (zones["count"] == 64 * 64).all()
assert all(zones["mean"][z, t] == math.fsum(a[8 + t][blocks == z].tolist()) / 4096.0 for z in range(16) for t in range(16))
q = R.quantile_time([0.5, 0.9], 8, 24)  # float64 [2, 256, 256]: the median and the 90th percentile of every cell's 16 values, exact
srt, h = np.sort(a[8:24], axis=0).astype(np.float64), 15 * 0.9
assert (q[0] == (srt[7] + srt[8]) / 2).all() and (q[1] == srt[int(h)] + (srt[int(h) + 1] - srt[int(h)]) * (h - int(h))).all()
assert (R.quantile_time(0.9, 8, 24, method="higher") == np.quantile(a[8:24], 0.9, axis=0, method="higher")).all()
trend = R.regress_time(("slope", "intercept", "corr"))  # per cell, the least-squares line against the instant index: a trend map
fit = np.polyfit(np.arange(32.0), a.reshape(32, -1).astype(np.float64), 1)
assert np.allclose(trend["slope"].ravel(), fit[0]) and np.allclose(trend["intercept"].ravel(), fit[1])
years = 1990.0 + np.arange(32)  # any regressor: taken less its first value, so the intercept is the fitted value at years[0]
assert np.allclose(R.regress_time(("intercept",), years)["intercept"], trend["intercept"]) and (np.abs(trend["corr"]) <= 1).all()
rx5 = R.rolling_time(("max", "argmax"), 5)  # per cell, the greatest sum of 5 consecutive instants and the instant it ended on: Rx5day
s5 = np.lib.stride_tricks.sliding_window_view(a.astype(np.float64), 5, axis=0).sum(-1)  # [28, 256, 256]: the windows that end at 4 .. 31
assert (rx5["max"] == s5.max(0)).all() and (rx5["argmax"] == s5.argmax(0) + 4).all()
low = R.rolling_time_groups(("min",), (np.arange(32) // 16).astype(np.uint16), 7, mean=True)  # the lowest 7-instant mean per half; a window is its last instant's
s7 = np.lib.stride_tricks.sliding_window_view(a.astype(np.float64), 7, axis=0).sum(-1)  # windows that end at 6 .. 31
assert (low["min"][0] == s7[:10].min(0) / 7.0).all() and (low["min"][1] == s7[10:].min(0) / 7.0).all()
print("readme example ok")
