#!/usr/bin/env python3
"""Query rates of a variable stored through Dataset.append, answered by Variable.raster() (dcdf_raster_create_tiles): the
configs[2] synthetic model, about a quarter of the 256 x 256 tiles forced uniform (NaN for float32, a constant for int32),
k2_levels [4, 8] (leaves of 256), chunk_size 32.  Measured, each with the in-kernel rate (HIP events) and the end-to-end rate
(wall time of the call, host routing and transfers included), results left on the device:
  windows   configs[4]-shaped cubes through fill_windows_flat
  values    the same cubes through search_values_flat, 10-percentile-wide bands of the value range
  points    random points through get_flat
  series    random cell series (length U[1, 64]) through fill_cells_flat
and, for comparison, host-routed Variable.window on a few of the cubes.  A spot check compares every kind with the source
array.  Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_query import SEED, make_queries  # noqa: E402


def stored_variable(dtype, T, E):
    from dcdf_amd import dataset as ds, _lib as L
    from dcdf_amd.encoder import DeviceBuffer, synth_fill
    buf = DeviceBuffer(T * E * E * 4)
    synth_fill(buf.ptr, L.DCDF_I32, SEED, 0, T, 0, E, 0, E)
    a = buf.read(0, T * E * E * 4, np.int32).reshape(T, E, E)
    buf.free()
    nt = E // 256
    rng = np.random.default_rng(11)
    uniform = rng.random((nt, nt)) < 0.25
    if dtype == "float32":
        a = (a / 8.0).astype(np.float32)
    for ti, tj in np.argwhere(uniform):
        a[:, 256 * ti:256 * ti + 256, 256 * tj:256 * tj + 256] = np.nan if dtype == "float32" else 7
    t = ds.Coordinate.time("t", 0, np.timedelta64(86400, "s"))
    y = ds.Coordinate.range("y", 0, 1, E, np.float64)
    x = ds.Coordinate.range("x", 0, 1, E, np.float64)
    d = ds.Dataset.new([t, y, x], [E, E], ds.Resolver())
    d = d.add_variable("v", 8, 32, [4, 8], dtype=a.dtype.type)
    d = d.append("v", a)
    return d.v, a, int(uniform.sum())


def timed(fn, reps):
    """(best kernel ms, best wall s) over reps calls."""
    best_k, best_w = float("inf"), float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        k = fn()
        best_w = min(best_w, time.perf_counter() - t0)
        best_k = min(best_k, k)
    return best_k, best_w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["int32", "float32"], default="int32")
    ap.add_argument("--extent", type=int, default=2304, help="rows = cols (k2_levels [4, 8] need 2048 < extent <= 4096)")
    ap.add_argument("--instants", type=int, default=64)
    ap.add_argument("--cubes", type=int, default=200000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--series", type=int, default=100000)
    ap.add_argument("--host-cubes", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    from dcdf_amd.encoder import DeviceBuffer
    T, E = a.instants, a.extent
    t0 = time.perf_counter()
    v, src, n_uniform = stored_variable(a.dtype, T, E)
    store_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    R = v.raster()
    raster_s = time.perf_counter() - t0
    n_elided = sum(t.chunk is None for t in R.tiles)

    rng = np.random.default_rng(7)
    spec, _ = make_queries(rng, a.cubes, T, E, E // 256)
    cubes = np.ascontiguousarray(np.stack(spec[:6], axis=1).astype(np.uint32))
    vol = ((cubes[:, 1] - cubes[:, 0]).astype(np.uint64) * (cubes[:, 3] - cubes[:, 2]) * (cubes[:, 5] - cubes[:, 4]))
    off = np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64)
    es = 4
    out = DeviceBuffer(int(vol.sum()) * es)
    res = {}
    k, w = timed(lambda: R.fill_windows_flat(cubes, dtype=src.dtype, out_device_ptr=out.ptr, out_offset=off), a.reps)
    res["windows"] = {"n": a.cubes, "kernel_qps": a.cubes / (k / 1e3), "e2e_qps": a.cubes / w}
    for q in (0, a.cubes // 2, a.cubes - 1):  # spot check
        c = cubes[q]
        got = out.read(int(off[q]) * es, int(vol[q]) * es, src.dtype)
        np.testing.assert_array_equal(got, src[c[0]:c[1], c[2]:c[3], c[4]:c[5]].ravel())
    out.free()

    sample = src[:, ::37, ::37]
    sample = sample[np.isfinite(sample)].astype(np.float64) if a.dtype == "float32" else sample.ravel().astype(np.float64)
    pct = np.percentile(sample, np.arange(0, 101, 10))
    band = rng.integers(0, 10, a.cubes)
    lo, hi = pct[band], pct[band + 1]
    cap = int(vol.sum())
    trip = DeviceBuffer(cap * 12)
    k, w = timed(lambda: R.search_values_flat(cubes, lo, hi, out_device_ptr=trip.ptr, cap=cap)[3], a.reps)
    res["values"] = {"n": a.cubes, "kernel_qps": a.cubes / (k / 1e3), "e2e_qps": a.cubes / w}
    _, offs, counts, _ = R.search_values_flat(cubes[:50], lo[:50], hi[:50], out_device_ptr=trip.ptr, cap=cap)
    for q in range(0, 50, 7):
        c = cubes[q]
        got = trip.read(int(offs[q]) * 12, int(counts[q]) * 12, np.uint32).reshape(-1, 3).astype(np.int64)
        w64 = src[c[0]:c[1], c[2]:c[3], c[4]:c[5]].astype(np.float64)
        want = np.argwhere((w64 >= lo[q]) & (w64 <= hi[q])) + np.array([c[0], c[2], c[4]])
        assert np.array_equal(got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))], want)
    trip.free()

    pts = np.stack([rng.integers(0, T, a.points), rng.integers(0, E, a.points), rng.integers(0, E, a.points)], axis=1).astype(np.uint32)
    pout = DeviceBuffer(a.points * es)
    k, w = timed(lambda: R.get_flat(pts, dtype=src.dtype, out_device_ptr=pout.ptr), a.reps)
    res["points"] = {"n": a.points, "kernel_qps": a.points / (k / 1e3), "e2e_qps": a.points / w}
    np.testing.assert_array_equal(pout.read(0, 4096 * es, src.dtype), src[pts[:4096, 0], pts[:4096, 1], pts[:4096, 2]])
    pout.free()

    s0 = rng.integers(0, T, a.series)
    s1 = np.minimum(T, s0 + rng.integers(1, 65, a.series))
    cells = np.stack([s0, s1, rng.integers(0, E, a.series), rng.integers(0, E, a.series)], axis=1).astype(np.uint32)
    ln = (s1 - s0).astype(np.uint64)
    soff = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    sout = DeviceBuffer(int(ln.sum()) * es)
    k, w = timed(lambda: R.fill_cells_flat(cells, dtype=src.dtype, out_device_ptr=sout.ptr, out_offset=soff), a.reps)
    res["series"] = {"n": a.series, "kernel_qps": a.series / (k / 1e3), "e2e_qps": a.series / w,
                     "elements_per_s_kernel": float(ln.sum()) / (k / 1e3)}
    for i in (0, a.series - 1):
        np.testing.assert_array_equal(sout.read(int(soff[i]) * es, int(ln[i]) * es, src.dtype), src[s0[i]:s1[i], cells[i, 2], cells[i, 3]])
    sout.free()

    nh = min(a.host_cubes, a.cubes)
    t0 = time.perf_counter()
    for c in cubes[:nh]:
        v.window(*(int(x) for x in c))
    host_s = time.perf_counter() - t0
    res["host_variable_window"] = {"n": nh, "e2e_qps": nh / host_s}

    print(json.dumps({"tool": "bench_stored_raster", "dtype": a.dtype, "shape": [T, E, E], "k2_levels": [4, 8], "chunk_size": 32,
                      "uniform_tiles": n_uniform, "elided_leaves": n_elided, "leaves": len(R.tiles), "store_s": round(store_s, 2),
                      "raster_create_s": round(raster_s, 2),
                      **{k: {x: (round(y, 1) if isinstance(y, float) else y) for x, y in d.items()} for k, d in res.items()}}))


if __name__ == "__main__":
    main()
