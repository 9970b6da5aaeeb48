#!/usr/bin/env python3
"""Value search throughput: the configs[4]-shaped search mix (random cubes, len_t U[1,8], h, w U[1,64], 10-percentile-wide
bands of the value range) on a float32 encoding of the configs[2] raster (the synthetic cells / 8, stored with 3 fractional
bits), through the raster entry points.

Two ways to ask the same question of the same chunks, alternated over three repetitions in one process:
  values   EncodedRaster.search_values_flat: real-valued bounds, translated per piece on the device
  integer  EncodedRaster.search_flat: the bounds translated beforehand on the host by dcdf_value_bounds (every chunk has the
           same fractional bits here, so one translation serves all the pieces of a cube; the raster has no NaN cells)
Both leave their triples on the device.  A spot check compares both result sets with each other and with a brute force.
Prints ONE JSON line."""
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

BITS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--extent", type=int, default=1024, help="rows = cols of the raster (a multiple of 256)")
    ap.add_argument("--segments", type=int, default=2, help="time segments of 32 instants")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=50)
    a = ap.parse_args()

    import dcdf_amd
    from dcdf_amd import _lib as L, synth
    from dcdf_amd.encoder import DeviceBuffer
    from dcdf_amd.raster import EncodedRaster

    extent, nt, TT = a.extent, a.extent // 256, 32 * a.segments
    t0 = time.perf_counter()
    grid = EncodedRaster.chunk_grid((TT, extent, extent), 256, 32)
    arrays = [(synth.cells(SEED, g[0], g[1], g[2], g[3], g[4], g[5], np.int32) / 8.0).astype(np.float32) for g in grid]
    builds = dcdf_amd.build_batch(arrays, k=2, fractional_bits=BITS)
    ER = EncodedRaster((TT, extent, extent), [b.data for b in builds], tile=256, chunk_size=32)
    ER._handle()
    build_s = time.perf_counter() - t0

    rng = np.random.default_rng(7)
    spec, _ = make_queries(rng, a.queries, TT, extent, nt)
    cubes = np.ascontiguousarray(np.stack(spec[:6], axis=1).astype(np.uint32))
    sample = np.concatenate([x[::97].ravel() for x in arrays]).astype(np.float64)
    pct = np.percentile(sample, np.arange(0, 101, 10))
    band = rng.integers(0, 10, a.queries)
    lo, hi = pct[band], pct[band + 1]
    t1 = time.perf_counter()
    tr = np.array([L.value_bounds(L.DCDF_F32, BITS, x, y) for x, y in zip(lo, hi)], dtype=object)
    ilo, ihi = tr[:, 0].astype(np.int64), tr[:, 1].astype(np.int64)
    translate_s = time.perf_counter() - t1
    vol = (spec[1] - spec[0]) * (spec[3] - spec[2]) * (spec[5] - spec[4])
    cap = int(vol.sum())
    dbuf = DeviceBuffer(max(12, cap * 12))

    runs = {"values": [], "integer": []}
    res = {}
    for _ in range(a.reps):
        for name in ("values", "integer"):
            w0 = time.perf_counter()
            if name == "values":
                _, offs, counts, ms = ER.search_values_flat(cubes, lo, hi, out_device_ptr=dbuf.ptr, cap=cap)
            else:
                _, offs, counts, ms = ER.search_flat(cubes, ilo, ihi, out_device_ptr=dbuf.ptr, cap=cap)
            wall = time.perf_counter() - w0
            runs[name].append({"wall_s": wall, "kernel_ms": ms, "queries_per_s": a.queries / wall})
            res[name] = (offs.copy(), counts.copy(), dbuf.read(0, int(counts.sum()) * 12, np.uint32).reshape(-1, 3))

    # spot check: both result sets, and a brute force of the predicate on the typed values
    (vo, vc, vt), (io, ic, it) = res["values"], res["integer"]
    assert np.array_equal(vc, ic), "values / integer counts differ"
    checked = 0
    for q in rng.integers(0, a.queries, a.check):
        g = lambda o, c, t: set(map(tuple, t[int(o[q]):int(o[q]) + int(c[q])].tolist()))  # noqa: E731
        got = g(vo, vc, vt)
        assert got == g(io, ic, it), "values / integer triples differ"
        t0_, t1_, r0, r1, c0, c1 = (int(s[q]) for s in spec[:6])
        ref = (synth.cells(SEED, t0_, t1_, r0, r1, c0, c1, np.int32) / 8.0).astype(np.float32).astype(np.float64)
        want = set(map(tuple, (np.argwhere((ref >= lo[q]) & (ref <= hi[q])) + [t0_, r0, c0]).tolist()))
        assert got == want, "search_values mismatch"
        checked += 1
    dbuf.free()

    best = {k: max(r["queries_per_s"] for r in v) for k, v in runs.items()}
    print(json.dumps({
        "metric": "value search: queries/s end to end (raster entry points, device-resident triples), best of the alternated runs",
        "config": {"raster": [TT, extent, extent], "tile": 256, "chunk_size": 32, "encoding": "float32", "fractional_bits": BITS,
                   "chunks": len(grid), "queries": a.queries, "hits": int(vc.sum()), "reps": a.reps},
        "search_values_flat_queries_per_s": best["values"],
        "search_flat_pretranslated_queries_per_s": best["integer"],
        "ratio": best["values"] / best["integer"],
        "runs": runs,
        "host_translation_s": translate_s, "build_s": build_s,
        "spot_check": {"queries": checked, "ok": True},
    }))


if __name__ == "__main__":
    main()
