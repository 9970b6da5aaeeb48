#!/usr/bin/env python3
"""Reduce over time (dcdf_raster_reduce_time_batch) against dcdf_raster_decode_batch on the same cube, results left on the device,
in-kernel time (HIP events), the three calls alternated in one process:
  a  the first --segments segments of the configs[2] int32 raster (4096 x 4096, encoded on the device, opened where it lies)
  b  the same raster as float32 (values / 8, three fractional bits)
For each: reduce_time with all five statistics, reduce_time with the mean alone, and the decode of the same cube (the yardstick:
its code is what it was before reduce_time existed).  A few row bands of the five planes are checked bit for bit against the
decode of the band reduced by the NumPy model of tests/reduce_model.py.  Prints ONE JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_bulk_decode import device_raster  # noqa: E402

ALL, MEAN = 31, 16
NAMES = ("min", "max", "sum", "count", "mean")


def measure(R, T, E, dt, reps, band_rows=64):
    import reduce_model as M
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    dec = DeviceBuffer(T * plane * dt.itemsize)
    red = DeviceBuffer(5 * plane * 8)
    zero = np.zeros(1, dtype=np.uint64)
    calls = {
        "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
        "reduce_all": lambda: R.reduce_time_flat(cube, ALL, out_device_ptr=red.ptr, out_offset=zero)[0],
        "reduce_mean": lambda: R.reduce_time_flat(cube, MEAN, out_device_ptr=red.ptr, out_offset=zero)[0],
    }
    for fn in calls.values():  # warm up (code objects, pooled allocations)
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(fn())
    # bit-for-bit: row bands of the five planes against decode + model
    _, stats = R.reduce_time_flat(cube, ALL, out_device_ptr=red.ptr, out_offset=zero)
    bands = sorted({0, (E // 2 // band_rows) * band_rows, E - band_rows})
    for r0 in bands:
        flat, _, _, _ = R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)
        want = M.reduce_time(flat[:T * band_rows * E].reshape(T, band_rows, E))
        for i, n in enumerate(NAMES):
            got = red.read((i * plane + r0 * E) * 8, band_rows * E * 8, np.uint64)
            assert np.array_equal(got, np.ascontiguousarray(want[n]).view(np.uint64).ravel()), "plane %s differs in the band at row %d" % (n, r0)
    dec.free()
    red.free()
    best = {k: min(v) for k, v in ms.items()}
    cells = T * plane
    return {"cells_read": cells, "decode_out_bytes": cells * dt.itemsize, "reduce_all_out_bytes": 5 * plane * 8, "reduce_mean_out_bytes": plane * 8,
            "kernel_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "best_kernel_ms": {k: round(v, 3) for k, v in best.items()},
            "cells_per_s_kernel": {k: cells / (v / 1e3) for k, v in best.items()},
            "reduce_all_over_decode": round(best["reduce_all"] / best["decode"], 3), "reduce_mean_over_decode": round(best["reduce_mean"] / best["decode"], 3),
            "stats_bulk_walk_elided": [int(x) for x in stats], "bands_checked_rows": bands}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab", help="any of a, b")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    a = ap.parse_args()
    res = {}
    for w in a.workload:
        R, dt, keep = device_raster(a.segments, w == "b", a.extent)
        res[w] = measure(R, 32 * a.segments, a.extent, dt, a.reps)
        R.close()
        for c in keep[1]:
            c.close()
        keep[0].close()
    print(json.dumps({"tool": "bench_reduce_time", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res}))


if __name__ == "__main__":
    main()
