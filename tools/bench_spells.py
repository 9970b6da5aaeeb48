#!/usr/bin/env python3
"""Spell statistics (dcdf_raster_spells_batch) against dcdf_raster_decode_batch and dcdf_raster_reduce_time_batch on the same cube,
results left on the device, in-kernel time (HIP events), the four calls alternated in one process:
  a  the first --segments segments of the configs[2] int32 raster (4096 x 4096, encoded on the device, opened where it lies)
  b  the same raster as float32 (values / 8, three fractional bits)
For each, with the bound at the raster's median (a half-selective threshold, upper bound +inf): the decode of the cube (the
yardstick), reduce_time with COUNT alone, spells with COUNT alone, spells with all five statistics.  A few row bands of the five
planes are checked against the decode of the band folded by the NumPy model of tests/spell_model.py.  Prints ONE JSON line."""
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

ALL, COUNT, REDUCE_COUNT = 31, 1, 8


def measure(R, T, E, dt, reps, band_rows=64):
    import spell_model as M
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    # the bound: the median of a sample of the raster (three row bands of every instant)
    bands = sorted({0, (E // 2 // band_rows) * band_rows, E - band_rows})
    sample = np.concatenate([R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)[0] for r0 in bands])
    lower = float(np.nanmedian(sample))
    dec = DeviceBuffer(T * plane * dt.itemsize)
    red = DeviceBuffer(plane * 8)
    spl = DeviceBuffer(5 * plane * 4)
    zero = np.zeros(1, dtype=np.uint64)
    calls = {
        "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
        "reduce_count": lambda: R.reduce_time_flat(cube, REDUCE_COUNT, out_device_ptr=red.ptr, out_offset=zero)[0],
        "spells_count": lambda: R.spells_flat(cube, lower, np.inf, COUNT, out_device_ptr=spl.ptr, out_offset=zero)[0],
        "spells_all": lambda: R.spells_flat(cube, lower, np.inf, ALL, out_device_ptr=spl.ptr, out_offset=zero)[0],
    }
    for fn in calls.values():  # warm up (code objects, pooled allocations)
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(fn())
    # exact: row bands of the five planes against decode + model
    _, stats = R.spells_flat(cube, lower, np.inf, ALL, out_device_ptr=spl.ptr, out_offset=zero)
    hit_fraction = []
    for r0 in bands:
        flat, _, _, _ = R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)
        h = M.hits(flat[:T * band_rows * E].reshape(T, band_rows, E), lower, np.inf)
        hit_fraction.append(float(h.mean()))
        want = M.spells(h)
        for i, n in enumerate(M.NAMES):
            got = spl.read((i * plane + r0 * E) * 4, band_rows * E * 4, np.uint32)
            assert np.array_equal(got, want[n].ravel()), "plane %s differs in the band at row %d" % (n, r0)
    dec.free()
    red.free()
    spl.free()
    best = {k: min(v) for k, v in ms.items()}
    cells = T * plane
    return {"cells_read": cells, "lower": lower, "hit_fraction_of_bands": [round(x, 4) for x in hit_fraction], "decode_out_bytes": cells * dt.itemsize,
            "spells_all_out_bytes": 5 * plane * 4, "spells_count_out_bytes": plane * 4,
            "kernel_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "best_kernel_ms": {k: round(v, 3) for k, v in best.items()},
            "spread": {k: round(max(v) / min(v), 3) for k, v in ms.items()},
            "cells_per_s_kernel": {k: cells / (v / 1e3) for k, v in best.items()},
            "over_decode": {k: round(best[k] / best["decode"], 3) for k in ("reduce_count", "spells_count", "spells_all")},
            "over_reduce_count": {k: round(best[k] / best["reduce_count"], 3) for k in ("spells_count", "spells_all")},
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
    print(json.dumps({"tool": "bench_spells", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res}))


if __name__ == "__main__":
    main()
