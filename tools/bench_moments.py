#!/usr/bin/env python3
"""Moments over time (dcdf_raster_moments_time_batch, dcdf_raster_moments_time_groups_batch) against the calls next to them, on one
cube over the first --segments segments of the configs[2] raster (4096 x 4096; int32, and float32 = values / 8), results left on
the device, in-kernel time (HIP events).  A row's variants are alternated --reps times after a warm-up, best of the repetitions,
every repetition kept:
  plain   moments_time, std alone and all four planes       against decode_flat and reduce_time with all five statistics
  clim    the same under the labels i % 7                    against reduce_time_groups with all five under the same labels
  runs    the same under the labels i // 16                  against reduce_time_groups with all five under the same labels
Three row bands of the plain and the clim row (all four planes, ddof 1) are compared bit for bit with decode plus the model of
tests/moment_model.py.  Prints ONE JSON line and writes it to profiles/moments_bench.json."""
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
from bench_reduce_time_groups import alternate  # noqa: E402

STD, ALL, REDUCE_ALL = 8, 15, 31


def measure(R, T, E, dt, reps, band_rows=64):
    import moment_model as MM
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    zero = np.zeros(1, dtype=np.uint64)
    i = np.arange(T)
    n_runs = -(-T // 16)
    out = DeviceBuffer(5 * max(7, n_runs) * plane * 8)  # the largest result: reduce_time_groups with all five statistics
    dec = DeviceBuffer(T * plane * dt.itemsize)
    sets = {"clim": ((i % 7).astype(np.uint16), 7), "runs": ((i // 16).astype(np.uint16), n_runs)}

    def moments(ops, key=None):
        if key is None:
            return lambda: R.moments_time_flat(cube, ops, 1, out_device_ptr=out.ptr, out_offset=zero)[0]
        lab, n = sets[key]
        return lambda: R.moments_time_groups_flat(cube, ops, [lab], n, 1, out_device_ptr=out.ptr, out_offset=zero)[0]

    def reduce_groups(key):
        lab, n = sets[key]
        return lambda: R.reduce_time_groups_flat(cube, REDUCE_ALL, [lab], n, out_device_ptr=out.ptr, out_offset=zero)[0]

    res = {"plain": alternate({"moments_std": moments(STD), "moments_all": moments(ALL),
                               "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
                               "reduce_time_all": lambda: R.reduce_time_flat(cube, REDUCE_ALL, out_device_ptr=out.ptr, out_offset=zero)[0]}, reps)}
    for key in sets:
        res[key] = alternate({"moments_std": moments(STD, key), "moments_all": moments(ALL, key), "reduce_time_groups_all": reduce_groups(key)}, reps)
    best = {r: {k: min(v) for k, v in res[r].items()} for r in res}
    ratios = {r: {"%s_over_%s" % (m, k): round(best[r][m] / v, 3) for m in ("moments_std", "moments_all") for k, v in best[r].items()
                  if not k.startswith("moments")} for r in res}
    # bit for bit: three row bands of the plain and the clim row against decode + model
    bands = sorted({0, (E // 2 // band_rows) * band_rows, E - band_rows})
    lab, n_groups = sets["clim"]
    for grouped in (False, True):
        (moments(ALL, "clim") if grouped else moments(ALL))()
        for r0 in bands:
            flat, _, _, _ = R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)
            a = flat[:T * band_rows * E].reshape(T, band_rows, E)
            want = MM.moments_time_groups(a, lab, n_groups, 1) if grouped else {n: v[None] for n, v in MM.moments_time(a, 1).items()}
            for k, name in enumerate(MM.NAMES):
                for g in range(n_groups if grouped else 1):
                    got = out.read(((k * (n_groups if grouped else 1) + g) * plane + r0 * E) * 8, band_rows * E * 8, np.uint64)
                    assert np.array_equal(got, MM.bits(want[name][g]).ravel()), "%s of group %d differs in the band at row %d" % (name, g, r0)
    _, stats = R.moments_time_flat(cube, ALL, 1, out_device_ptr=out.ptr, out_offset=zero)
    out.free()
    dec.free()
    return {"cells_read": T * plane, "kernel_ms": res, "best_kernel_ms": best, "ratios": ratios, "stats_bulk_walk_elided": [int(v) for v in stats],
            "bands_checked_rows": bands}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab", help="any of a (int32), b (float32)")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_bench.json"))
    a = ap.parse_args()
    res = {}
    for w in a.workload:
        R, dt, keep = device_raster(a.segments, w == "b", a.extent)
        res[{"a": "int32", "b": "float32"}[w]] = measure(R, 32 * a.segments, a.extent, dt, a.reps)
        R.close()
        for c in keep[1]:
            c.close()
        keep[0].close()
    line = json.dumps({"tool": "bench_moments", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
