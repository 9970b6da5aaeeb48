#!/usr/bin/env python3
"""Reduce over space (dcdf_raster_reduce_space_batch) against dcdf_raster_decode_batch and dcdf_raster_reduce_time_batch on the same
cube, results left on the device, in-kernel time (HIP events), the calls alternated in one process:
  a  the first --segments segments of the configs[2] int32 raster (4096 x 4096, encoded on the device, opened where it lies)
  b  the same raster as float32 (values / 8, three fractional bits)
For each: reduce_space with all five statistics, with the mean alone, and with the mean under a mask on the device (a disc that
covers about half the cells); the decode of the same cube (the yardstick: its code is what it was before) and reduce_time's
mean.  The series of three instants are checked bit for bit against math.fsum, fmin / fmax and the count over the decode of
those instants (tests/space_model.py).  Prints ONE JSON line."""
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


def disc(E):
    """A disc of half the square's area, as uint8 [E, E]."""
    r, c = np.mgrid[0:E, 0:E]
    return (((r - E / 2.0) ** 2 + (c - E / 2.0) ** 2) < E * E / (2.0 * np.pi)).astype(np.uint8)


def measure(R, T, E, dt, reps):
    import space_model as SM
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    dec = DeviceBuffer(T * plane * dt.itemsize)
    red = DeviceBuffer(plane * 8)
    ser = DeviceBuffer(5 * T * 8)
    mask = disc(E)
    mbuf = DeviceBuffer(plane)
    mbuf.write(0, mask)
    zero = np.zeros(1, dtype=np.uint64)
    dmask = (mbuf.ptr, zero)
    calls = {
        "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
        "reduce_time_mean": lambda: R.reduce_time_flat(cube, MEAN, out_device_ptr=red.ptr, out_offset=zero)[0],
        "space_all": lambda: R.reduce_space_flat(cube, ALL, out_device_ptr=ser.ptr, out_offset=zero)[0],
        "space_mean": lambda: R.reduce_space_flat(cube, MEAN, out_device_ptr=ser.ptr, out_offset=zero)[0],
        "space_mean_masked": lambda: R.reduce_space_flat(cube, MEAN, masks=dmask, out_device_ptr=ser.ptr, out_offset=zero)[0],
    }
    for fn in calls.values():  # warm up (code objects, pooled allocations)
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(fn())
    # bit for bit: three instants against decode + model, unmasked (all five) and masked (the mean)
    _, stats = R.reduce_space_flat(cube, ALL, out_device_ptr=ser.ptr, out_offset=zero)
    got_all = ser.read(0, 5 * T * 8, np.float64).reshape(5, T)
    R.reduce_space_flat(cube, MEAN, masks=dmask, out_device_ptr=ser.ptr, out_offset=zero)
    got_masked = ser.read(0, T * 8, np.float64)
    instants = sorted({0, T // 2, T - 1})
    for t in instants:
        flat, _, _, _ = R.decode_flat([[t, t + 1, 0, E, 0, E]], dtype=dt)
        w = flat[:plane].reshape(1, E, E)
        want = SM.reduce_space(w)
        for i, n in enumerate(NAMES):
            assert np.float64(got_all[i, t]).view(np.uint64) == np.float64(want[n][0]).view(np.uint64), "%s differs at instant %d" % (n, t)
        want = SM.reduce_space(w, mask)
        assert np.float64(got_masked[t]).view(np.uint64) == np.float64(want["mean"][0]).view(np.uint64), "the masked mean differs at instant %d" % t
    for b in (dec, red, ser, mbuf):
        b.free()
    best = {k: min(v) for k, v in ms.items()}
    cells = T * plane
    return {"cells_read": cells, "decode_out_bytes": cells * dt.itemsize, "space_all_out_bytes": 5 * T * 8, "mask_selected_fraction": round(float(mask.mean()), 4),
            "kernel_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "best_kernel_ms": {k: round(v, 3) for k, v in best.items()},
            "spread_kernel_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
            "cells_per_s_kernel": {k: cells / (v / 1e3) for k, v in best.items()},
            "over_decode": {k: round(best[k] / best["decode"], 3) for k in best if k != "decode"},
            "over_reduce_time_mean": {k: round(best[k] / best["reduce_time_mean"], 3) for k in best if k.startswith("space")},
            "stats_bulk_walk_elided": [int(x) for x in stats], "instants_checked": instants}


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
    print(json.dumps({"tool": "bench_reduce_space", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res}))


if __name__ == "__main__":
    main()
