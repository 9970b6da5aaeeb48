#!/usr/bin/env python3
"""Grouped reduce over time (dcdf_raster_reduce_time_groups_batch) against what a user does without it, on one cube over the
first --segments segments of the configs[2] raster (4096 x 4096; int32, and float32 = values / 8), results left on the device,
in-kernel time (HIP events).  Each row is run for the mean alone and for all five statistics; a row's variants are alternated
--reps times after a warm-up, best of the repetitions, every repetition kept:
  a  labels all 0, one group         against reduce_time_flat of the same cube (the cost of the label test)
  b  labels i // 16                  against reduce_time_flat with one cube per run of equal labels (what a user does today)
  c  labels i % 7                    against reduce_time_flat with one cube per instant; the host recombination of the per-instant
                                     planes that must follow is timed apart, on one band of rows, and scaled to the raster
  d  labels i % T, every group once  against decode_flat of the same cube (the output is as large as the cube)
  none  every label GROUP_NONE       nothing is decoded: the pass that fills the identities, the empty walk and the mean pass
Three row bands of row c are compared bit for bit with decode plus the model of tests/group_model.py.  Prints ONE JSON line and
writes it to profiles/reduce_time_groups_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_bulk_decode import device_raster  # noqa: E402

ALL, MEAN = 31, 16
NAMES = ("min", "max", "sum", "count", "mean")


def alternate(calls, reps):
    for fn in calls.values():  # warm up (code objects, pooled allocations)
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(fn())
    return {k: [round(x, 3) for x in v] for k, v in ms.items()}


def measure(R, T, E, dt, reps, band_rows=64):
    import group_model as GM
    import reduce_model as M
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    zero = np.zeros(1, dtype=np.uint64)
    i = np.arange(T)
    out = DeviceBuffer(5 * T * plane * 8)  # the largest result: row d with all five statistics
    dec = DeviceBuffer(T * plane * dt.itemsize)
    rows = {}

    def groups(ops, labels, n_groups):
        lab = [np.asarray(labels, dtype=np.uint16)]
        return lambda: R.reduce_time_groups_flat(cube, ops, lab, n_groups, out_device_ptr=out.ptr, out_offset=zero)[0]

    def per_cube(ops, bounds):
        cubes = np.array([[t0, t1, 0, E, 0, E] for t0, t1 in bounds], dtype=np.uint32)
        off = (np.arange(len(cubes), dtype=np.uint64) * np.uint64(bin(ops).count("1") * plane))
        return lambda: R.reduce_time_flat(cubes, ops, out_device_ptr=out.ptr, out_offset=off)[0]

    for tag, ops in (("mean", MEAN), ("all", ALL)):
        res = {}
        res["a"] = alternate({"groups": groups(ops, i * 0, 1), "reduce_time": per_cube(ops, [(0, T)])}, reps)
        res["b"] = alternate({"groups": groups(ops, i // 16, -(-T // 16)), "reduce_time_per_run": per_cube(ops, [(t, min(T, t + 16)) for t in range(0, T, 16)])},
                             reps)
        # (one cube per instant: MEAN alone is not enough to recombine -- the user asks for sum and count)
        res["c"] = alternate({"groups": groups(ops, i % 7, 7), "reduce_time_per_instant": per_cube(12 if ops == MEAN else ops, [(t, t + 1) for t in range(T)])},
                             reps)
        res["d"] = alternate({"groups": groups(ops, i % T, T), "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0]},
                             reps)
        res["none"] = alternate({"groups": groups(ops, i * 0 + 0xffff, 7)}, reps)
        best = {r: {k: min(v) for k, v in res[r].items()} for r in res}
        ratios = {r: round(best[r]["groups"] / min(v for k, v in best[r].items() if k != "groups"), 3) for r in "abcd"}
        rows[tag] = {"kernel_ms": res, "best_kernel_ms": best, "groups_over_other": ratios}
    # the host recombination row c needs after its per-instant call: sums and counts of one band of rows, chained per group in
    # instant order (the order the contract asks for; summing per-group partial results instead would give it up)
    x = np.random.default_rng(1).normal(size=(T, band_rows, E))
    t0 = time.perf_counter()
    for g in range(7):
        s = np.zeros((band_rows, E))
        for t in range(g, T, 7):
            s = s + x[t]
        s / max(1, len(range(g, T, 7)))
    band_ms = (time.perf_counter() - t0) * 1e3
    # bit for bit: three row bands of row c against decode + model
    lab = (i % 7).astype(np.uint16)
    _, stats = R.reduce_time_groups_flat(cube, ALL, [lab], 7, out_device_ptr=out.ptr, out_offset=zero)
    bands = sorted({0, (E // 2 // band_rows) * band_rows, E - band_rows})
    for r0 in bands:
        flat, _, _, _ = R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)
        want = GM.reduce_time_groups(flat[:T * band_rows * E].reshape(T, band_rows, E), lab, 7)
        for k, n in enumerate(NAMES):
            for g in range(7):
                got = out.read(((k * 7 + g) * plane + r0 * E) * 8, band_rows * E * 8, np.uint64)
                assert np.array_equal(got, np.ascontiguousarray(want[n][g]).view(np.uint64).ravel()), "%s of group %d differs in the band at row %d" % (n, g, r0)
    assert M.NAMES == NAMES
    out.free()
    dec.free()
    return {"cells_read": T * plane, "rows": rows, "host_recombine_ms_band": round(band_ms, 3), "host_recombine_band_rows": band_rows,
            "host_recombine_ms_scaled": round(band_ms * E / band_rows, 1), "stats_bulk_walk_elided": [int(v) for v in stats], "bands_checked_rows": bands}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab", help="any of a (int32), b (float32)")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_time_groups_bench.json"))
    a = ap.parse_args()
    res = {}
    for w in a.workload:
        R, dt, keep = device_raster(a.segments, w == "b", a.extent)
        res[{"a": "int32", "b": "float32"}[w]] = measure(R, 32 * a.segments, a.extent, dt, a.reps)
        R.close()
        for c in keep[1]:
            c.close()
        keep[0].close()
    line = json.dumps({"tool": "bench_reduce_time_groups", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
