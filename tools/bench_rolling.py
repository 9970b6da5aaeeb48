#!/usr/bin/env python3
"""Rolling windows over time (dcdf_raster_rolling_time_batch, dcdf_raster_rolling_time_groups_batch) against the calls next to it,
on one cube over the first --segments segments of the configs[2] raster (4096 x 4096; int32, and float32 = values / 8), results
left on the device, in-kernel time (HIP events).  The variants are alternated --reps times after a warm-up, best of the
repetitions, every repetition kept:
  rolling_all / rolling_max     rolling_time_flat with window 5, all five planes, and with the max alone
  rolling_w30                   all five planes, window 30
  rolling_runs                  window 5 under the labels i // 16: contiguous groups, one rebuild per run
  rolling_mod7                  window 5 under the labels i % 7: every window summed again from its values
  decode                        decode_flat of the same cube in the raster's own dtype
  regress_all                   regress_time_flat with all four planes: the same stream, every value read once
  median                        quantile_time_flat, p = 0.5
The one expectation: the median reads the slab several times and the plain window-5 call twice (head and tail), both with a lane
per cell over the same slab, so rolling_all above the median of the same run is an error (asserted, margin 1.0).  Three row bands
of rolling_all and rolling_runs are compared bit for bit with decode plus the model of tests/rolling_model.py.  Prints ONE JSON
line and writes it to profiles/rolling_bench.json."""
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

MAX, ALL = 1, 31
ROLLING = ("rolling_all", "rolling_max", "rolling_w30", "rolling_runs", "rolling_mod7")


def measure(R, T, E, dt, reps, band_rows=4):
    import rolling_model as WM
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    zero = np.zeros(1, dtype=np.uint64)
    i = np.arange(T)
    runs, mod7 = (i // 16).astype(np.uint16), (i % 7).astype(np.uint16)
    n_runs = int(runs.max()) + 1
    out = DeviceBuffer(5 * max(7, n_runs) * plane * 8)  # the largest result: five planes per group
    dec = DeviceBuffer(T * plane * dt.itemsize)

    def rolling(ops, w, lab=None, n=None):
        if lab is None:
            return lambda: R.rolling_time_flat(cube, ops, w, out_device_ptr=out.ptr, out_offset=zero)[0]
        return lambda: R.rolling_time_groups_flat(cube, ops, [lab], n, w, out_device_ptr=out.ptr, out_offset=zero)[0]

    res = alternate({"rolling_all": rolling(ALL, 5), "rolling_max": rolling(MAX, 5), "rolling_w30": rolling(ALL, 30),
                     "rolling_runs": rolling(ALL, 5, runs, n_runs), "rolling_mod7": rolling(ALL, 5, mod7, 7),
                     "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
                     "regress_all": lambda: R.regress_time_flat(cube, 15, out_device_ptr=out.ptr, out_offset=zero)[0],
                     "median": lambda: R.quantile_time_flat(cube, [0.5], "linear", out_device_ptr=out.ptr, out_offset=zero)[0]}, reps)
    best = {k: min(v) for k, v in res.items()}
    ratios = {"%s_over_%s" % (m, k): round(best[m] / best[k], 3) for m in ROLLING for k in ("decode", "regress_all", "median")}
    # bit for bit: three row bands of the plain and the runs call against decode + model
    bands = sorted({0, (E // 2 // band_rows) * band_rows, E - band_rows})
    for grouped in (False, True):
        (rolling(ALL, 5, runs, n_runs) if grouped else rolling(ALL, 5))()
        n_groups = n_runs if grouped else 1
        for r0 in bands:
            flat, _, _, _ = R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)
            a = flat[:T * band_rows * E].reshape(T, band_rows, E)
            want = WM.rolling_time_groups(a, 5, runs if grouped else None, n_groups)
            for k, name in enumerate(WM.NAMES):
                for g in range(n_groups):
                    got = out.read(((k * n_groups + g) * plane + r0 * E) * 8, band_rows * E * 8, np.uint64)
                    assert np.array_equal(got, WM.bits(want[name][g]).ravel()), "%s of group %d differs in the band at row %d" % (name, g, r0)
    _, stats = R.rolling_time_flat(cube, ALL, 5, out_device_ptr=out.ptr, out_offset=zero)
    out.free()
    dec.free()
    return {"cells_read": T * plane, "kernel_ms": res, "best_kernel_ms": best, "ratios": ratios,
            "rolling_all_minus_regress_all_ms": round(best["rolling_all"] - best["regress_all"], 3),
            "rolling_all_minus_decode_ms": round(best["rolling_all"] - best["decode"], 3), "stats_bulk_walk_elided": [int(v) for v in stats],
            "bands_checked_rows": bands, "band_rows": band_rows, "rolling_all_not_above_median": bool(best["rolling_all"] <= best["median"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab", help="any of a (int32), b (float32)")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_bench.json"))
    a = ap.parse_args()
    res = {}
    for w in a.workload:
        R, dt, keep = device_raster(a.segments, w == "b", a.extent)
        res[{"a": "int32", "b": "float32"}[w]] = measure(R, 32 * a.segments, a.extent, dt, a.reps)
        R.close()
        for c in keep[1]:
            c.close()
        keep[0].close()
    line = json.dumps({"tool": "bench_rolling", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for name, r in res.items():  # the one expectation, after the figures are out
        b = r["best_kernel_ms"]
        assert b["rolling_all"] <= b["median"], "%s: the plain window-5 call (two reads of the slab) is slower than the median (several): %r" % (name, b)


if __name__ == "__main__":
    main()
