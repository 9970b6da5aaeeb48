#!/usr/bin/env python3
"""Quantiles over time (dcdf_raster_quantile_time_batch) against dcdf_raster_decode_batch on the same cube, results left on the
device, in-kernel time (HIP events), the calls alternated in one process:
  a  the first --segments segments of the configs[2] int32 raster (4096 x 4096, encoded on the device, opened where it lies)
  b  the same raster as float32 (values / 8, three fractional bits)
For each: the decode of the cube (unchanged code: the yardstick), the median alone and five probabilities (0.05, 0.25, 0.5, 0.75,
0.95), method linear, each with the slab cap (K2R_QUANTILE_SLAB_BYTES) at 64 MiB, 256 MiB (the default) and 1 GiB.  Three row bands of the planes are
checked bit for bit against the decode of the band through the NumPy model of tests/quantile_model.py; the same bands give the
passes per cell (the library's host form of the selection).  Prints ONE JSON line and saves it to --out."""
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

MEDIAN, FIVE = [0.5], [0.05, 0.25, 0.5, 0.75, 0.95]
CAPS = {"64MiB": 64 << 20, "256MiB": 256 << 20, "1GiB": 1 << 30}


def measure(R, T, E, dt, reps, band_rows=64):
    import quantile_model as M
    from dcdf_amd import _lib
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    bands = sorted({0, (E // 2 // band_rows) * band_rows, E - band_rows})
    dec = DeviceBuffer(T * plane * dt.itemsize)
    qnt = DeviceBuffer(5 * plane * 8)
    zero = np.zeros(1, dtype=np.uint64)

    def quantile(probs, cap):
        def run():
            os.environ["K2R_QUANTILE_SLAB_BYTES"] = str(cap)  # (read on every call)
            return R.quantile_time_flat(cube, probs, "linear", out_device_ptr=qnt.ptr, out_offset=zero)[0]
        return run

    calls = {"decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0]}
    for name, cap in CAPS.items():
        calls["median_" + name] = quantile(MEDIAN, cap)
        calls["five_" + name] = quantile(FIVE, cap)
    for fn in calls.values():  # warm up (code objects, pooled allocations)
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(fn())
    # exact: row bands of the planes against decode + model; the passes of the same cells
    os.environ["K2R_QUANTILE_SLAB_BYTES"] = str(CAPS["256MiB"])
    passes = {}
    for label, probs in (("median", MEDIAN), ("five", FIVE)):
        _, stats = R.quantile_time_flat(cube, probs, "linear", out_device_ptr=qnt.ptr, out_offset=zero)
        per_cell = []
        for r0 in bands:
            flat, _, _, _ = R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)
            a = flat[:T * band_rows * E].reshape(T, band_rows, E)
            want = M.quantile_time(a, probs, "linear")
            for i in range(len(probs)):
                got = qnt.read((i * plane + r0 * E) * 8, band_rows * E * 8, np.float64)
                M.same_bits(got, want[i].ravel())
            host, n_pass = _lib.quantile_select_host(M.widen(a[:, :16]), probs, "linear")  # (16 rows of the band: 65 536 cells)
            M.same_bits(host, want[:, :16])
            per_cell.append(n_pass.ravel())
        per_cell = np.concatenate(per_cell)
        passes[label] = {"mean": round(float(per_cell.mean()), 3), "max": int(per_cell.max()), "cells": int(per_cell.size)}
    del os.environ["K2R_QUANTILE_SLAB_BYTES"]
    dec.free()
    qnt.free()
    best = {k: min(v) for k, v in ms.items()}
    cells = T * plane
    return {"cells_read": cells, "decode_out_bytes": cells * dt.itemsize, "slab_bytes_per_call": cells * 8, "median_out_bytes": plane * 8,
            "five_out_bytes": 5 * plane * 8, "kernel_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "best_kernel_ms": {k: round(v, 3) for k, v in best.items()}, "spread": {k: round(max(v) / min(v), 3) for k, v in ms.items()},
            "cells_per_s_kernel": {k: cells / (v / 1e3) for k, v in best.items()},
            "over_decode": {k: round(best[k] / best["decode"], 3) for k in best if k != "decode"},
            "passes_per_cell_after_the_first": passes, "stats_bulk_walk_elided": [int(x) for x in stats], "bands_checked_rows": bands}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab", help="any of a, b")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_bench.json"))
    a = ap.parse_args()
    res = {}
    for w in a.workload:
        R, dt, keep = device_raster(a.segments, w == "b", a.extent)
        res[w] = measure(R, 32 * a.segments, a.extent, dt, a.reps)
        R.close()
        for c in keep[1]:
            c.close()
        keep[0].close()
    line = json.dumps({"tool": "bench_quantile", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res})
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
