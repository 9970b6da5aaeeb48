#!/usr/bin/env python3
"""Bulk decode (dcdf_raster_decode_batch) against fill_windows_flat on the same cubes, results left on the device, in-kernel time
(HIP events) and wall time of the call:
  a  whole-segment cubes over the first --segments segments of the configs[2] int32 raster (4096 x 4096, encoded on the device,
     opened where it lies)
  b  the same raster as float32 (values / 8, three fractional bits)
  c  the stored-raster model of tools/bench_stored_raster.py (64 x 2304 x 2304 int32 through Dataset.append, about a quarter of
     the tiles elided)
Every workload checks a few bands of both results against each other bit for bit.  --baseline-only times fill_windows_flat alone:
that form also runs against a library built from an earlier commit (DCDF_K2R_LIB), which is how the two are alternated.
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

from bench_query import SEED  # noqa: E402

BITS = 3


def device_raster(segments, as_float, extent=4096):
    """The bench.py raster (first `segments` segments) encoded on the device from int32 or float32 tiles, opened from device
    memory.  Returns (EncodedRaster, numpy dtype, things to keep alive)."""
    from dcdf_amd import _lib as L
    from dcdf_amd.encoder import DeviceBuffer, Encoder, synth_fill
    from dcdf_amd.raster import EncodedRaster
    S, nt = 256, extent // 256
    grid = [(seg, i, j) for seg in range(segments) for i in range(nt) for j in range(nt)]
    n = 32 * S * S
    flat = DeviceBuffer(len(grid) * n * 4)
    descs = []
    for g, (seg, i, j) in enumerate(grid):
        ptr = flat.ptr + g * n * 4
        synth_fill(ptr, L.DCDF_I32, SEED, 32 * seg, 32 * seg + 32, S * i, S * i + S, S * j, S * j + S)
        descs.append((ptr, L.DCDF_F32, (S * S, S, 1), (32, S, S), BITS, False) if as_float else (ptr, L.DCDF_I32, (S * S, S, 1), (32, S, S)))
    if as_float:  # the same cells / 8 as float32, converted in place a slab at a time
        slab = 64 * n
        for o in range(0, len(grid) * n, slab):
            m = min(slab, len(grid) * n - o)
            flat.write(o * 4, (flat.read(o * 4, m * 4, np.int32) / 8.0).astype(np.float32))
    enc = Encoder(descs, k=2)
    enc.run()
    chunks = enc.open_chunks()
    flat.free()
    return EncodedRaster((32 * segments, extent, extent), chunks), np.dtype(np.float32 if as_float else np.int32), (enc, chunks)


def measure(R, cubes, dt, reps, baseline_only, check_bands=3):
    from dcdf_amd.encoder import DeviceBuffer
    cubes = np.ascontiguousarray(np.asarray(cubes, dtype=np.uint32).reshape(-1, 6))
    vol = ((cubes[:, 1] - cubes[:, 0]).astype(np.uint64) * (cubes[:, 3] - cubes[:, 2]) * (cubes[:, 5] - cubes[:, 4]))
    off = np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64)
    cells = int(vol.sum())
    out = DeviceBuffer(cells * dt.itemsize)
    res = {"cells": cells, "out_bytes": cells * dt.itemsize}

    def timed(fn):
        ks, ws = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            k = fn()
            ws.append(time.perf_counter() - t0)
            ks.append(k)
        return ks, ws

    fn_fill = lambda: R.fill_windows_flat(cubes, dtype=dt, out_device_ptr=out.ptr, out_offset=off)
    fn_fill()  # warm up (allocations)
    ks, ws = timed(fn_fill)
    res["fill_window"] = {"kernel_ms": [round(k, 3) for k in ks], "best_kernel_ms": round(min(ks), 3), "cells_per_s_kernel": cells / (min(ks) / 1e3),
                          "best_wall_s": round(min(ws), 4)}
    band = int(cubes[0, 3] - cubes[0, 2]) * int(cubes[0, 5] - cubes[0, 4])
    picks = sorted({0, int(vol[0]) // band // 2, int(vol[0]) // band - 1})[:check_bands]
    want = [out.read(p * band * dt.itemsize, band * dt.itemsize, np.uint8) for p in picks]
    if not baseline_only:
        stats = [None]

        def fn_dec():
            ms, stats[0] = R.decode_flat(cubes, dtype=dt, out_device_ptr=out.ptr, out_offset=off)
            return ms
        out.write(0, np.zeros(min(cells * dt.itemsize, 1 << 20), dtype=np.uint8))
        fn_dec()
        for p, w in zip(picks, want):
            assert np.array_equal(out.read(p * band * dt.itemsize, band * dt.itemsize, np.uint8), w), "decode differs from fill_window in band %d" % p
        ks, ws = timed(fn_dec)
        res["decode"] = {"kernel_ms": [round(k, 3) for k in ks], "best_kernel_ms": round(min(ks), 3), "cells_per_s_kernel": cells / (min(ks) / 1e3),
                         "out_GBps_kernel": round(cells * dt.itemsize / (min(ks) / 1e3) / 1e9, 1), "best_wall_s": round(min(ws), 4),
                         "stats_bulk_walk_elided": [int(x) for x in stats[0]]}
        res["decode_over_fill_window"] = round(res["fill_window"]["best_kernel_ms"] / res["decode"]["best_kernel_ms"], 3)
    out.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="abc", help="any of a, b, c")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    E = 4096
    res = {}
    for w in a.workload:
        if w in "ab":
            R, dt, keep = device_raster(a.segments, w == "b", E)
            cubes = [[32 * s, 32 * s + 32, 0, E, 0, E] for s in range(a.segments)]
            res[w] = measure(R, cubes, dt, a.reps, a.baseline_only)
            R.close()
            for c in keep[1]:
                c.close()
            keep[0].close()
        elif w == "c":
            from bench_stored_raster import stored_variable
            v, src, n_uniform = stored_variable("int32", 64, 2304)
            del src
            R = v.raster()
            res[w] = measure(R, [[0, 32, 0, 2304, 0, 2304], [32, 64, 0, 2304, 0, 2304]], np.dtype(np.int32), a.reps, a.baseline_only)
            res[w]["elided_leaves"] = sum(t.chunk is None for t in R.tiles)
    from dcdf_amd import _lib as L
    print(json.dumps({"tool": "bench_bulk_decode", "library": os.path.basename(os.path.dirname(L.LIB_PATH)) + "/" + os.path.basename(L.LIB_PATH),
                      "segments": a.segments, "reps": a.reps, "baseline_only": a.baseline_only, "workloads": res}))


if __name__ == "__main__":
    main()
