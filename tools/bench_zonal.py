#!/usr/bin/env python3
"""Zonal statistics (dcdf_raster_zonal_batch) against dcdf_raster_decode_batch and dcdf_raster_reduce_space_batch on the same cube:
the first --segments segments of the configs[2] int32 raster (4096 x 4096, encoded on the device, opened where it lies), labels and
results on the device, in-kernel time (HIP events), the calls alternated in one process.  Four label rasters:
  a  one zone everywhere
  b  a grid of 64 x 64 blocks: 4096 zones, one per unit of the bulk kernel
  c  a grid of 100 x 100 blocks: 1681 zones that straddle the units, 1 to 4 zones in a unit
  d  300 Voronoi-like zones from a fixed seed (nearest of 300 seeds on a 1024 x 1024 grid, each grid cell 4 x 4 raster cells)
For each: zonal with all five statistics; the decode of the same cube; reduce_space, all five, unmasked and under one zone's mask;
and min(Z, 8) masked reduce_space calls, one per zone, extrapolated to the Z calls the zones cost without zonal.  Checked bit for
bit: the rows of up to 8 zones equal reduce_space under the zone's mask at every instant, and the counts of all zones add up to
the unmasked count.  Prints ONE JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_bulk_decode import device_raster  # noqa: E402

ALL = 31


def label_rasters(E):
    r, c = np.arange(E)[:, None], np.arange(E)[None, :]
    g = -(-E // 100)
    out = {"a": np.zeros((E, E), dtype=np.uint16), "b": ((r // 64) * (E // 64) + c // 64).astype(np.uint16), "c": ((r // 100) * g + c // 100).astype(np.uint16)}
    rng = np.random.default_rng(2025)
    n = E // 4
    seeds = rng.random((300, 2)) * n
    best, lab = np.full((n, n), np.inf), np.zeros((n, n), dtype=np.uint16)
    y, x = np.arange(n)[:, None] + 0.5, np.arange(n)[None, :] + 0.5
    for z, (sy, sx) in enumerate(seeds):
        d = (y - sy) ** 2 + (x - sx) ** 2
        near = d < best
        best[near], lab[near] = d[near], z
    out["d"] = np.ascontiguousarray(np.repeat(np.repeat(lab, 4, axis=0), 4, axis=1))
    return out


def measure(R, T, E, dt, labels, reps):
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    Z = int(labels.max()) + 1
    some = sorted({0, Z // 2, Z - 1} | set(range(min(Z, 8))))[:8]
    dec = DeviceBuffer(T * plane * dt.itemsize)
    ser = DeviceBuffer(5 * T * 8)
    mat = DeviceBuffer(5 * Z * T * 8)
    lbuf = DeviceBuffer(plane * 2)
    lbuf.write(0, labels)
    mbufs = []
    for z in some:
        m = DeviceBuffer(plane)
        m.write(0, (labels == z).astype(np.uint8))
        mbufs.append(m)
    zero = np.zeros(1, dtype=np.uint64)
    calls = {
        "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
        "space_all": lambda: R.reduce_space_flat(cube, ALL, out_device_ptr=ser.ptr, out_offset=zero)[0],
        "space_all_one_mask": lambda: R.reduce_space_flat(cube, ALL, masks=(mbufs[0].ptr, zero), out_device_ptr=ser.ptr, out_offset=zero)[0],
        "space_all_masks": lambda: sum(R.reduce_space_flat(cube, ALL, masks=(m.ptr, zero), out_device_ptr=ser.ptr, out_offset=zero)[0] for m in mbufs),
        "zonal_all": lambda: R.zonal_flat(cube, ALL, (lbuf.ptr, zero), Z, out_device_ptr=mat.ptr, out_offset=zero)[0],
    }
    for fn in calls.values():  # warm up (code objects, pooled allocations)
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(fn())
    # bit for bit: the zones of `some` against reduce_space under their masks; the zones' counts against the unmasked count
    _, stats = R.zonal_flat(cube, ALL, (lbuf.ptr, zero), Z, out_device_ptr=mat.ptr, out_offset=zero)
    got = mat.read(0, 5 * Z * T * 8, np.float64).reshape(5, Z, T)
    for z, m in zip(some, mbufs):
        R.reduce_space_flat(cube, ALL, masks=(m.ptr, zero), out_device_ptr=ser.ptr, out_offset=zero)
        want = ser.read(0, 5 * T * 8, np.float64).reshape(5, T)
        assert (np.ascontiguousarray(got[:, z, :]).view(np.uint64) == want.view(np.uint64)).all(), "zone %d differs from reduce_space under its mask" % z
    R.reduce_space_flat(cube, ALL, out_device_ptr=ser.ptr, out_offset=zero)
    whole = ser.read(0, 5 * T * 8, np.float64).reshape(5, T)
    assert (got[3].sum(0) == whole[3]).all(), "the zones' counts do not add up to the cube's"
    for b in [dec, ser, mat, lbuf] + mbufs:
        b.free()
    best = {k: min(v) for k, v in ms.items()}
    best["space_all_Z_masks_extrapolated"] = best["space_all_masks"] / len(some) * Z
    cells = T * plane
    return {"zones": Z, "cells_read": cells, "zonal_out_bytes": 5 * Z * T * 8, "masks_measured": len(some),
            "kernel_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "best_kernel_ms": {k: round(v, 3) for k, v in best.items()},
            "spread_kernel_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
            "zonal_over": {k: round(best["zonal_all"] / best[k], 4) for k in best if k not in ("zonal_all", "space_all_masks")},
            "stats_bulk_walk_elided": [int(x) for x in stats], "zones_checked": some}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", default="abcd", help="any of a, b, c, d")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    a = ap.parse_args()
    labels = label_rasters(a.extent)
    R, dt, keep = device_raster(a.segments, False, a.extent)
    res = {w: measure(R, 32 * a.segments, a.extent, dt, labels[w], a.reps) for w in a.labels}
    R.close()
    for c in keep[1]:
        c.close()
    keep[0].close()
    print(json.dumps({"tool": "bench_zonal", "segments": a.segments, "reps": a.reps, "extent": a.extent, "dtype": "int32", "labels": res}))


if __name__ == "__main__":
    main()
