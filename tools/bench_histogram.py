#!/usr/bin/env python3
"""Value histograms (dcdf_raster_histogram_batch) against dcdf_raster_decode_batch and dcdf_raster_reduce_space_batch (count alone)
on the same cube, results and mask on the device, in-kernel time (HIP events), the calls alternated in one process:
  a  the first --segments segments of the configs[2] int32 raster (4096 x 4096, encoded on the device, opened where it lies)
  b  the same raster as float32 (values / 8, three fractional bits)
  c  a constant field of the same shape: every cell of every wave falls into one bin, the contention case of the LDS counters
For a and b: 16 and 256 bins with edges at quantiles of the data, unmasked and under a mask on the device (a disc that covers about
half the cells).  For c: 16 bins.  The decode of the same cube and reduce_space's count are the yardsticks: their code is what
it was before.  The histograms of three instants are checked against the model (tests/hist_model.py) over the decode of those
instants.  Prints ONE JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_bulk_decode import BITS, device_raster  # noqa: E402
from bench_query import SEED  # noqa: E402
from bench_reduce_space import disc  # noqa: E402

COUNT = 8


def constant_raster(segments, extent, value=1234):
    """A raster of the bench's shape whose every cell holds `value`: one constant tile on the device, encoded once per chunk."""
    from dcdf_amd import _lib as L
    from dcdf_amd.encoder import DeviceBuffer, Encoder
    from dcdf_amd.raster import EncodedRaster
    S, nt = 256, extent // 256
    tile = DeviceBuffer(32 * S * S * 4)
    tile.write(0, np.full(32 * S * S, value, dtype=np.int32))
    enc = Encoder([(tile.ptr, L.DCDF_I32, (S * S, S, 1), (32, S, S))] * (segments * nt * nt), k=2)
    enc.run()
    chunks = enc.open_chunks()
    tile.free()
    return EncodedRaster((32 * segments, extent, extent), chunks), np.dtype(np.int32), (enc, chunks)


def quantile_edges(sample, bins):
    x = np.asarray(sample).astype(np.float64).ravel()
    x = x[~np.isnan(x)]
    e = np.unique(np.quantile(x, np.linspace(0.0, 1.0, bins + 1), method="nearest"))
    if e.size < 2:  # a constant field: `bins` bins around the one value
        e = x[0] + np.arange(bins + 1, dtype=np.float64) - bins // 2
    return e


def measure(R, T, E, dt, reps, bin_counts, masked, check=True):
    import hist_model as HM
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    dec = DeviceBuffer(T * plane * dt.itemsize)
    ser = DeviceBuffer(T * 8)
    cnt = DeviceBuffer(T * 256 * 8)
    mask = disc(E)
    mbuf = DeviceBuffer(plane)
    mbuf.write(0, mask)
    zero = np.zeros(1, dtype=np.uint64)
    dmask = (mbuf.ptr, zero)
    first, _, _, _ = R.decode_flat([[0, 1, 0, E, 0, E]], dtype=dt)
    edges = {b: quantile_edges(first[:plane], b) for b in bin_counts}

    def hist(e, m=None):
        return lambda: R.histogram_flat(cube, e, masks=m, out_device_ptr=cnt.ptr, out_offset=zero)[0]

    calls = {
        "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
        "space_count": lambda: R.reduce_space_flat(cube, COUNT, out_device_ptr=ser.ptr, out_offset=zero)[0],
    }
    for b in bin_counts:
        calls["hist_%d" % b] = hist(edges[b])
        if masked:
            calls["hist_%d_masked" % b] = hist(edges[b], dmask)
    for fn in calls.values():  # warm up (code objects, pooled allocations)
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(fn())
    # exact: three instants against decode + model, every bin count, unmasked and masked
    instants = sorted({0, T // 2, T - 1})
    windows = {}
    for t in instants:
        flat, _, _, _ = R.decode_flat([[t, t + 1, 0, E, 0, E]], dtype=dt)
        windows[t] = flat[:plane].reshape(1, E, E).copy()
    stats = None
    for b in (bin_counts if check else []):
        e = edges[b]
        nb = e.size - 1
        for name, fn, m in (("", hist(e), None), ("masked", hist(e, dmask), mask)):
            fn()
            got = cnt.read(0, T * nb * 8, np.uint64).reshape(T, nb)
            for t in instants:
                assert (got[t] == HM.histogram(windows[t], e, m)[0]).all(), "%d bins %s: instant %d differs from the model" % (b, name, t)
    _, stats = R.histogram_flat(cube, edges[bin_counts[0]], out_device_ptr=cnt.ptr, out_offset=zero)
    for b in (dec, ser, cnt, mbuf):
        b.free()
    best = {k: min(v) for k, v in ms.items()}
    cells = T * plane
    return {"cells_read": cells, "decode_out_bytes": cells * dt.itemsize, "bins": {str(b): int(edges[b].size - 1) for b in bin_counts},
            "mask_selected_fraction": round(float(mask.mean()), 4) if masked else None,
            "kernel_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "best_kernel_ms": {k: round(v, 3) for k, v in best.items()},
            "spread_kernel_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
            "cells_per_s_kernel": {k: cells / (v / 1e3) for k, v in best.items()},
            "over_decode": {k: round(best[k] / best["decode"], 3) for k in best if k != "decode"},
            "over_space_count": {k: round(best[k] / best["space_count"], 3) for k in best if k.startswith("hist")},
            "stats_bulk_walk_elided": [int(x) for x in stats], "instants_checked": instants}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="abc", help="any of a, b, c")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the model: for the diagnostic builds "
                    "(K2R_HIST_VARIANT, DESIGN.md section 4h) whose counts are wrong on purpose")
    a = ap.parse_args()
    res = {}
    for w in a.workload:
        if w == "c":
            R, dt, keep = constant_raster(a.segments, a.extent)
            res[w] = measure(R, 32 * a.segments, a.extent, dt, a.reps, [16], False, not a.no_check)
        else:
            R, dt, keep = device_raster(a.segments, w == "b", a.extent)
            res[w] = measure(R, 32 * a.segments, a.extent, dt, a.reps, [16, 256], True, not a.no_check)
        R.close()
        for c in keep[1]:
            c.close()
        keep[0].close()
    print(json.dumps({"tool": "bench_histogram", "segments": a.segments, "reps": a.reps, "extent": a.extent, "checked": not a.no_check,
                      "lib": os.path.basename(os.environ.get("DCDF_K2R_LIB", "libdcdf_k2r.so")), "workloads": res}))


if __name__ == "__main__":
    main()
