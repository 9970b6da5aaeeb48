#!/usr/bin/env python3
"""Regression over time (dcdf_raster_regress_time_batch, dcdf_raster_regress_time_groups_batch) against the calls next to it, on one
cube over the first --segments segments of the configs[2] raster (4096 x 4096; int32, and float32 = values / 8), results left on
the device, in-kernel time (HIP events).  The variants are alternated --reps times after a warm-up, best of the repetitions,
every repetition kept:
  regress_all / regress_slope   regress_time_flat with all four planes, and with the slope alone, against the instant index
  regress_clim                  all four planes under the labels i % 7
  regress_own                   the slope alone, every instant its own group (a group of one value: NaN -- the cost of the planes)
  decode                        decode_flat of the same cube in the raster's own dtype
  moments_all                   moments_time_flat with all four planes
  median                        quantile_time_flat, p = 0.5
The one expectation: the median reads the slab several times and the regression once, so regress_all above the median of the same
run is an error (asserted).  slab_copy: a device-to-device copy of as many bytes as the cube's slab holds (8 a value), in pieces of
the slab's cap, what reading the slab once and writing it once costs at the least.  Three row bands of regress_all and regress_clim
are compared bit for bit with decode plus the model of tests/regress_model.py.  Prints ONE JSON line and writes it to
profiles/regress_bench.json."""
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

SLOPE, ALL = 2, 15
SLAB_BYTES = int(os.environ.get("K2R_QUANTILE_SLAB_BYTES") or 0) or 256 << 20  # the cap of one band as the calls of this run read it


def slab_copy_ms(total_bytes, reps):
    """best time of device-to-device copies adding up to total_bytes, in pieces of the slab's cap, between two HIP events on the
    null stream (the HIP runtime the library itself is linked with, through ctypes)"""
    import ctypes as C
    from dcdf_amd.encoder import DeviceBuffer
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc

    src, dst = DeviceBuffer(SLAB_BYTES), DeviceBuffer(SLAB_BYTES)
    src.write(0, np.zeros(SLAB_BYTES // 8, dtype=np.int64))
    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    n = max(1, total_bytes // SLAB_BYTES)
    best = None
    for _ in range(reps + 1):
        ok(hip.hipEventRecord(e0, None))
        for _ in range(n):
            ok(hip.hipMemcpyAsync(C.c_void_p(dst.ptr), C.c_void_p(src.ptr), C.c_size_t(SLAB_BYTES), 3, None))  # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        scaled = ms.value * total_bytes / (n * SLAB_BYTES)
        best = scaled if best is None else min(best, scaled)
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))
    src.free()
    dst.free()
    return round(best, 3)


def measure(R, T, E, dt, reps, band_rows=64):
    import regress_model as RM
    from dcdf_amd.encoder import DeviceBuffer
    cube = np.array([[0, T, 0, E, 0, E]], dtype=np.uint32)
    plane = E * E
    zero = np.zeros(1, dtype=np.uint64)
    i = np.arange(T)
    out = DeviceBuffer(max(4 * 7, T) * plane * 8)  # the largest result: 28 planes, or one per instant
    dec = DeviceBuffer(T * plane * dt.itemsize)
    clim, own = (i % 7).astype(np.uint16), i.astype(np.uint16)

    def regress(ops, lab=None, n=None):
        if lab is None:
            return lambda: R.regress_time_flat(cube, ops, out_device_ptr=out.ptr, out_offset=zero)[0]
        return lambda: R.regress_time_groups_flat(cube, ops, [lab], n, out_device_ptr=out.ptr, out_offset=zero)[0]

    res = alternate({"regress_all": regress(ALL), "regress_slope": regress(SLOPE), "regress_clim": regress(ALL, clim, 7),
                     "regress_own": regress(SLOPE, own, T),
                     "decode": lambda: R.decode_flat(cube, dtype=dt, out_device_ptr=dec.ptr, out_offset=zero)[0],
                     "moments_all": lambda: R.moments_time_flat(cube, 15, 1, out_device_ptr=out.ptr, out_offset=zero)[0],
                     "median": lambda: R.quantile_time_flat(cube, [0.5], "linear", out_device_ptr=out.ptr, out_offset=zero)[0]}, reps)
    best = {k: min(v) for k, v in res.items()}
    assert best["regress_all"] <= best["median"], "the regression (one read of the slab) is slower than the median (several): %r" % (best,)
    ratios = {"%s_over_%s" % (m, k): round(best[m] / best[k], 3) for m in ("regress_all", "regress_slope", "regress_clim", "regress_own")
              for k in ("decode", "moments_all", "median")}
    # bit for bit: three row bands of the plain and the clim call against decode + model
    bands = sorted({0, (E // 2 // band_rows) * band_rows, E - band_rows})
    e = np.arange(T, dtype=np.float64)
    for grouped in (False, True):
        (regress(ALL, clim, 7) if grouped else regress(ALL))()
        n_groups = 7 if grouped else 1
        for r0 in bands:
            flat, _, _, _ = R.decode_flat([[0, T, r0, r0 + band_rows, 0, E]], dtype=dt)
            a = flat[:T * band_rows * E].reshape(T, band_rows, E)
            want = RM.regress_time_groups(a, e, clim, 7) if grouped else {n: v[None] for n, v in RM.regress_time(a, e).items()}
            for k, name in enumerate(RM.NAMES):
                for g in range(n_groups):
                    got = out.read(((k * n_groups + g) * plane + r0 * E) * 8, band_rows * E * 8, np.uint64)
                    assert np.array_equal(got, RM.bits(want[name][g]).ravel()), "%s of group %d differs in the band at row %d" % (name, g, r0)
    _, stats = R.regress_time_flat(cube, ALL, out_device_ptr=out.ptr, out_offset=zero)
    out.free()
    dec.free()
    copy = slab_copy_ms(T * plane * 8, reps)
    return {"cells_read": T * plane, "kernel_ms": res, "best_kernel_ms": best, "ratios": ratios, "slab_bytes": T * plane * 8, "slab_copy_ms": copy,
            "regress_all_minus_decode_ms": round(best["regress_all"] - best["decode"], 3), "stats_bulk_walk_elided": [int(v) for v in stats],
            "bands_checked_rows": bands}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab", help="any of a (int32), b (float32)")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extent", type=int, default=4096, help="rows = cols of the raster (a multiple of 256)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regress_bench.json"))
    a = ap.parse_args()
    res = {}
    for w in a.workload:
        R, dt, keep = device_raster(a.segments, w == "b", a.extent)
        res[{"a": "int32", "b": "float32"}[w]] = measure(R, 32 * a.segments, a.extent, dt, a.reps)
        R.close()
        for c in keep[1]:
            c.close()
        keep[0].close()
    line = json.dumps({"tool": "bench_regress", "segments": a.segments, "reps": a.reps, "extent": a.extent, "workloads": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
