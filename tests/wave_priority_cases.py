"""Tiles for the wave priorities of the encoder (k2r_exec.h: prio; k2r_encode.h: the lean phase 1).  A priority moves WHEN a wave
issues, never what it computes -- unless a phase already depended on timing.  The places where that could be are the groups of
phases with no barrier between them around phase 1: the tail of one instant's emission, the replay of the top nodes' second bytes
and the zeroing of the bitmaps run into the next instant's phase 1.  A tile of four instants -- one Snapshot, a Log after the
Snapshot, a Log after a Log, twice -- is the smallest that crosses them twice with a Log on both sides.

  * the sidelen-256 int32 tiles of tests/wave_balance_cases.py (every record count and placement), a fourth instant appended:
    sidelen 256 is the only workgroup with several waves on a SIMD, so the only kernel a priority is emitted for;
  * two tiles of the model raster (the benchmark's data), the float32 and int64 views of the first;
  * one sidelen-128 tile, whose kernel holds no priority instruction at all.

Pure numpy; tests/test_gpu_wave_priority.py runs the table on the card, tests/test_wave_priority_host.py part of it through the
host simulator."""
import numpy as np

import wave_balance_cases as W
from dcdf_amd import synth

INSTANTS = 4
FBITS = 3  # the float view stores exact multiples of 2^-3: its stored integers are the int32 tile's
SEED = 0xDCDF0003
MODEL_TILES = ((0, 0), (1, 2))  # (tile row, tile column) of the model raster, instants 0..3


def four(a):
    """[3, S, S] -> [4, S, S]: instant 1 again after instant 2 (a Log against the same Snapshot, after another Log)."""
    return np.ascontiguousarray(a[[0, 1, 2, 1]])


def model(i, j, dtype=np.int32):
    return synth.cells(SEED, 0, INSTANTS, 256 * i, 256 * i + 256, 256 * j, 256 * j + 256, dtype)


_tiles = None


def tiles():
    """[(name, array [4, S, S], fractional bits, row loader of the fused kernel)]"""
    global _tiles
    if _tiles is None:
        out = [(c.name + "-int32", four(c.array), 0, 1) for c in W.cases() if c.array.shape[1] == 256 and c.array.shape[0] == 3]
        m = [model(i, j) for i, j in MODEL_TILES]
        out += [("model-%d-%d-int32" % ij, a, 0, 1) for ij, a in zip(MODEL_TILES, m)]
        out.append(("model-0-0-float32", (m[0].astype(np.float64) / 2.0 ** FBITS).astype(np.float32), FBITS, 2))
        out.append(("model-0-0-int64", m[0].astype(np.int64), 0, 3))
        out.append(("S128-int32", four(W.case("S128").array), 0, 1))
        for _, a, _, _ in out:
            assert a.shape[0] == INSTANTS and a.shape[1] == a.shape[2]
        _tiles = out
    return _tiles
