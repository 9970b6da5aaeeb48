"""The case table of the SHA-256 tests: small tiles whose encoded lengths land on every tail a SHA-256 implementation can get
wrong, each with the oracle's bytes.  Pure numpy and the CPU oracle: imports neither the GPU nor the library, so the host test
(tests/test_sha_cases_host.py) can insist on the coverage the GPU test (tests/test_gpu_object_sha256.py) relies on.

A stored object is the 8-byte header HEADER followed by the Chunk::write_to bytes; with `len` the chunk's length the hashed
message has total = len + 8 bytes.  Implementations break where the padding changes shape: total % 64 in {55, 56, 63, 0, 1},
that is len % 64 in CRITICAL.  k_object_sha256 (k2r_cid.hip) also has a word-wise path for every block b > 0 that lies wholly
inside the message (64 b + 64 <= total): fast_blocks(len) of them.

  table()      -> [Case]: one tile per value of len % 64 (the first found among seeded candidates), then the named extras
  generate()   -> the same list, built afresh (table() keeps one copy for the process)
  k3_cases()   -> three tiles encoded with k = 3, on three different residues
  split_cases()-> tiles long enough to be encoded in speculative parts, one of them with a block closing early
"""
import hashlib

import numpy as np

import oracle_lib as O

HEADER = bytes([0xDC, 0xE0, 0, 0, 0, 1, 2, 4])
CID_PREFIX = bytes([0x01, 0x12, 0x12, 0x20])
CRITICAL = {47: "total % 64 == 55: the last length at which 0x80 and the bit count share the final block",
            48: "total % 64 == 56: 0x80 fits, the bit count needs one more block",
            55: "total % 64 == 63: 0x80 is the block's last byte",
            56: "total % 64 == 0: 0x80 opens a block of its own",
            57: "total % 64 == 1: one message byte spills into the last block"}
SEED = 0x5AA256
CANDIDATES = 640


def fast_blocks(length):
    """Blocks of the message that k_object_sha256 reads word-wise: every b > 0 with 64 b + 64 <= total."""
    return max(0, (length + 8) // 64 - 1)


class Case:
    """One tile: `array` with its fractional bits and rounding, `ref` the oracle's Chunk::write_to bytes (arity k)."""

    def __init__(self, name, array, bits=0, round_=False, k=2):
        self.name, self.array, self.bits, self.round, self.k = name, np.ascontiguousarray(array), bits, round_, k
        self.ref = O.chunk_build(self.array, k=k, fractional_bits=bits, round_=round_)

    @property
    def length(self):
        return len(self.ref)

    @property
    def residue(self):
        return len(self.ref) % 64

    @property
    def digest(self):
        return hashlib.sha256(HEADER + self.ref).digest()

    @property
    def cid(self):
        return CID_PREFIX + self.digest

    def key(self):
        """What two generations of the table must agree on."""
        return self.name, self.array.dtype.str, self.array.shape, self.array.tobytes(), self.bits, self.round, self.k, self.ref


def candidate(rng, i):
    """Candidate i: T = 1..8 instants of side 8 or 16, values from a few ranges, sometimes later instants that differ from
    their predecessor in a handful of cells only (short Logs: lengths move in small steps)."""
    T = int(rng.integers(1, 9))
    S = int(rng.choice([8, 16]))
    span = int(rng.choice([2, 16, 300, 70000, 1 << 20]))
    a = rng.integers(-span, span, size=(T, S, S))
    if rng.random() < 0.5:
        for t in range(1, T):
            a[t] = a[t - 1]
            for _ in range(int(rng.integers(0, 6))):
                a[t, rng.integers(S), rng.integers(S)] += rng.integers(-span, span)
    return Case("cand%03d-%dx%dx%d-span%d" % (i, T, S, S, span), a.astype(np.int32))


def residue_cases():
    """The first candidate found for each value of len % 64, in order of residue."""
    rng = np.random.default_rng(SEED)
    first = {}
    for i in range(CANDIDATES):
        c = candidate(rng, i)
        first.setdefault(c.residue, c)
    return [first[r] for r in sorted(first)]


def one_fast_block():
    """A chunk with exactly one word-wise block (128 <= total < 192): one instant, side 8, a few cells set."""
    rng = np.random.default_rng(SEED + 1)
    for i in range(200):
        a = np.zeros((1, 8, 8), dtype=np.int32)
        for _ in range(1 + i % 24):
            a[0, rng.integers(8), rng.integers(8)] = rng.integers(1, 200)
        c = Case("one-fast-block-%d" % i, a)
        if fast_blocks(c.length) == 1:
            return c
    raise AssertionError("no chunk with exactly one word-wise block among the candidates")


def extras():
    from dcdf_amd import synth
    rng = np.random.default_rng(SEED + 2)
    out = [Case("uniform-1x8x8", np.zeros((1, 8, 8), dtype=np.int32) + 7),          # the shortest chunk there is
           one_fast_block(),
           Case("noise-1x64x64", rng.integers(-(1 << 29), 1 << 29, size=(1, 64, 64)).astype(np.int32)),
           Case("synth-2x256x256", synth.cells(0xDCDF0005, 0, 2, 0, 256, 0, 256, np.int32)),
           Case("int64-3x16x16", rng.integers(-(1 << 40), 1 << 40, size=(3, 16, 16)).astype(np.int64))]
    for dtype in (np.float32, np.float64):                                           # fractional bits, one NaN
        f = (rng.integers(-4000, 4000, size=(3, 16, 16)) / 8.0).astype(dtype)
        f[1, 5, 9] = np.nan
        out.append(Case("%s-3x16x16-nan" % np.dtype(dtype).name, f, bits=3))
    return out


def generate():
    return residue_cases() + extras()


_table = None


def table():
    global _table
    if _table is None:
        _table = generate()
    return _table


def k3_cases():
    """Three small tiles for the universal kernel at k = 3 (sidelen 9 and 27), the first three candidates on pairwise different
    residues."""
    rng = np.random.default_rng(SEED + 3)
    out = []
    for i in range(40):
        T, S = int(rng.integers(1, 5)), int(rng.choice([9, 20]))
        c = Case("k3-%d-%dx%dx%d" % (i, T, S, S), rng.integers(-300, 300, size=(T, S, S)).astype(np.int32), k=3)
        if all(c.residue != o.residue for o in out):
            out.append(c)
        if len(out) == 3:
            return out
    raise AssertionError("fewer than three residues among the k = 3 candidates")


def split_cases():
    """Tiles long enough to be encoded in speculative parts (K2R_SPLIT=all), as test_speculative_parts_splice builds them: two
    synthetic [32, 256, 256] chunks, one with a Snapshot inside the first half (a block closes early: the parts do not splice and
    the tile is re-encoded whole), one with block boundaries in the second half only."""
    from dcdf_amd import synth
    a = synth.cells(0xDCDF0003, 0, 32, 0, 256, 0, 256, np.int32)
    b = synth.cells(0xDCDF0003, 32, 64, 768, 1024, 0, 256, np.int32)
    early = a.copy()
    early[5] = np.random.default_rng(5).integers(0, 1 << 20, size=early[5].shape)
    late = b.copy()
    late[20:] = np.random.default_rng(6).integers(0, 1 << 20, size=late[20:].shape)
    return [Case("split-synth-a", a), Case("split-synth-b", b), Case("split-early-close", early), Case("split-late-noise", late)]
