"""A numpy model of the bulk decoder's rule, for the tests: parse one chunk's serialized bytes, decode
each block's Snapshot ONCE into a max-pyramid (level l = the Snapshot's own max of every node of side 2^l, a leaf's value repeated
below it), then decode every Log of the block from its own tree alone (T, eqB, Lmax): a uniform leaf at level l is d + P[l][node],
an "equal" leaf or a cell is d + P[0][cell].  Lmin is never read.  Also the array the leaf-kind tests are built on."""
import struct

import numpy as np

from dcdf_amd.dataset import _dac_values

SEED = 0xDCDF0011


def _bitmap(buf, pos):  # bitmap.rs:142-164: length, index stride, rank index, words (MSB first)
    nbits, k = struct.unpack_from(">II", buf, pos)
    pos += 8 + 4 * (nbits // 32 // k)
    nw = (nbits + 31) // 32
    bits = np.unpackbits(np.frombuffer(buf, dtype=np.uint8, count=4 * nw, offset=pos))[:nbits].astype(np.int64)
    return bits, pos + 4 * nw


def parse_chunk(buf):
    """[blocks], each [(T, E or None, Lmax, sidelen, rows, cols)] per instant (chunk.rs:247-266, block.rs:99-109)."""
    pos = 2
    (n_blocks,) = struct.unpack_from(">I", buf, pos)
    pos += 4
    blocks = []
    for _ in range(n_blocks):
        n_inst = buf[pos]
        pos += 1
        insts = []
        for i in range(n_inst):
            k, rows, cols, sidelen = struct.unpack_from(">BIII", buf, pos)
            assert k == 2
            pos += 13
            T, pos = _bitmap(buf, pos)
            E = None
            if i > 0:
                E, pos = _bitmap(buf, pos)
            mx, pos = _dac_values(buf, pos)
            _, pos = _dac_values(buf, pos)  # Lmin: skipped
            insts.append((T, E, mx, sidelen, rows, cols))
        blocks.append(insts)
    assert pos == len(buf)
    return blocks


def _children(idx, T):
    """For parents with first-child index idx (shape [n, n], -1 = none): (child index i [2n, 2n] or -1, T bit, rank1(T, i))."""
    n = idx.shape[0]
    i = np.repeat(np.repeat(idx, 2, axis=0), 2, axis=1)
    c = (np.arange(2 * n)[:, None] % 2) * 2 + np.arange(2 * n)[None, :] % 2  # child order i * k + j (snapshot.rs:468-474)
    i = np.where(i >= 0, i + c, -1)
    rank = np.concatenate([[0], np.cumsum(T)])
    inside = (i >= 0) & (i < len(T))
    safe = np.where(inside, i, 0)
    return i, np.where(inside, T[safe], 0), rank[safe]


def snapshot_pyramid(T, mx, sidelen):
    """P[l] = [sidelen >> l, sidelen >> l] values, l = 0 .. log2(sidelen), filled top-down from the tree."""
    top = sidelen.bit_length() - 1
    P = {top: np.array([[mx[0]]], dtype=np.int64)}
    idx = np.array([[1 if T[0] else -1]], dtype=np.int64)
    for l in range(top, 0, -1):
        i, bit, rank = _children(idx, T)
        up = np.repeat(np.repeat(P[l], 2, axis=0), 2, axis=1)
        P[l - 1] = np.where(i >= 0, up - mx[np.where(i >= 0, i, 0)], up)
        idx = np.where(bit == 1, 1 + rank * 4, -1)
    return P


def log_decode(T, E, mx, sidelen, P):
    """The Log's own tree alone over the pyramid.  State per node: open (first-child index) or resolved (d, source level)."""
    top = sidelen.bit_length() - 1
    d = np.array([[mx[0]]], dtype=np.int64)
    if T[0]:
        idx, lev = np.array([[1]], dtype=np.int64), np.array([[-1]], dtype=np.int64)
    else:  # the root shortcuts (log.rs:315-327): the same rule at the root
        idx, lev = np.array([[-1]], dtype=np.int64), np.array([[0 if E[0] else top]], dtype=np.int64)
    for l in range(top, 0, -1):
        i, bit, rank = _children(idx, T)
        opened = i >= 0
        safe = np.where(opened, i, 0)
        d = np.where(opened, mx[safe], np.repeat(np.repeat(d, 2, axis=0), 2, axis=1))
        lev_up = np.repeat(np.repeat(lev, 2, axis=0), 2, axis=1)
        cells = opened & (i >= len(T))
        Ep = E if len(E) else np.zeros(1, dtype=np.int64)  # (a Log without leaves above the cells has an empty eqB)
        eq = np.where(opened & ~cells & (bit == 0), Ep[np.clip(safe - rank, 0, len(Ep) - 1)], 1)  # eqB: one bit per T = 0 node
        lev = np.where(opened, np.where(bit == 1, -1, np.where(eq == 1, 0, l - 1)), lev_up)
        idx = np.where(opened & (bit == 1), 1 + rank * 4, -1)
    assert (lev >= 0).all()
    out = np.zeros((sidelen, sidelen), dtype=np.int64)
    r, c = np.indices((sidelen, sidelen))
    for l in range(top + 1):
        m = lev == l
        out[m] = d[m] + P[l][r[m] >> l, c[m] >> l]
    return out


def decode_chunk(buf):
    """[instants, rows, cols] int64 stored values of a serialized k = 2 chunk, block by block."""
    out = []
    for insts in parse_chunk(bytes(buf)):
        T, _, mx, sidelen, rows, cols = insts[0]
        P = snapshot_pyramid(T, mx, sidelen)
        out.append(P[0][:rows, :cols])
        for T, E, mx, sidelen, rows, cols in insts[1:]:
            out.append(log_decode(T, E, mx, sidelen, P)[:rows, :cols])
    return np.stack(out)


def leaf_kinds_array(rng):
    """[40, 256, 256] int64, five forced blocks of eight instants (instants 0, 8, 16, 24, 32 are Snapshots, the others Logs):
    every leaf kind of the Log rule."""
    a = np.zeros((40, 256, 256), dtype=np.int64)
    s0 = rng.integers(0, 500, size=(256, 256))
    s0[0:64, 64:128] = 77          # uniform 64 x 64 and 16 x 16 squares of the Snapshot (leaves above the cells)
    s0[128:144, 16:32] = 5
    s0[192:256, 192:256] = 300
    sparse = lambda p, lo, hi: np.where(rng.random((256, 256)) < p, rng.integers(lo, hi, size=(256, 256)), 0)
    a[0] = s0
    a[1] = s0                       # equal to its Snapshot: single-node Log, eqB[0] = 1
    a[2] = s0 + 13                  # the Snapshot plus a constant
    a[3] = 321                      # uniform over the whole tile: single-node Log, eqB[0] = 0
    a[4] = s0
    a[4, 32:96, 32:160] = 250       # one constant over a varied Snapshot: uniform, not "equal" leaves at several levels
    a[4, 200:204, 200:202] = 9
    a[4, 100:116, 240:256] = -7
    a[5] = s0 + sparse(0.05, -20, 20)   # a varied Log over the Snapshot's uniform squares too (Snapshot leaf above, Log continues)
    a[6] = s0
    a[6, 10:20, 10:30] += 40000     # differences of three Dac bytes (zig-zag > 65535), values far inside +-2^30
    a[6, 100, 100] -= 70000
    a[6, 70:75, 70:90] += 9000000   # and four
    a[7] = s0 + rng.integers(-30, 30, size=(256, 256))
    n8 = rng.integers(-1000, 1000, size=(256, 256))
    a[8] = n8                       # a noise Snapshot
    a[9] = rng.integers(-1000, 1000, size=(256, 256))
    a[10] = n8
    a[10, 64:128, 0:64] = 0
    a[10, 3:5, 7:9] = 1
    a[11] = n8
    a[12] = -5
    a[13] = n8 - 100000
    a[14] = n8 + sparse(0.01, -70000, 70000)
    a[15] = n8 + sparse(0.3, -3, 3)
    a[16] = 42                      # a single-node Snapshot under varied Logs
    a[17] = 42 + sparse(0.05, -9, 9)
    a[18] = rng.integers(0, 2000, size=(256, 256))
    a[19] = 42
    a[20] = 50
    a[21] = 42
    a[21, 16:48, 80:144] = 7
    a[22] = 42 + sparse(0.002, -100000, 100000)
    a[23] = 42
    a[23, 255, 255] = 43
    blocks = np.repeat(np.repeat(rng.integers(0, 50, size=(4, 4)), 64, axis=0), 64, axis=1)
    a[24] = blocks                  # a Snapshot of 64 x 64 leaves, some refined
    a[24, 64:80, 64:80] = 900
    a[24, 130, 131] = 1
    a[25] = blocks + sparse(0.05, -5, 5)
    a[26] = blocks + 1
    a[27] = blocks
    a[27, 0:128, 128:256] = 11
    a[28] = a[24] + sparse(0.5, -2, 2)
    a[29] = a[24]
    a[30] = a[24]
    a[30, 64:80, 64:80] = 901
    a[31] = 0
    from dcdf_amd import synth
    a[32:40] = synth.cells(SEED, 100, 108, 0, 256, 0, 256, np.int32)
    return a
