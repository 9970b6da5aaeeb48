"""Tiles for the emission of stash Logs (k2r_encode.h: the straight-line pass A of the nodes of heights >= 3, the 4-byte store
of a record's second bytes, the per-value stores of every other group), and the proof that they reach what grouped forms of
that emission can get wrong.  Pure numpy: the host test (simulator against the oracle) and the GPU test (device views against
the oracle) walk the same table.

  cases()        -> [Case]: `array` int32 [T, S, S], unpadded; instant 0 is the Snapshot, every later instant a narrow Log
  coverage(a)    -> what the Logs of one array contain, restated from log.rs:112-165 on arrays (no encoder involved)
  check_table()  -> raises AssertionError where the table misses a condition (a fault of the table, never a skip)

What a Log stores (k = 2, unpadded): breadth first from the root, Lmax = max_t - max_s of every visited node; a node with
children is internal (T = 1, its Lmin = min_t - min_s stored, its children visited) unless it is uniform at t or all its
cells differ from the snapshot by one constant ("equal").  Within a height the visited nodes come in Morton order, four
children per internal parent, so the Lmax values of a parent's children and the Lmin values of its internal children are
adjacent in their streams: the groups the encoder emits together.  A value is "long" when its zigzag code needs a second
byte; the second bytes of a Dac are stored in stream order.

The conditions are asserted over the table as a whole (S = 16 has four height-2 groups per instant: no single small tile
can hold all of them); the overflow case has to meet its own on its own."""
import zlib

import numpy as np


def seeded(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def zigzag(v):
    v = v.astype(np.int64)
    return (v << 1) ^ (v >> 63)


def morton_perm(n):
    """perm[code] = r * n + c of the n x n grid in the order the tree visits it (child 2 i + j: row bit above column bit)."""
    r = np.arange(n)[:, None] * np.ones((1, n), dtype=np.int64)
    c = np.arange(n)[None, :] * np.ones((n, 1), dtype=np.int64)
    code = np.zeros((n, n), dtype=np.int64)
    b = 0
    while (1 << b) < n:
        code |= ((c >> b) & 1) << (2 * b)
        code |= ((r >> b) & 1) << (2 * b + 1)
        b += 1
    perm = np.empty(n * n, dtype=np.int64)
    perm[code.reshape(-1)] = np.arange(n * n)
    return perm


def blocks(a2, h, fn):
    """fn over the 2^h x 2^h blocks of a square array, in Morton order."""
    S = a2.shape[0]
    n, b = S >> h, 1 << h
    v = fn(a2.reshape(n, b, n, b), axis=(1, 3))
    return v.reshape(-1)[morton_perm(n)]


class LogStreams:
    """The streams of Log::build(snapshot s2, instant t2), per height H..0: visited / internal flags (Morton order) and the
    zigzag codes of the Lmax / Lmin values."""

    def __init__(self, s2, t2):
        S = s2.shape[0]
        H = S.bit_length() - 1
        assert s2.shape == t2.shape == (S, S) and 1 << H == S
        s2, t2 = s2.astype(np.int64), t2.astype(np.int64)
        d = t2 - s2
        self.H = H
        self.visited, self.internal, self.zmax, self.zmin = {}, {}, {}, {}
        for h in range(H, -1, -1):
            mx_t, mn_t = blocks(t2, h, np.max), blocks(t2, h, np.min)
            mx_s, mn_s = blocks(s2, h, np.max), blocks(s2, h, np.min)
            equal = blocks(d, h, np.max) == blocks(d, h, np.min)
            vis = np.ones(1, dtype=bool) if h == H else np.repeat(self.internal[h + 1], 4)
            self.visited[h] = vis
            self.internal[h] = vis & (mn_t != mx_t) & ~equal if h > 0 else np.zeros_like(vis)
            self.zmax[h] = zigzag(mx_t - mx_s)
            self.zmin[h] = zigzag(mn_t - mn_s)
        # positions: Lmax / T index and Lmin index of the first node of each height, and the second bytes before it
        self.offV, self.offI, self.lngV, self.lngM = {}, {}, {}, {}
        v = i = lv = lm = 0
        for h in range(H, -1, -1):
            self.offV[h], self.offI[h], self.lngV[h], self.lngM[h] = v, i, lv, lm
            v += int(self.visited[h].sum())
            i += int(self.internal[h].sum())
            lv += int((self.zmax[h][self.visited[h]] > 0xff).sum())
            lm += int((self.zmin[h][self.internal[h]] > 0xff).sum())
        self.max_code = max(int(self.zmax[h][self.visited[h]].max(initial=0)) for h in self.visited)
        self.max_code = max([self.max_code] + [int(self.zmin[h][self.internal[h]].max(initial=0)) for h in self.internal])

    def lmax_groups(self, h):
        """Per group of four Lmax values at height h: (subset of long children, bit 3 = first; plane-0 position; plane-1
        position of its first second byte)."""
        lng = (self.zmax[h][self.visited[h]] > 0xff).reshape(-1, 4).astype(np.int64)
        subset = lng[:, 0] * 8 + lng[:, 1] * 4 + lng[:, 2] * 2 + lng[:, 3]
        n = lng.sum(1)
        return subset, self.offV[h] + 4 * np.arange(len(n)), self.lngV[h] + np.cumsum(n) - n, lng

    def lmin_groups(self, h):
        """Per internal parent at height h + 1 with at least one internal child: (group length, long values in it, plane-0
        position, plane-1 position, whether its first member is long, whether its last is)."""
        par = self.visited[h].reshape(-1, 4).any(1)
        inter = self.internal[h].reshape(-1, 4)[par]
        lng = (inter & (self.zmin[h] > 0xff).reshape(-1, 4)[par]).astype(np.int64)
        ln, nl = inter.sum(1), lng.sum(1)
        pos = self.offI[h] + np.cumsum(ln) - ln
        lpos = self.lngM[h] + np.cumsum(nl) - nl
        keep = ln > 0
        inter, lng, rows = inter[keep], lng[keep], np.arange(int(keep.sum()))
        first_long = lng[rows, np.argmax(inter, axis=1)]
        last_long = lng[rows, 3 - np.argmax(inter[:, ::-1], axis=1)]
        return ln[keep], nl[keep], pos[keep], lpos[keep], first_long, last_long


class Coverage:
    def __init__(self):
        self.lmax_subsets = {0: set(), 1: set(), 2: set()}
        self.lmin_shapes = {1: set(), 2: set()}       # (length, long values)
        self.lpos_residues = {"lmax": set(), "lmin": set()}
        self.straddle = {"lmax": set(), "lmin": set()}  # plane-0 start mod 32 of groups whose continuation run has a set
                                                        # bit on both sides of a bitmap word boundary
        self.top_long_lmax = 0
        self.top_long_lmin = 0
        self.logs = 0
        self.max_code = 0

    def add(self, L):
        self.logs += 1
        self.max_code = max(self.max_code, L.max_code)
        for h in (0, 1, 2):
            if h + 1 > L.H:
                continue
            subset, pos, lpos, lng = L.lmax_groups(h)
            self.lmax_subsets[h] |= set(subset.tolist())
            self.lpos_residues["lmax"] |= set((lpos[subset != 0] % 4).tolist())
            at29 = (pos % 32 == 29) & (lng[:, :3].sum(1) > 0) & (lng[:, 3] > 0)
            if at29.any():
                self.straddle["lmax"].add(29)
        for h in (1, 2):
            if h + 1 > L.H:
                continue
            ln, nl, pos, lpos, first_long, last_long = L.lmin_groups(h)
            self.lmin_shapes[h] |= set(zip(ln.tolist(), nl.tolist()))
            self.lpos_residues["lmin"] |= set((lpos[nl > 0] % 4).tolist())
            cross = (pos % 32 + ln > 32) & (first_long > 0) & (last_long > 0)
            self.straddle["lmin"] |= set((pos[cross] % 32).tolist())
        for h in range(3, L.H + 1):
            self.top_long_lmax += int((L.zmax[h][L.visited[h]] > 0xff).sum())
            self.top_long_lmin += int((L.zmin[h][L.internal[h]] > 0xff).sum())

    def merge(self, o):
        for h in self.lmax_subsets:
            self.lmax_subsets[h] |= o.lmax_subsets[h]
        for h in self.lmin_shapes:
            self.lmin_shapes[h] |= o.lmin_shapes[h]
        for k in self.lpos_residues:
            self.lpos_residues[k] |= o.lpos_residues[k]
            self.straddle[k] |= o.straddle[k]
        self.top_long_lmax += o.top_long_lmax
        self.top_long_lmin += o.top_long_lmin
        self.logs += o.logs
        self.max_code = max(self.max_code, o.max_code)


def coverage(a):
    """Coverage of the Logs of instants 1.. of `a` against instant 0."""
    cov = Coverage()
    for t in range(1, a.shape[0]):
        cov.add(LogStreams(a[0], a[t]))
    return cov


# ---- the tiles ---------------------------------------------------------------------------------------------------------

SIDES = (16, 64, 128)
INSTANTS = 4
OVERFLOW_SHAPE = (2, 256, 256)


def deltas(S, rng):
    """Per-cell deltas of one instant: 0, +-small (one byte) or +-(129..30000) (two bytes), chosen per cell -- except that
    nodes of every height are, with some probability, given one constant (they are "equal": not internal), so that the
    groups of internal children have every length."""
    kind = rng.random((S, S))
    small = rng.integers(1, 60, size=(S, S)) * rng.choice([-1, 1], size=(S, S))
    big = rng.integers(129, 30001, size=(S, S)) * rng.choice([-1, 1], size=(S, S))
    d = np.where(kind < 0.35, 0, np.where(kind < 0.70, small, big))
    # within a block, the share of two-byte deltas varies from none to nearly all: every subset of a group gets its turn
    dens = rng.choice([0.0, 0.1, 0.5, 0.9], size=(S // 8, S // 8)).repeat(8, 0).repeat(8, 1)
    d = np.where((np.abs(d) > 128) & (rng.random((S, S)) >= dens), small, d)
    for side, prob in ((2, 0.35), (4, 0.30), (8, 0.12), (16, 0.06), (32, 0.04)):
        if side > S // 2:
            break
        n = S // side
        pick = (rng.random((n, n)) < prob).repeat(side, 0).repeat(side, 1)
        const = (rng.integers(-40, 41, size=(n, n)) * (rng.random((n, n)) < 0.5)).repeat(side, 0).repeat(side, 1)
        d = np.where(pick, const, d)
    return d


def block_base(S, rng):
    """Instant 0: non-uniform at every level, and within 1000 inside an 8 x 8 block -- the encoder keeps an instant's Log in
    its stash only while, per block, max_t - min_s and min_t - max_s fit 16 bits, whatever the Log's own values are."""
    return rng.integers(0, 1000, size=(S, S)) + 100 * (np.arange(S)[:, None] // 8 + np.arange(S)[None, :] // 8)


def tile(S, rng):
    base = block_base(S, rng)
    a = np.stack([base] + [base + deltas(S, rng) for _ in range(INSTANTS - 1)])
    return a.astype(np.int32)


def overflow_tile(rng):
    """Every quad of instant 1 internal (no two of its cells share a delta), a quarter of the cells two bytes away: 16384
    internal quads and 4096 internal height-2 nodes, more records than the LDS stash holds."""
    T, S, _ = OVERFLOW_SHAPE
    base = block_base(S, rng)
    q = rng.permuted(np.tile(np.arange(4), (S // 2, S // 2, 1)), axis=2)        # a permutation of 0..3 per quad
    q = q.reshape(S // 2, S // 2, 2, 2).transpose(0, 2, 1, 3).reshape(S, S)
    small = 4 * rng.integers(-10, 11, size=(S, S)) + q                            # distinct within a quad
    big = (4 * rng.integers(40, 7000, size=(S, S)) + q) * rng.choice([-1, 1], size=(S, S))
    d = np.where(rng.random((S, S)) < 0.25, big, small)
    return np.stack([base, base + d]).astype(np.int32)


class Case:
    def __init__(self, name, array):
        self.name, self.array = name, array
        self.logs = array.shape[0] - 1


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [Case("S%d" % S, tile(S, seeded("emit_groups", S))) for S in SIDES]
        _cases.append(Case("overflow256", overflow_tile(seeded("emit_groups", "overflow"))))
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


def check_table():
    total = Coverage()
    for c in cases():
        a = c.array
        assert a.dtype == np.int32 and a.shape[1] == a.shape[2]
        for h in range(1, a.shape[1].bit_length()):
            assert (blocks(a[0], h, np.max) != blocks(a[0], h, np.min)).all(), (c.name, "instant 0 uniform at height", h)
        assert int(a[0].max()) - int(a[0].min()) < 65536, c.name
        cov = coverage(a)
        assert cov.max_code <= 0xffff, (c.name, "a value of a Log needs three bytes")
        if c.name == "overflow256":
            L = LogStreams(a[0], a[1])
            assert L.internal[1].all() and L.visited[0].all(), "overflow case: every quad internal"
            assert len(set(L.lmax_groups(0)[0].tolist())) == 16
        total.merge(cov)
    for h in (0, 1, 2):
        assert total.lmax_subsets[h] == set(range(16)), ("Lmax subsets at height", h, sorted(total.lmax_subsets[h]))
    want = {(n, l) for n in (1, 2, 3, 4) for l in range(n + 1)}
    for h in (1, 2):
        assert total.lmin_shapes[h] >= want, ("Lmin groups at height", h, sorted(want - total.lmin_shapes[h]))
    for k in ("lmax", "lmin"):
        assert total.lpos_residues[k] == {0, 1, 2, 3}, (k, total.lpos_residues[k])
    assert 29 in total.straddle["lmax"], "no Lmax run across a bitmap word boundary"
    assert total.straddle["lmin"] >= {29, 30, 31}, ("Lmin runs across a word boundary", sorted(total.straddle["lmin"]))
    assert total.top_long_lmax > 0 and total.top_long_lmin > 0, "no two-byte value at heights >= 3 (the replay)"
    return total
