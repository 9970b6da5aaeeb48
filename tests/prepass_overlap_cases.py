"""Tiles for phase 2 of the encoder -- the record pre-pass, the levels of the tree top and the snapshot side of the top, which
is built once per block (k2r_encode.h: s_build) -- and the proof that they reach what a change there can get wrong.  Pure numpy;
the host test (simulator against the oracle) and the GPU test (device views against the oracle) walk the same table.  The model
of a Log is the one of tests/emit_group_cases.py (LogStreams).

The snapshot side.  smin / smax of heights 3..H are written only by the first instant a workgroup compares with a snapshot and
read by the block's other instants.  Every count tile has a second Log on other nodes, which reuses the arrays; "resnap128" has
T = 5 with instant 3 a second Snapshot whose extremes differ from the first one's at every height, so that stale arrays change
Lmax / Lmin of the nodes of heights >= 3 of instant 4; "parts128" (T = 8) goes through the speculative parts, whose continuations
never encoded the snapshot they compare with.  Five instants of 256 x 256 do not fit the 768 KB a tile may take: those two and
the tile whose counts swing have S = 128, and the swing at S = 256 has two Logs.

The pre-pass.  It ORs "this value needs a second byte" flags into its owner's words, so a record it does not visit loses its
second bytes -- IF it has any.  Hence the three variants of the values: "all" (every record of instant 1 has a two-byte value,
every height-2 node of it an internal quad: ANY dropped record changes the bytes, whatever order the records arrived in), "none"
(no value of heights 0 and 1 has: a flag set for nothing shows) and "mix" (a seeded 30 % of the quads).  check_table asserts
these properties on the model.

The record counts of instant 1 are built exactly (STRIDES, boundary_counts): 1; the number of levels of the tree top - 1, that
number and + 1; counts around the 768 (S = 128) and 4608 (S = 256) threads that a sliced pre-pass under the levels of the top would
have as helpers -- that form was built with this table, was bit-exact on it and slower, and the counts are kept as
regression shapes: a few records more or less than whole trips of the strided loops --; every height-2 node and every quad (more
records than the LDS pool holds at S = 256: the pre-pass reads them from global scratch).  S = 256 has 4096 height-2 nodes, so
only its Q records reach the larger counts; at S = 128 both kinds do.  S = 64 (one wave) is the control."""
import numpy as np

import emit_group_cases as G
import wave_balance_cases as W

SIDES = (128, 256)
VARIANTS = ("all", "none", "mix")
SWING = [("all", "all"), (3, 3), (700, 1500), (1, 1)]  # (I, Q) of the Logs of the swinging tile; "all" = every node / quad
MAX_BYTES = 768 * 1024


STRIDES = {128: (764, 768, 772), 256: (4603, 4608, 4612, 4614)}  # Q (and, where the tree has as many nodes, I) of the stride tiles


def levels(S):
    return S.bit_length() - 4  # heights 4..H


def deltas(S, nodes, quads, rng, variant):
    """Deltas of one Log with exactly the height-2 nodes `nodes` and the quads `quads` (Morton indices) internal: everything else
    keeps the snapshot's value ("equal"), the quads of an internal node get four different constants, an internal quad four
    different cell deltas on top.  variant "none": all within -20 .. 38, one byte at heights 0 and 1; "all": "none" with 2000 added
    to the first cell of every internal quad -- that cell's value and the quad's Lmax (the snapshot varies by less than 1000 within
    a quad) take two bytes, so every Q record and every I record above an internal quad carries a flag, and the Log still costs
    less than a Snapshot would; "mix": "none" with 300 added to a seeded 30 % of the quads."""
    n2, n1 = S // 4, S // 2
    m2 = np.zeros((n2, n2), dtype=bool)
    m2[W.node_rc(n2, nodes)] = True
    m1 = np.zeros((n1, n1), dtype=bool)
    m1[W.node_rc(n1, quads)] = True
    assert not (m1 & ~m2.repeat(2, 0).repeat(2, 1)).any()
    k2 = 4 * rng.integers(-5, 6, size=(n2, n2))
    kq = k2.repeat(2, 0).repeat(2, 1) + np.tile(np.array([[0, 1], [2, 3]]), (n2, n2))
    if variant == "mix":
        kq = kq + np.where(rng.random((n1, n1)) < 0.3, 300, 0)
    d = np.where(m2.repeat(2, 0).repeat(2, 1), kq, 0).repeat(2, 0).repeat(2, 1)
    var = np.tile(np.array([[2000 if variant == "all" else 0, 5], [10, 15]]), (n1, n1))
    return d + np.where(m1.repeat(2, 0).repeat(2, 1), var, 0)


class Case:
    def __init__(self, name, array, want=None, variant=None, snapshots=(0,)):
        self.name, self.array, self.want, self.variant, self.snapshots = name, array, want, variant, tuple(snapshots)
        self.logs = array.shape[0] - len(self.snapshots)


def counts_of(S, I, Q):
    n2 = (S // 4) ** 2
    return (n2 if I == "all" else I), (4 * n2 if Q == "all" else Q)


def select(S, I, Q, mirror=False):
    n2 = (S // 4) ** 2
    nodes = W.pick("spread", n2, I)
    quads = W.pick_quads("spread", nodes, Q)
    if mirror:
        nodes, quads = n2 - 1 - nodes[::-1], 4 * n2 - 1 - quads[::-1]
    return nodes, quads


def count_tile(S, I, Q, variant):
    """[3, S, S]: instant 1 with exactly I internal height-2 nodes and Q internal quads, instant 2 the mirrored selection."""
    I, Q = counts_of(S, I, Q)
    name = "S%d-I%d-Q%d-%s" % (S, I, Q, variant)
    rng = G.seeded("prepass_overlap", name)
    base = G.block_base(S, rng)
    out = [base]
    for t in (1, 2):
        nodes, quads = select(S, I, Q, mirror=t == 2)
        out.append(base + deltas(S, nodes, quads, rng, variant))
    return Case(name, np.stack(out).astype(np.int32), (I, Q), variant)


def swing_tile(S, counts):
    rng = G.seeded("prepass_overlap", "swing", S)
    base = G.block_base(S, rng)
    out = [base]
    for I, Q in counts:
        out.append(base + deltas(S, *select(S, *counts_of(S, I, Q)), rng, "all"))
    return Case("swing%d" % S, np.stack(out).astype(np.int32), variant="all")


def quiet_base(S, rng):
    """A second snapshot: noise of 0 .. 99 on its own ramp, 5000 above the first one's values -- cheap to store as a Snapshot (one
    byte per value below the top), dear as a Log against block_base (differences of up to 1000 everywhere)."""
    return 5000 + rng.integers(0, 100, size=(S, S)) + 37 * (np.arange(S)[:, None] // 8) + 53 * (np.arange(S)[None, :] // 8)


def resnap_tile():
    """T = 5 at S = 128: Snapshot, two Logs, a second Snapshot (instant 3), one Log against it."""
    S = 128
    rng = G.seeded("prepass_overlap", "resnap")
    base = G.block_base(S, rng)
    out = [base]
    for I, Q, mirror in ((300, 700, False), (500, 900, True)):
        out.append(base + deltas(S, *select(S, I, Q, mirror), rng, "mix"))
    base2 = quiet_base(S, rng)
    out.append(base2)
    out.append(base2 + deltas(S, *select(S, 400, 800), rng, "mix"))
    return Case("resnap128", np.stack(out).astype(np.int32), variant="mix", snapshots=(0, 3))


def parts_tile():
    """T = 8 at S = 128 for the speculative parts: [0, 4) [4, 8) with two parts, [0, 4) [4, 6) [6, 8) with four."""
    S = 128
    rng = G.seeded("prepass_overlap", "parts")
    base = G.block_base(S, rng)
    out = [base]
    for t in range(1, 8):
        out.append(base + deltas(S, *select(S, 100 * t + 7, 250 * t + 3, mirror=t % 2 == 0), rng, "mix"))
    return Case("parts128", np.stack(out).astype(np.int32), variant="mix")


def boundary_counts(S):
    """(I, Q) of instant 1 of the "all" tiles of sidelen S."""
    n2, L = (S // 4) ** 2, levels(S)
    out = [(c, c) for c in (1, L - 1, L, L + 1)]
    out += [(min(c, n2), c) for c in STRIDES[S]]
    out.append(("all", "all"))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = []
        for S in SIDES:
            _cases += [count_tile(S, i, q, "all") for i, q in boundary_counts(S)]
            Wt = STRIDES[S][1]
            for v in ("none", "mix"):
                _cases += [count_tile(S, min(Wt, (S // 4) ** 2), Wt, v), count_tile(S, "all", "all", v)]
        _cases.append(swing_tile(128, SWING))
        _cases.append(swing_tile(256, SWING[:2]))
        _cases.append(resnap_tile())
        _cases.append(parts_tile())
        _cases.append(count_tile(64, "all", 700, "mix"))  # the control: one wave, the old order
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


def loader_case():
    """The tile whose float32 and int64 views run the other loaders' kernels (S = 128)."""
    Wt = STRIDES[128][1]
    return case("S128-I%d-Q%d-all" % (Wt, Wt))


def record_flags(L):
    """Per internal quad and per internal height-2 node of one Log: does its stash record carry a second-byte flag?  Q record:
    one of its four cell values is long; I record: the Lmax of one of its four quads is, or the Lmin of an internal one."""
    long0 = (L.zmax[0] > 0xff).reshape(-1, 4).any(1)
    q = long0[L.internal[1]]
    long1 = ((L.zmax[1] > 0xff) | (L.internal[1] & (L.zmin[1] > 0xff))).reshape(-1, 4).any(1)
    return q, long1[L.internal[2]]


def check_table():
    """Raises AssertionError where the table misses a condition (a fault of the table, never a skip)."""
    seen = {}
    for c in cases():
        a = c.array
        T, S, _ = a.shape
        assert a.dtype == np.int32 and a.shape[2] == S and a.nbytes <= MAX_BYTES, c.name
        for s in c.snapshots:
            for h in range(1, S.bit_length()):
                assert (G.blocks(a[s], h, np.max) != G.blocks(a[s], h, np.min)).all(), (c.name, "snapshot uniform at height", h)
            assert int(a[s].max()) - int(a[s].min()) < 65536, c.name
        snap = 0
        for t in range(1, T):
            if t in c.snapshots:
                snap = t
                continue
            Lg = G.LogStreams(a[snap], a[t])
            assert Lg.max_code <= 0xffff, (c.name, "a value of a Log needs three bytes")
            hi = G.blocks(a[t], 3, np.max).astype(np.int64) - G.blocks(a[snap], 3, np.min)
            lo = G.blocks(a[t], 3, np.min).astype(np.int64) - G.blocks(a[snap], 3, np.max)
            assert hi.max() <= 32767 and lo.min() >= -32768, c.name
            got = (int(Lg.internal[2].sum()), int(Lg.internal[1].sum()))
            if c.name.startswith("swing"):
                assert got == counts_of(S, *SWING[t - 1]), (c.name, t, got)
            if t == 1 and c.want:
                assert got == c.want, (c.name, got)
                seen.setdefault(S, {}).setdefault(c.variant, set()).add(got)
            if t == 1 and c.want or c.name.startswith("swing"):
                fq, fi = record_flags(Lg)
                if c.variant == "all":  # a record the pre-pass does not visit changes the bytes: every record carries a flag
                    assert fq.all() and fi.all(), (c.name, t)
                elif c.variant == "none":
                    assert not fq.any() and not fi.any(), (c.name, t)
                elif min(got) >= 100:
                    assert 0.1 < fq.mean() < 0.5 and fi.any() and not fi.all(), (c.name, float(fq.mean()), float(fi.mean()))
    for S in SIDES:
        n2 = (S // 4) ** 2
        assert seen[S]["all"] >= {counts_of(S, i, q) for i, q in boundary_counts(S)}, (S, sorted(seen[S]["all"]))
        for v in ("none", "mix"):
            assert (n2, 4 * n2) in seen[S][v] and len(seen[S][v]) == 2, (S, v)
    # the second snapshot's extremes differ from the first one's at every node of heights >= 3, and instant 4 visits such nodes at
    # every height: Lmax = max_t - max_s and Lmin = min_t - min_s taken against the first snapshot's would be other values
    r = case("resnap128").array
    Lg = G.LogStreams(r[3], r[4])
    for h in range(3, Lg.H + 1):
        assert (G.blocks(r[3], h, np.max) != G.blocks(r[0], h, np.max)).all(), h
        assert (G.blocks(r[3], h, np.min) != G.blocks(r[0], h, np.min)).all(), h
        assert Lg.visited[h].any() and Lg.internal[h].any(), h
    p = case("parts128").array
    assert p.shape[0] == 8 and len({int(G.LogStreams(p[0], p[t]).internal[2].sum()) for t in range(1, 8)}) == 7
    return seen
