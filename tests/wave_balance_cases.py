"""Tiles for the thread-to-work mapping of the stash-Log emission (k2r_exec.h: wave_item; k2r_encode.h: bm_share, phase 5a),
and the proof that they reach what a changed mapping can get wrong.  Pure numpy; the host test (simulator against the oracle)
and the GPU test (device views against the oracle) walk the same table.  The model of a Log is the one of
tests/emit_group_cases.py (LogStreams, checked against the oracle there and again in the host test of this table).

What the mapping decides, and so what the table has to vary:

  * the record passes walk the I records (one per internal height-2 node) and the Q records (one per internal quad) in strides of
    the workgroup, starting at a rotated thread index: the NUMBER of records decides which waves get a remainder trip, and
    whether a workgroup has no full wave, one, four or sixteen (S = 16, 64, 128, 256) decides whether the rotation is the identity;
  * phase 1 appends the records in the order its waves get there: WHERE the records come from (one wave's corner of the tile, the
    last wave's, everywhere) decides their order in the stash;
  * the serialized bitmaps are shared out by words: the number of WORDS decides how many each wave and lane takes;
  * the nodes of heights >= 4 have worker threads of their own, whose second bytes are replayed after the bitmaps: a two-byte
    value at the first and the last of them, and at the root, exercises both ends of the worker range.

Every tile but one is int32 [3, S, S]: instant 0 the Snapshot, instants 1 and 2 narrow Logs, so that the second Log's phase 1 follows
the first one's tail phases with no barrier in between.  Instant 1 of a sidelen-256 tile is BUILT to hold exactly the wanted
numbers of internal height-2 nodes and internal quads (check_table asserts them on the model).  The record passes of the emission
draw their items from LDS counters: "tickets128" has four Logs whose counts swing between every node and one (at sidelen 128:
five instants of 256 x 256 would not fit the 768 KB a tile may take), so that a counter left over from the instant before shows.

Bounds the tree itself sets (k = 2, sidelen 256: 4096 height-2 nodes, 16384 quads):
  * an internal quad lies in an internal height-2 node, so Q <= 4 I: Q = 1023 and up need I >= 256;
  * a 64 x 64 corner holds 256 height-2 nodes: the corner placements exist for I <= 256 only, the larger counts are spread;
  * the T bitmap has at most 21845 bits = 683 words; the word counts 1023, 1024, 1025 and "more than 2048" are met by the
    largest bitmap the same code serializes, the continuation bitmap of the Lmax Dac (one bit per visited node)."""
import numpy as np

import emit_group_cases as G

INSTANTS = 3
SIDES = (16, 64, 128, 256)
I_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 4096)
Q_COUNTS = (1, 1023, 1024, 1025, 3073, 16384)
# (I, Q, placement) of instant 1, sidelen 256
SMALL = [(i, 1, p) for i in (1, 63, 64, 65) for p in ("first", "last", "spread")]
LARGE = [(1023, 1025, "spread"), (1024, 1023, "spread"), (1025, 1024, "spread"), (2047, 3073, "spread"), (4096, 16384, "spread")]
# Lmax continuation bitmap of exactly this many words: I = 2047 spread, Q tuned (1 + 4 * internal nodes bits)
V0_WORDS = (1023, 1024, 1025)
# (I, Q, placement) of instants 1..4 of the sidelen-128 tile whose record counts swing (1024 height-2 nodes, 4096 quads)
TICKET_COUNTS = [(1024, 4096, "spread"), (3, 3, "last"), (700, 1500, "spread"), (1, 1, "first")]


def remainder_waves(n):
    """Waves of a 16-wave workgroup that make one trip more than the others over n records."""
    return -(-(n % 1024) // 64)


def node_rc(n, idx):
    """Row / column of the nodes with Morton indices idx in an n x n grid."""
    rc = G.morton_perm(n)[np.asarray(idx, dtype=np.int64)]
    return rc // n, rc % n


def pick(place, total, count):
    """`count` of the Morton indices 0..total-1: the first ones, the last ones, or evenly spread."""
    if place == "first":
        return np.arange(count)
    if place == "last":
        return np.arange(total - count, total)
    return (np.arange(count, dtype=np.int64) * total) // count


def pick_quads(place, nodes, count):
    cand = (4 * np.asarray(nodes, dtype=np.int64)[:, None] + np.arange(4)[None, :]).reshape(-1)
    assert count <= len(cand), "an internal quad needs an internal height-2 node above it"
    if place == "first":
        return cand[:count]
    if place == "last":
        return cand[len(cand) - count:]
    return cand[(np.arange(count, dtype=np.int64) * len(cand)) // count]


def plant(base):
    """Instant 0 with the extremes of the first and the last height-4 node (and so of the root) in their first / last quad."""
    S = base.shape[0]
    base = base.copy()
    base[0, 0], base[0, 1] = 8000, -2000
    if S > 16:
        base[S - 1, S - 1], base[S - 1, S - 2] = 9000, -3000
    return base


def deltas(S, nodes, quads, rng, planted=False):
    """Deltas of one Log with exactly the height-2 nodes `nodes` and the quads `quads` (Morton indices) internal.  Everything else
    keeps the snapshot's value (one constant delta: "equal", not internal, its children not visited).  The quads of an internal
    height-2 node get four different constants (equal quads under a node that is not); an internal quad gets four different cell
    deltas on top.  A share of both is two bytes away, so that second bytes occur at every height."""
    n2, n1 = S // 4, S // 2
    m2 = np.zeros((n2, n2), dtype=bool)
    m2[node_rc(n2, nodes)] = True
    m1 = np.zeros((n1, n1), dtype=bool)
    m1[node_rc(n1, quads)] = True
    assert not (m1 & ~m2.repeat(2, 0).repeat(2, 1)).any()
    k2 = 4 * rng.integers(-20, 21, size=(n2, n2)) + np.where(rng.random((n2, n2)) < 0.2, 1000, 0)
    kq = k2.repeat(2, 0).repeat(2, 1) + np.tile(np.array([[0, 1], [2, 3]]), (n2, n2))
    d = np.where(m2.repeat(2, 0).repeat(2, 1), kq, 0).repeat(2, 0).repeat(2, 1)
    var = np.tile(np.array([[0, 5], [10, 15]]), (n1, n1))
    big = (np.where(rng.random((n1, n1)) < 0.3, 300, 0) * rng.choice([-1, 1], size=(n1, n1))).repeat(2, 0).repeat(2, 1)
    big = big * np.tile(np.array([[1, 0], [0, 0]]), (n1, n1))
    d = d + np.where(m1.repeat(2, 0).repeat(2, 1), var + big, 0)
    if planted:  # the planted extremes move two bytes outwards: two-byte Lmax and Lmin of every node above them
        assert m1[0, 0] and m1[n1 - 1, n1 - 1], "the planted quads have to be internal"
        d[0, 0], d[0, 1] = 200, -200
        if S > 16:
            d[S - 1, S - 1], d[S - 1, S - 2] = 200, -200
    return d


class Case:
    def __init__(self, name, array, want=None, place=None):
        self.name, self.array, self.want, self.place = name, array, want, place
        self.logs = array.shape[0] - 1


def tile256(name, I, Q, place, planted=False):
    rng = G.seeded("wave_balance", name)
    S, n2 = 256, 64 * 64
    base = G.block_base(S, rng)
    if planted:
        base = plant(base)
    out = [base]
    for t in (1, 2):  # instant 2: the mirrored selection with other values
        nodes = pick(place, n2, I)
        quads = pick_quads(place, nodes, Q)
        if t == 2:
            nodes, quads = n2 - 1 - nodes[::-1], 4 * n2 - 1 - quads[::-1]
        if planted:  # (the counts are then no longer exactly I and Q)
            nodes, quads = np.union1d(nodes, [0, n2 - 1]), np.union1d(quads, [0, 4 * n2 - 1])
        out.append(base + deltas(S, nodes, quads, rng, planted))
    return Case(name, np.stack(out).astype(np.int32), None if planted else (I, Q), place)


def small_tile(S):
    """Sidelen 16, 64, 128: no full wave, one wave, four waves.  About half the height-2 nodes internal, the planted corners
    among them."""
    rng = G.seeded("wave_balance", "S", S)
    n2 = (S // 4) ** 2
    base = plant(G.block_base(S, rng))
    out = [base]
    for _ in range(INSTANTS - 1):
        nodes = np.union1d(np.flatnonzero(rng.random(n2) < 0.5), [0, n2 - 1])
        cand = (4 * nodes[:, None] + np.arange(4)[None, :]).reshape(-1)
        quads = np.union1d(cand[rng.random(len(cand)) < 0.6], [0, 4 * n2 - 1])
        out.append(base + deltas(S, nodes, quads, rng, planted=True))
    return Case("S%d" % S, np.stack(out).astype(np.int32))


def ticket_tile():
    """Four Logs at sidelen 128 (four waves), the record counts swinging between all and next to none: a record pass that draws
    its items from a counter finds them only if the counter was cleared since the instant before."""
    S, n2 = 128, 32 * 32
    rng = G.seeded("wave_balance", "tickets")
    base = G.block_base(S, rng)
    out = [base]
    for I, Q, place in TICKET_COUNTS:
        nodes = pick(place, n2, I)
        out.append(base + deltas(S, nodes, pick_quads(place, nodes, Q), rng))
    return Case("tickets128", np.stack(out).astype(np.int32))


def v0_tile(words):
    """A Log with X internal nodes visits 1 + 4 X nodes: I = 2047 spread, their ancestors, and Q tuned to the X wanted."""
    I, n2 = 2047, 64 * 64
    nodes = pick("spread", n2, I)
    above = sum(len(np.unique(nodes >> (2 * (h - 2)))) for h in range(3, 9))
    X = {1023: 8183, 1024: 8191, 1025: 8192}[words]  # 1 + 4 X bits: 32733 (1023 words), 32765 (1024), 32769 (1025)
    return tile256("v0w%d" % words, I, X - I - above, "spread")


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [small_tile(S) for S in SIDES[:3]]
        _cases += [tile256("I%d-Q%d-%s" % (i, q, p), i, q, p) for i, q, p in SMALL + LARGE]
        _cases += [v0_tile(w) for w in V0_WORDS]
        _cases.append(tile256("top256", 65, 130, "spread", planted=True))
        _cases.append(ticket_tile())
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


def words(bits):
    return (bits + 31) // 32


def two_byte_tops(L):
    """(two-byte Lmax, two-byte Lmin) at the first height-4 node, the last one and the root of one Log."""
    out = []
    for h, j in ((4, 0), (4, -1), (L.H, 0)):
        out.append((bool(L.visited[h][j] and L.zmax[h][j] > 0xff), bool(L.internal[h][j] and L.zmin[h][j] > 0xff)))
    return out


def check_table():
    """Raises AssertionError where the table misses a condition (a fault of the table, never a skip)."""
    seen_i, seen_q, t_words, v_words, places = set(), set(), set(), set(), {}
    for c in cases():
        a = c.array
        T, S, _ = a.shape
        assert a.dtype == np.int32 and a.shape[2] == S and a.nbytes <= 768 * 1024, c.name
        assert T == (1 + len(TICKET_COUNTS) if c.name == "tickets128" else INSTANTS), c.name
        for h in range(1, S.bit_length()):
            assert (G.blocks(a[0], h, np.max) != G.blocks(a[0], h, np.min)).all(), (c.name, "instant 0 uniform at height", h)
        for t in range(1, T):
            L = G.LogStreams(a[0], a[t])
            if c.name == "tickets128":
                assert (int(L.internal[2].sum()), int(L.internal[1].sum())) == TICKET_COUNTS[t - 1][:2], (c.name, t)
            assert L.max_code <= 0xffff, (c.name, "a value of a Log needs three bytes")
            # a Log stays in the stash while, per 8 x 8 block, max_t - min_s and min_t - max_s fit 16 bits
            hi = G.blocks(a[t], 3, np.max).astype(np.int64) - G.blocks(a[0], 3, np.min)
            lo = G.blocks(a[t], 3, np.min).astype(np.int64) - G.blocks(a[0], 3, np.max)
            assert hi.max() <= 32767 and lo.min() >= -32768, c.name
            if t == 1:
                lt = sum(int(L.visited[h].sum()) for h in range(1, L.H + 1))
                n0 = lt + int(L.visited[0].sum())
                if S == 256:
                    t_words.add(words(lt))
                    v_words.add(words(n0))
        L = G.LogStreams(a[0], a[1])
        if c.want:
            got = (int(L.internal[2].sum()), int(L.internal[1].sum()))
            assert got == c.want, (c.name, got)
            seen_i.add(got[0])
            seen_q.add(got[1])
            i2, i1 = np.flatnonzero(L.internal[2]), np.flatnonzero(L.internal[1])
            # Morton indices: the first 64 x 64 corner is height-2 nodes 0..255 and quads 0..1023, the last one the last of them
            if c.place == "first":
                assert i2.max() < 256 and i1.max() < 1024, c.name
            if c.place == "last":
                assert i2.min() >= 4096 - 256 and i1.min() >= 16384 - 1024, c.name
            if c.place == "spread" and got[0] >= 16:
                assert len(np.unique(i2 >> 8)) == 16, (c.name, "not every wave's region has a record")
            places.setdefault(c.place, set()).add(got[0])
        if c.name in ("S16", "S64", "S128", "top256"):  # the planted tiles
            want_tops = [(True, True)] * 3
            assert two_byte_tops(L) == want_tops, (c.name, two_byte_tops(L))
    assert seen_i >= set(I_COUNTS), sorted(set(I_COUNTS) - seen_i)
    assert seen_q >= set(Q_COUNTS), sorted(set(Q_COUNTS) - seen_q)
    for p in ("first", "last", "spread"):
        assert places[p] >= {1, 63, 64, 65}, (p, places[p])
    # where the tree allows a choice (Q <= 4 I leaves none below I = 256), the two passes differ in their remainder waves
    for i, q, _ in LARGE[:-1]:
        assert remainder_waves(i) != remainder_waves(q), (i, q)
    assert min(t_words) < 16 and any(16 <= w <= 64 for w in t_words), sorted(t_words)
    assert v_words >= set(V0_WORDS) and max(v_words) > 2048, sorted(v_words)
    ovf = G.LogStreams(case("I4096-Q16384-spread").array[0], case("I4096-Q16384-spread").array[1])
    assert ovf.internal[1].all() and ovf.visited[0].all(), "overflow case: every quad internal"
    return {"I": seen_i, "Q": seen_q, "T words": t_words, "V0 words": v_words}
