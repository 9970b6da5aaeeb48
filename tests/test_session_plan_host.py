"""The plan of an encode session without a GPU: tests/sim/session_check.cpp runs dcdf_amd/csrc/k2r_session_plan.h in a stand-alone
program built with AddressSanitizer and UBSan and prints every list of the plan and what the post-run functions decide; a model
that does not restate the planner's loops checks them.  check() holds EVERY plan printed in this file to the invariants a GPU run
would otherwise have to trip over: every valid tile in one class or one universal group, queues that are permutations in
non-increasing cost with every continuation behind the part it waits for (the deadlock argument of DESIGN.md 3e), parts that tile
[0, T), slots that are aligned, inside their slab and disjoint.  The tests add the expected values: statuses, loaders, which tiles
are split, where parts are cut, which tiles run again."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
I32, I64, F32, F64 = 4, 8, 32, 64
ESZ = {I32: 4, F32: 4, I64: 8, F64: 8}
OK, BAD_ARG, UNSUPPORTED = 0, -1, -8
ST_OK, ST_UNSUPPORTED, ST_OUT_CAPACITY, ST_RESPLIT = 0, -8, -100, -102
DEFAULT, OFF, ALL, TAIL = 0, 1, 2, 3
PER_CU = {4: 4, 5: 2, 6: 1, 7: 1, 8: 1}             # stand-ins for encode_blocks_per_cu / encode_list_words, by log2 sidelen
LIST_WORDS = {4: 11, 5: 23, 6: 31, 7: 41, 8: 53}
COUNTED = {"classes", "class_tiles", "generic_tiles", "class_items", "split", "items", "again", "declined_tiles"}


def r256(x):
    return (x + 255) // 256 * 256


class Tile:
    def __init__(self, T, R, C, dtype=I32, strides=None, base=4096, fbits=0):
        self.T, self.R, self.C, self.dtype, self.base, self.fbits = T, R, C, dtype, base, fbits
        self.strides = strides or (R * C, C, 1)

    def line(self):
        return "%d %d %d %d %d %d %d %d %d" % ((self.T, self.R, self.C, self.dtype) + tuple(self.strides) + (self.base, self.fbits))


class Session:
    def __init__(self, tiles, k=2, cap=0, cus=4, split=DEFAULT, parts=8, max_wgs=0, passes=()):
        self.tiles, self.k, self.cap, self.cus, self.split, self.parts, self.max_wgs = list(tiles), k, cap, cus, split, parts, max_wgs
        self.passes = [list(p) for p in passes]

    def text(self):
        lines = ["%d %d %d %d %d %d 0" % (self.k, self.cap, self.cus, self.split, self.parts, self.max_wgs),
                 " ".join(str(PER_CU[g]) for g in range(4, 9)), " ".join(str(LIST_WORDS[g]) for g in range(4, 9)), str(len(self.tiles))]
        lines += [t.line() for t in self.tiles]
        lines.append(str(len(self.passes)))
        lines += [" ".join(map(str, p)) for p in self.passes]
        return "\n".join(lines) + "\n"

    def wgs(self, lg):
        w = self.cus * PER_CU[lg]
        return min(w, self.max_wgs) if self.max_wgs else w


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("session") / "session_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", path, os.path.join(HERE, "sim", "session_check.cpp")])
    return path


def parse(text):
    """[plan]: name -> list of ints, or list of rows for the counted lists; plan["passes"] = the same per pass."""
    plans, cur, rows = [], None, None
    for ln in text.splitlines():
        tok = ln.split()
        if ln.startswith(" "):
            rows.append([int(x) for x in tok])
            continue
        name, vals = tok[0], [int(x) for x in tok[1:]]
        if name == "session":
            cur = {"passes": []}
            plans.append(cur)
        elif name == "pass":
            cur = {}
            plans[-1]["passes"].append(cur)
        elif name in COUNTED:
            rows = cur[name] = []
        else:
            cur[name] = vals
    return plans


def run(exe, tmp_path, sessions):
    src = tmp_path / "sessions.txt"
    src.write_text("".join(s.text() for s in sessions))
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-3000:]
    plans = parse(out.stdout)
    assert len(plans) == len(sessions)
    for s, p in zip(sessions, plans):
        assert len(p["passes"]) == len(s.passes)
        check(s, p, p)
        for q in p["passes"]:
            check(s, p, q)
    return plans


def disjoint(spans, total, what):
    """[(offset, bytes)]: 256-aligned, inside [0, total), no two overlapping."""
    end = 0
    for off, size in sorted(spans):
        assert off % 256 == 0 and off >= end and size > 0, (what, off, size, end)
        end = off + size
    assert end <= total, (what, end, total)


def check(S, P, Q):
    """P: the plan as created; Q: P itself, or the queues, parts and items after a pass."""
    n = len(S.tiles)
    items, split, queues = Q["items"], Q["split"], Q["class_items"]
    classes = P["classes"]
    # every valid tile in exactly one class or universal group, an invalid one in none; the per-tile tables agree with the groups
    seen = [0] * n
    for ci, tiles in enumerate(P["class_tiles"]):
        for t in tiles:
            seen[t] += 1
            assert P["tile_class"][t] == ci and P["tile_gkey"][t] == 0
        assert [S.tiles[t].T for t in tiles] == sorted((S.tiles[t].T for t in tiles), reverse=True)   # longest first
    for key, tiles in zip(P["generic_keys"], P["generic_tiles"]):
        for t in tiles:
            seen[t] += 1
            assert P["tile_class"][t] == -1 and P["tile_gkey"][t] == key != 0
    assert seen == [int(st == OK) for st in P["pre_status"]]
    assert len(set(map(tuple, classes))) == len(classes) and len(set(P["generic_keys"])) == len(P["generic_keys"])
    # parts: the tile's own item first, then continuations that tile [0, T) in order; 2 .. min(8, K2R_PARTS) of them
    part_of, first_of = {}, {}
    for parts in split:
        t, T = parts[0], S.tiles[parts[0]].T
        assert t < n and all(p >= n for p in parts[1:]) and 2 <= len(parts) <= min(8, S.parts)
        at = 0
        for j, p in enumerate(parts):
            tile, b, e = items[p][:3]
            assert tile == t and b == at and e > b, (parts, p)
            at = e
            part_of[p] = (t, j)
        assert at == T
        first_of[t] = parts
    assert Q["part_items"] == [p for parts in split for p in parts]
    assert Q["part_first"] == list(np.cumsum([0] + [len(parts) for parts in split]))
    whole = [i for i in range(n) if i not in first_of]
    assert all(items[i][1:3] == [0, 0] and items[i][6] == -1 for i in whole)                         # inst_begin, inst_end, flag
    # queues: a permutation of the class's items, cost non-increasing, a continuation behind its first part and the part before
    # it, no first part shorter than one of its continuations
    length = lambda p: items[p][2] - items[p][1] if p in part_of else S.tiles[p].T

    def cost(p):  # a continuation never counts for more than the parts it follows
        if p not in part_of or part_of[p][1] == 0:
            return length(p)
        t, j = part_of[p]
        return min(length(q) for q in first_of[t][:j + 1])
    for ci, queue in enumerate(queues):
        lg = classes[ci][0]
        want = [p for t in P["class_tiles"][ci] for p in first_of.get(t, [t])]
        assert sorted(queue) == sorted(want) and len(set(queue)) == len(queue)
        costs = [cost(p) for p in queue]
        # (after a pass the queues are pruned, not sorted again -- today's behaviour: a tile that has become whole keeps the place
        # of its first part, in front of longer items.  What the deadlock argument needs, the order of a tile's parts, still holds.)
        assert Q is not P or costs == sorted(costs, reverse=True), (ci, costs)
        pos = {p: i for i, p in enumerate(queue)}
        for t in P["class_tiles"][ci]:
            parts = first_of.get(t, [t])
            assert all(pos[a] < pos[b] for a, b in zip(parts, parts[1:])) and all(pos[parts[0]] < pos[p] for p in parts[1:])
            assert all(length(parts[0]) >= length(p) for p in parts[1:])
        assert 1 <= P["grid"][ci] <= max(1, S.wgs(lg))
    # slots: aligned, inside their slab, disjoint; flags and shared copies the same; capacities by the two formulas
    out_total, parts_total, shared_total, minmax_total, flags, order_total, lists_total = P["totals"]
    valid = [i for i in range(n) if P["pre_status"][i] == OK]
    live = valid + [p for p in part_of if p >= n]
    disjoint([(items[i][4], items[i][5]) for i in live if not items[i][3]], out_total, "main slab")
    disjoint([(items[i][4], items[i][5]) for i in live if items[i][3]], parts_total, "parts' slab")
    assert all(items[i][3] == int(i >= n) for i in live)
    for i in valid:
        t = S.tiles[i]
        assert items[i][5] == r256(S.cap if S.cap else 4 * t.T * t.R * t.C + 4096)
    shared = {}
    for parts in split:
        t = S.tiles[parts[0]]
        lg = classes[P["tile_class"][parts[0]]][0]
        for p in parts[1:]:
            b, e = items[p][1:3]
            assert items[p][5] == r256(-(-items[parts[0]][5] * (e - b) // t.T) + 4096)
        assert len({(items[p][6], items[p][7]) for p in parts}) == 1 and 0 <= items[parts[0]][6] < flags
        shared[items[parts[0]][6]] = (items[parts[0]][7], r256(2 << (2 * lg)))
    assert len(shared) == len(split)
    disjoint(shared.values(), shared_total, "shared copies")
    if Q is P:
        assert flags == len(split)
        assert P["order_off"] == list(np.cumsum([0] + [len(q) for q in queues]))[:-1] and order_total == sum(len(q) for q in queues)
        words = [P["grid"][ci] * LIST_WORDS[classes[ci][0]] for ci in range(len(classes))]
        assert P["lists_off"] == list(np.cumsum([0] + words))[:-1] and lists_total == sum(words)
        assert all(P["grid"][ci] == max(1, min(len(queues[ci]), S.wgs(classes[ci][0]))) for ci in range(len(classes)))
        mm = np.cumsum([0] + [2 * S.tiles[i].T for i in valid])
        assert [P["minmax_off"][i] for i in valid] == list(mm[:-1]) and minmax_total == mm[-1]


def split_tiles(P):
    return sorted(parts[0] for parts in P["split"])


# ---- classification ----------------------------------------------------------------------------------------------------------

def test_statuses_and_the_universal_kernels_keys(exe, tmp_path):
    """validate_tile: what is refused and with which code, and the universal kernel's key k << 8 | levels with the reference's f64
    depth: k = 5, m = 125 has 4 levels (sidelen 625); k = 6, m = 216 too, and its sidelen 1296 is beyond the kernel's 1024."""
    good = Tile(3, 16, 16)
    bad = [Tile(3, 16, 16, base=0), Tile(0, 16, 16), Tile(3, 0, 16), Tile(3, 16, 0), Tile(3, 16, 16, dtype=7), Tile(3, 16, 16, dtype=F32, fbits=63),
           Tile(3, 16, 16, dtype=F64, fbits=63)]
    fine = [Tile(3, 16, 16, dtype=F32, fbits=62), Tile(3, 16, 16, dtype=I32, fbits=63), Tile(3, 16, 16, dtype=I64, fbits=99)]
    P = run(exe, tmp_path, [Session([good] + bad + fine)] + [Session([good], k=k) for k in (-1, 0, 1, 17)] +
            [Session([Tile(1, 1024, 3), Tile(1, 1025, 3), Tile(2, 8, 8), Tile(2, 9, 8), Tile(2, 300, 257), Tile(1, 1, 1)]),
             Session([Tile(2, 125, 100), Tile(2, 124, 125), Tile(2, 126, 3), Tile(1, 625, 1), Tile(1, 626, 1)], k=5),
             Session([Tile(2, 216, 216), Tile(2, 215, 215), Tile(2, 36, 36)], k=6),
             Session([Tile(2, 16, 16), Tile(2, 256, 256), Tile(2, 257, 1)], k=16), Session([Tile(2, 16, 16), Tile(2, 64, 64)], k=3)])
    assert P[0]["pre_status"] == [OK] + [BAD_ARG] * 7 + [OK] * 3
    assert all(p["pre_status"] == [BAD_ARG] and not p["classes"] and not p["generic_keys"] for p in P[1:5])
    assert P[5]["pre_status"] == [OK, UNSUPPORTED, OK, OK, OK, OK]
    assert P[5]["tile_gkey"] == [(2 << 8) | 10, 0, (2 << 8) | 3, 0, (2 << 8) | 9, 2 << 8] and P[5]["tile_class"] == [-1, -1, -1, 0, -1, -1]
    assert P[6]["pre_status"] == [OK, OK, OK, OK, UNSUPPORTED] and P[6]["tile_gkey"] == [(5 << 8) | 4, (5 << 8) | 4, (5 << 8) | 4, (5 << 8) | 4, 0]
    assert P[7]["pre_status"] == [UNSUPPORTED, OK, OK] and P[7]["tile_gkey"] == [0, (6 << 8) | 3, (6 << 8) | 2]
    assert P[8]["pre_status"] == [OK, OK, UNSUPPORTED] and P[8]["tile_gkey"] == [(16 << 8) | 1, (16 << 8) | 2, 0]
    assert P[9]["tile_gkey"] == [(3 << 8) | 3, (3 << 8) | 4] and not P[9]["classes"]           # k != 2: never a fused kernel
    assert P[6]["generic_keys"] == [(5 << 8) | 4] and P[6]["generic_tiles"] == [[0, 1, 2, 3]]


def test_loader_choice_at_the_boundaries(exe, tmp_path):
    """The row loader (1 int32, 2 float32, 3 int64, 4 float64) needs: no padding, unit column stride, a positive row stride and an
    instant stride that are multiples of 16 bytes, a 16-byte aligned base, row offsets below 2^31 bytes.  One step to either side
    of each condition; classes in order of first occurrence."""
    big4, big8 = (1 << 29) - 64, (1 << 28) - 32   # (rows - 1) * stride_r + cols: one element below 2^31 bytes at 64 rows of 64
    cases = [(Tile(2, 64, 64), (6, 0, 1)), (Tile(2, 64, 64, dtype=F32), (6, 0, 2)), (Tile(2, 64, 64, dtype=I64), (6, 0, 3)),
             (Tile(2, 64, 64, dtype=F64), (6, 0, 4)),
             (Tile(2, 64, 63), (6, 1, 0)), (Tile(2, 63, 64), (6, 1, 0)), (Tile(2, 33, 33), (6, 1, 0)), (Tile(2, 32, 32), (5, 0, 1)),
             (Tile(2, 64, 64, strides=(8192, 64, 2)), (6, 0, 0)), (Tile(2, 64, 64, strides=(8192, 1, 64)), (6, 0, 0)),
             (Tile(2, 64, 64, strides=(4096, 68, 1)), (6, 0, 1)), (Tile(2, 64, 64, strides=(4096, 66, 1)), (6, 0, 0)),
             (Tile(2, 64, 64, dtype=I64, strides=(4096, 66, 1)), (6, 0, 3)), (Tile(2, 64, 64, dtype=I64, strides=(4096, 65, 1)), (6, 0, 0)),
             (Tile(2, 64, 64, strides=(4098, 64, 1)), (6, 0, 0)), (Tile(2, 64, 64, strides=(-4096, 64, 1)), (6, 0, 1)),
             (Tile(2, 64, 64, strides=(4096, -64, 1)), (6, 0, 0)), (Tile(2, 64, 64, strides=(4096, 0, 1)), (6, 0, 0)),
             (Tile(2, 64, 64, base=4096 + 16), (6, 0, 1)), (Tile(2, 64, 64, base=4096 + 8), (6, 0, 0)), (Tile(2, 64, 64, base=4096 + 4), (6, 0, 0)),
             (Tile(2, 64, 64, dtype=F64, base=4096 + 8), (6, 0, 0)),
             (Tile(2, 64, 64, strides=(4096, (big4 - 64) // 63 // 4 * 4, 1)), (6, 0, 1)),
             (Tile(2, 64, 64, strides=(4096, -(-(big4) // 63) // 4 * 4 + 4, 1)), (6, 0, 0)),
             (Tile(2, 64, 64, dtype=F64, strides=(4096, (big8 - 64) // 63 // 2 * 2, 1)), (6, 0, 4)),
             (Tile(2, 64, 64, dtype=F64, strides=(4096, -(-(big8) // 63) // 2 * 2 + 2, 1)), (6, 0, 0))]
    for t, (lg, padded, vec) in cases:   # (the table's own arithmetic: which side of 2^31 bytes the two big strides are on)
        reach = ((t.R - 1) * t.strides[1] + t.C) * ESZ[t.dtype]
        if abs(t.strides[1]) > 1 << 20:
            assert (reach < 1 << 31) == (vec != 0), (t.strides, reach)
    P = run(exe, tmp_path, [Session([t for t, _ in cases])])[0]
    assert P["pre_status"] == [OK] * len(cases)
    assert [tuple(P["classes"][c]) for c in P["tile_class"]] == [want for _, want in cases]
    first = []
    for _, want in cases:
        if want not in first:
            first.append(want)
    assert [tuple(c) for c in P["classes"]] == first


# ---- which tiles are split, and where ----------------------------------------------------------------------------------------

def test_plan_split_as_a_table(exe, tmp_path):
    """plan_split over one class of n side-64 tiles, wgs = cus * 1 workgroups.  Default: nothing when n > 4 wgs, else the last
    min(n, 2 wgs) tiles of the longest-first order.  K2R_SPLIT=0: nothing; all: every tile; tail: the last min(n, 2 wgs) whatever n.

    TODAY'S RULE, not intent: a single tile of fewer than 4 instants anywhere among the candidates turns the split off for the
    whole class (sorted longest first, it sits at the candidates' end, where the shrinking loop of plan_split does not look).  Under
    `all` every tile is a candidate, so one 3-instant tile keeps a class whole; under the default and `tail` it does so when it is
    among the last min(n, 2 wgs).  A class of short tiles only is not split either."""
    def cls(instants):
        return [Tile(T, 64, 64) for T in instants]
    rng = np.random.default_rng(3)
    mixed = [int(x) for x in rng.integers(4, 40, size=9)]
    order = sorted(range(9), key=lambda i: -mixed[i])            # (stable: ties in order of occurrence)
    S = [Session(cls(mixed), cus=2),                             # 0: n = 9 > 4 * 2: nothing
         Session(cls(mixed[:8]), cus=2),                         # 1: n = 8 = 4 wgs: the last 4
         Session(cls(mixed), cus=3),                             # 2: the last 6
         Session(cls(mixed[:3]), cus=2),                         # 3: n < 2 wgs: all 3
         Session(cls(mixed), cus=2, split=OFF), Session(cls(mixed), cus=2, split=ALL), Session(cls(mixed), cus=2, split=TAIL),   # 4 5 6
         Session(cls(mixed), cus=8, max_wgs=2),                  # 7: K2R_MAX_WGS caps wgs: as 0
         Session(cls(mixed), cus=8, max_wgs=3),                  # 8: as 2
         Session(cls(mixed + [3]), cus=2, split=ALL),            # 9: one short tile: nothing
         Session(cls(mixed + [3]), cus=3),                       # 10: it is among the last 6: nothing
         Session(cls([3, 2, 1] + mixed[:5]), cus=1, split=TAIL),  # 11: the last 2 are short: nothing
         Session(cls([3] + mixed[:5] + [50, 60]), cus=1, split=TAIL),  # 12: the short tile is last: nothing
         Session(cls([3, 3, 2, 1]), cus=4, split=ALL),           # 13: short tiles only
         Session(cls(mixed[:4]) + [Tile(3, 32, 32)], cus=4, split=ALL)]  # 14: the short tile is of ANOTHER class: the first is split
    P = run(exe, tmp_path, S)
    last = lambda idx, m: sorted(idx[len(idx) - m:])
    assert split_tiles(P[0]) == [] and split_tiles(P[1]) == last(sorted(range(8), key=lambda i: -mixed[i]), 4)
    assert split_tiles(P[2]) == last(order, 6) and split_tiles(P[3]) == [0, 1, 2]
    assert split_tiles(P[4]) == [] and split_tiles(P[5]) == list(range(9)) and split_tiles(P[6]) == last(order, 4)
    assert split_tiles(P[7]) == [] and split_tiles(P[8]) == last(order, 6)
    assert [split_tiles(p) for p in P[9:14]] == [[]] * 5
    assert split_tiles(P[14]) == [0, 1, 2, 3] and len(P[14]["classes"]) == 2
    assert P[7]["grid"] == [2] and P[8]["grid"] == [3] and P[3]["grid"] == [2] and P[13]["grid"] == [4]


@pytest.mark.parametrize("parts", [2, 3, 4, 8])
def test_part_bounds(exe, tmp_path, parts):
    """Where a T-instant tile is cut, T = 4 .. 40: at half (rounded up), then at half of the rest, and so on while at least 4 instants
    are left and K2R_PARTS (clamped to 2 .. 8 where the environment is read) allows another part."""
    maxp = parts
    Ts = list(range(4, 41))
    P = run(exe, tmp_path, [Session([Tile(T, 16, 16) for T in Ts], split=ALL, parts=maxp)])[0]
    assert split_tiles(P) == list(range(len(Ts)))
    by_tile = {p[0]: p for p in P["split"]}
    for i, T in enumerate(Ts):
        begins = [P["items"][p][1] for p in by_tile[i]]
        want, left = [0], T
        while left >= 4 and len(want) < maxp:
            want.append(want[-1] + (left + 1) // 2)
            left = T - want[-1]
        assert begins == want, (T, begins)
    assert {len(p) for p in P["split"]} == set(range(2, min(maxp, 5) + 1))     # (40 instants: 20, 10, 5, 3, 2 -- five parts at the most)


def test_the_speculative_parts_gpu_session_is_split(exe, tmp_path):
    """The shapes of tests/test_gpu_encode.py::test_speculative_parts_splice's main session under K2R_SPLIT=all: every tile of its
    three classes is split, for each K2R_PARTS it runs with.  With the 3-instant tile it used to carry, the int32 class is not."""
    main = [Tile(32, 256, 256)] * 3 + [Tile(13, 256, 256), Tile(9, 200, 256), Tile(8, 128, 128, dtype=I64)] + [Tile(32, 256, 256)] * 27
    S = [Session(main, cus=256, split=ALL, parts=p) for p in (2, 4, 8)] + [Session(main + [Tile(3, 256, 256)], cus=256, split=ALL)]
    P = run(exe, tmp_path, S)
    for p in P[:3]:
        assert split_tiles(p) == list(range(len(main))) and [tuple(c) for c in p["classes"]] == [(8, 0, 1), (8, 1, 0), (7, 0, 3)]
    assert split_tiles(P[3]) == [4, 5]


def test_many_tiles_and_classes(exe, tmp_path):
    """A seeded mix of shapes, types, lengths and invalid tiles under every split mode: check() on each."""
    rng = np.random.default_rng(11)
    tiles = []
    for _ in range(300):
        side = int(rng.choice([8, 16, 16, 32, 64, 100, 128, 256, 2000]))
        tiles.append(Tile(int(rng.integers(1, 30)), side, side if rng.random() < 0.8 else side - 1, dtype=int(rng.choice([I32, I64, F32, F64])),
                          base=int(rng.choice([0, 4096, 4100, 8192]))))
    run(exe, tmp_path, [Session(tiles, cus=cus, split=mode, parts=parts, cap=cap, max_wgs=mw)
                        for cus, mode, parts, cap, mw in [(4, DEFAULT, 8, 0, 0), (4, ALL, 8, 0, 0), (64, TAIL, 3, 1000, 0), (256, DEFAULT, 8, 0, 5),
                                                          (1, ALL, 2, 256, 1), (2, OFF, 8, 0, 0)]])


# ---- after a run -------------------------------------------------------------------------------------------------------------

def worst_caps(exe):
    out = subprocess.run([exe, "worst"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr
    return dict(zip(range(4, 9), map(int, out.stdout.split())))


def test_retries_and_drop_parts(exe, tmp_path):
    """Statuses as a run leaves them, on split and unsplit tiles of two classes (tiles 0 .. 5 side 16, 6 .. 8 side 32; K2R_SPLIT=tail with
    wgs = 1 splits the last two of each): who runs again, who gets a worst-case slot and of what size, who is whole afterwards,
    and the plan without the dropped parts (check() again).  Second pass: a tile that was ST_RESPLIT and is ST_OUT_CAPACITY once
    whole; nothing else runs then."""
    tiles = [Tile(T, 16, 16) for T in (9, 30, 20, 12, 8, 25)] + [Tile(T, 32, 32) for T in (10, 16, 5)] + [Tile(4, 8, 8)]
    st1 = [ST_OUT_CAPACITY, ST_OK, ST_OK, ST_RESPLIT, ST_OUT_CAPACITY, ST_UNSUPPORTED, ST_RESPLIT, ST_UNSUPPORTED, ST_OK, ST_OK]
    st2 = [ST_OK, ST_OK, ST_OK, ST_OUT_CAPACITY, ST_OK, ST_UNSUPPORTED, ST_OK, ST_UNSUPPORTED, ST_OK, ST_OK]
    S = Session(tiles, cus=1, split=TAIL, max_wgs=1, passes=[st1, st2])
    P = run(exe, tmp_path, [S])[0]
    worst = worst_caps(exe)
    assert P["class_tiles"] == [[1, 5, 2, 3, 0, 4], [7, 6, 8]] and split_tiles(P) == [0, 4, 6, 8]
    a, b = P["passes"]
    # the splice lists: the split tiles whose status is ST_OK after the run -- tile 8 alone
    assert a["splice_first"] == [0, len(P["split"][3])] and a["splice_items"] == P["split"][3] and P["split"][3][0] == 8
    assert a["again"] == [[3, 0, 4], [6]] and a["retry_tiles"] == [3, 0, 4, 6] and a["unsplit"] == [1]
    assert a["retry_own_cap"] == [0, 6 + 9 * (1 + worst[4]), 6 + 8 * (1 + worst[4]), 0]
    assert split_tiles(a) == [8] and all(a["items"][t][1:3] == [0, 0] and a["items"][t][6] == -1 for t in (0, 3, 4, 6))
    gone = {p for parts in P["split"][:3] for p in parts[1:]}
    assert all(not gone & set(q) for q in a["class_items"]) and [len(q) for q in a["class_items"]] == [6, 2 + len(P["split"][3])]
    assert a["declined_keys"] == [(2 << 8) | 4, (2 << 8) | 5] and a["declined_tiles"] == [[5], [7]]
    # second pass: tile 3, whole already: nothing to drop
    assert b["again"] == [[3], []] and b["retry_tiles"] == [3] and b["retry_own_cap"] == [6 + 12 * (1 + worst[4])] and b["unsplit"] == [0]
    assert split_tiles(b) == [8] and b["class_items"] == a["class_items"] and b["declined_tiles"] == [[5], [7]]


def test_the_retry_gpu_session(exe, tmp_path):
    """tests/test_gpu_object_sha256.py::test_split_session_retries_and_runs_twice on the CPU: its five side-16 tiles are split in
    three parts each, and with the statuses its docstring derives for out_cap_per_tile = 1024 only `smooth` is still split after
    the first run and in the second."""
    tiles = [Tile(8, 16, 16)] * 5 + [Tile(5, 8, 8)]
    st1 = [ST_OK, ST_RESPLIT, ST_RESPLIT, ST_RESPLIT, ST_OUT_CAPACITY, ST_OK]
    st2 = [ST_OK, ST_OK, ST_OK, ST_OUT_CAPACITY, ST_OK, ST_OK]
    P = run(exe, tmp_path, [Session(tiles, cus=256, split=ALL, parts=4, cap=1024, passes=[st1, st2]),
                            Session(tiles, cus=256, split=ALL, parts=4, cap=256, passes=[[ST_OUT_CAPACITY] * 5 + [ST_OK]])])
    assert split_tiles(P[0]) == [0, 1, 2, 3, 4] and [[P[0]["items"][p][1:3] for p in parts] for parts in P[0]["split"]] == [[[0, 4], [4, 6], [6, 8]]] * 5
    a, b = P[0]["passes"]
    assert a["splice_items"] == P[0]["split"][0] and a["again"] == [[1, 2, 3, 4]] and a["unsplit"] == [1] and split_tiles(a) == [0]
    assert [c > 0 for c in a["retry_own_cap"]] == [False, False, False, True]
    assert b["again"] == [[3]] and b["unsplit"] == [0] and split_tiles(b) == [0] and b["retry_own_cap"][0] > 0
    assert split_tiles(P[1]["passes"][0]) == [] and P[1]["passes"][0]["class_items"] == [[0, 1, 2, 3, 4]]


def test_worst_instant_bytes_covers_noise(exe):
    """worst_instant_bytes(lg), the size of the slot a tile gets after ST_OUT_CAPACITY (6 + T (1 + worst)), against the oracle: one
    instant of iid noise over the fused kernel's whole value range, as a Snapshot and as a Log against a Snapshot of other noise --
    the two candidates an instant is chosen from."""
    worst = worst_caps(exe)
    rng = np.random.default_rng(0xB16)
    for lg in range(4, 9):
        s, t = rng.integers(-(1 << 30) + 1, 1 << 30, size=(2, 1 << lg, 1 << lg))
        snap, log = O.snapshot_dump(t)["serialized_len"], O.log_dump(s, t)["serialized_len"]
        print("lg %d: worst_instant_bytes %d, oracle snapshot %d, log %d" % (lg, worst[lg], snap, log))
        assert worst[lg] >= snap and worst[lg] >= log, (lg, worst[lg], snap, log)
