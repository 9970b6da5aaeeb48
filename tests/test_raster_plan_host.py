"""The plans of the raster's four region calls without a GPU: tests/sim/plan_check.cpp runs dcdf_amd/csrc/k2r_plan.h in a stand-alone
program built with AddressSanitizer and UBSan and prints every list of every plan; a model that does not restate the planner's loops
checks them by painting.  Every record says where it reads (leaf, instants, a rectangle in chunk coordinates) and where it writes
(offsets and strides); the model paints the raster cell each record reads onto the place it writes and compares with the cubes'
own windows: every cell once, the right one, and for reduce_time in the order of its instants."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
I32, I64, F32, F64 = 4, 8, 32, 64
OK, BOUNDS = 0, -5
SLAB_DEFAULT, REC_DEFAULT = 1 << 22, 6 << 20
EDGES = [-2.0, 0.0, 0.5, 3.0, 100.0]
N_BINS = len(EDGES) - 1


class Raster:
    def __init__(self, T, R, C, tile, cs, leaves):
        self.T, self.R, self.C, self.tile, self.cs = T, R, C, tile, cs
        self.nti, self.ntj, self.nseg = -(-R // tile), -(-C // tile), -(-T // cs)
        self.leaves = np.array(leaves, dtype=np.int64)  # row0 col0 enc fbits elided bulk_ok
        assert len(self.leaves) == self.nseg * self.nti * self.ntj

    def kind(self, leaf):
        return "const" if self.leaves[leaf, 4] else "bulk" if self.leaves[leaf, 5] else "walk"

    def where(self, leaf):
        return leaf // (self.nti * self.ntj), leaf // self.ntj % self.nti, leaf % self.ntj

    def source(self, leaf, t0, t1, top, bottom, left, right):
        """The raster's instants, rows and columns of a rectangle given in the coordinates of the leaf's chunk: inside the leaf."""
        seg, ti, tj = self.where(leaf)
        row0, col0 = self.leaves[leaf, :2]
        ts = np.arange(seg * self.cs + t0, seg * self.cs + t1)
        rs = np.arange(ti * self.tile + top - row0, ti * self.tile + bottom - row0)
        cs = np.arange(tj * self.tile + left - col0, tj * self.tile + right - col0)
        assert len(ts) and len(rs) and len(cs), "an empty record"
        assert seg * self.cs <= ts[0] and ts[-1] < min(self.T, (seg + 1) * self.cs)
        assert ti * self.tile <= rs[0] and rs[-1] < min(self.R, (ti + 1) * self.tile)
        assert tj * self.tile <= cs[0] and cs[-1] < min(self.C, (tj + 1) * self.tile)
        return ts, rs, cs

    def instants(self, leaf, t0, t1):
        seg = self.where(leaf)[0]
        assert t0 < t1 and seg * self.cs + t1 <= min(self.T, (seg + 1) * self.cs)
        return np.arange(seg * self.cs + t0, seg * self.cs + t1)


def plain(table):
    R = Raster(20, 100, 200, 96, 9, [[0, 0, I32, 0, 0, 0]] * 18)
    for leaf in range(18):
        R.leaves[leaf, 5] = {"bulk": 1, "walk": 0, "checker": sum(R.where(leaf)) % 2}[table]
    return R


def tiled():
    """Per segment: a chunk of 40 x 64 over the four leaves of tile columns 0 and 1 (row0 0 / 32, col0 0 / 32), an elided leaf, and a
    chunk leaf the bulk kernel does not take."""
    seg = [[0, 0, I32, 0, 0, 1], [0, 32, I32, 0, 0, 1], [0, 0, F32, 3, 1, 0],
           [32, 0, I32, 0, 0, 1], [32, 32, I32, 0, 0, 1], [0, 0, I64, 0, 0, 0]]
    return Raster(20, 40, 96, 32, 9, seg * 3)


def norm(c):
    return [min(c[0], c[1]), max(c[0], c[1]), min(c[2], c[3]), max(c[2], c[3]), min(c[4], c[5]), max(c[4], c[5])]


class Batch:
    """Cubes and where each call's output, scratch and mask of every cube start: ascending, with gaps between the cubes."""

    def __init__(self, G, cubes):
        self.raw = cubes
        self.cubes = np.array([norm(c) for c in cubes], dtype=np.int64)
        c = self.cubes
        self.nt, self.wr, self.wc = c[:, 1] - c[:, 0], c[:, 3] - c[:, 2], c[:, 5] - c[:, 4]
        self.plane = self.wr * self.wc
        self.cells = self.nt * self.plane
        live, any_t = self.cells > 0, self.nt > 0

        def lay(sizes, gap):
            at = np.concatenate([[0], np.cumsum(sizes + gap)])
            return at[:-1] + gap, int(at[-1]) + 7
        self.b_dec, self.n_dec = lay(self.cells, 3)
        self.b_time, self.n_time = lay(np.where(live, self.plane, 0), 5)
        self.s_time, self.n_scr = lay(np.where(live, self.plane, 0), 2)
        self.b_space, self.n_space = lay(np.where(any_t, self.nt, 0), 4)
        self.b_hist, self.n_hist = lay(np.where(any_t, self.nt * N_BINS, 0), 6)
        self.moff, self.n_mask = lay(np.where(any_t, self.plane, 0), 9)
        self.b_cube, self.n_cube = lay(self.cells, 0)  # (the model's own: every cube's cells, dense)

    def want(self, G, base, size, dims):
        """-1, but on every cube's window the id of the raster cell that belongs there: (t * R + r) * C + c, or r * C + c."""
        w = np.full(size, -1, dtype=np.int64)
        for q, c in enumerate(self.cubes):
            if self.cells[q] == 0:
                continue
            t, r, cc = np.meshgrid(np.arange(c[0], c[1]), np.arange(c[2], c[3]), np.arange(c[4], c[5]), indexing="ij")
            if dims == 3:
                w[base[q]:base[q] + self.cells[q]] = ((t * G.R + r) * G.C + cc).ravel()
            else:
                w[base[q]:base[q] + self.plane[q]] = (r[0] * G.C + cc[0]).ravel()
        return w

    def cube_at(self, base, off, sizes):
        q = int(np.searchsorted(base, off, "right")) - 1
        while q >= 0 and sizes[q] == 0:
            q -= 1
        assert q >= 0 and base[q] <= off < base[q] + sizes[q], "an offset in no cube"
        return q


class Canvas:
    def __init__(self, G, want, dims):
        self.G, self.want, self.dims = G, want, dims
        self.cnt = np.zeros(want.size, dtype=np.int64)
        self.got = np.full(want.size, -1, dtype=np.int64)

    def paint(self, off, st, sr, ts, rs, cs, leaf=None, weight=1):
        """The record writes len(ts) x len(rs) x len(cs) cells at off with instant stride st, row stride sr; it reads instants ts,
        rows rs, columns cs -- an elided record (rs is a count, leaf given) whatever cell of its leaf belongs there."""
        G = self.G
        nt, h, w = len(ts), (rs if leaf is not None else len(rs)), (cs if leaf is not None else len(cs))
        assert h == 1 or sr >= w
        assert nt == 1 or st >= (h - 1) * sr + w
        idx = off + np.arange(nt)[:, None, None] * st + np.arange(h)[None, :, None] * sr + np.arange(w)[None, None, :]
        assert idx.max() < self.cnt.size, "a record beyond the array"
        self.cnt[idx] += weight
        if leaf is not None:
            wid = self.want[idx]
            assert (wid >= 0).all(), "an elided record outside every window"
            r, c = wid // G.C % G.R, wid % G.C
            _, ti, tj = G.where(leaf)
            assert (r // G.tile == ti).all() and (c // G.tile == tj).all(), "an elided record outside its leaf"
        else:
            r, c = rs[None, :, None], cs[None, None, :]
        self.got[idx] = ((ts[:, None, None] * G.R + r) * G.C + c) if self.dims == 3 else (r * G.C + c + 0 * ts[:, None, None])
        return idx

    def check(self, live=None):
        live = (self.want >= 0) if live is None else live
        np.testing.assert_array_equal(self.cnt, live.astype(np.int64), err_msg="cells not written exactly once")
        np.testing.assert_array_equal(self.got[live > 0], self.want[live > 0], err_msg="a cell written from the wrong place")


def unit_ok(G, u):
    chunk, t0, t1, rr, rc, top, bottom, left, right = u[:9]
    assert G.kind(chunk) == "bulk"
    assert rr % 64 == 0 and rc % 64 == 0 and rr <= top < bottom <= rr + 64 and rc <= left < right <= rc + 64
    return G.source(chunk, t0, t1, top, bottom, left, right)


def item_ok(G, it, step):
    chunk, inst, top, bottom, left, right = it[:6]
    assert G.kind(chunk) == "walk" and bottom - top <= step and right - left <= step
    if step == 32:
        assert top // 32 == (bottom - 1) // 32 and left // 32 == (right - 1) // 32
    return G.source(chunk, inst, inst + 1, top, bottom, left, right)


def fold_leaf_ok(G, leaf, kind, enc, fbits, elided):
    assert G.kind(leaf) == kind and (enc, fbits) == tuple(G.leaves[leaf, 2:4]) and elided == (kind == "const")


def walk_sources(G, P, slab_cap, step, key):
    """What every fold of the window walk reads, from the items of its slab: the items fill the fold's dense [nt][rows][cols] block of
    the slab once, with one leaf's consecutive instants of one rectangle.  The blocks of a slab are disjoint and below slab_max, a
    slab holds more than slab_cap cells only when it is one instant of one piece, and no two folds of a slab have the same leaf and
    `id` column: the parts of a piece cut in time are in different slabs."""
    slab_max, fold_nt = P["slab_max"][0]
    folds, items, out = P["wfold"], P["item"], {}
    at_i = at_f = 0
    for item0, item1, fold0, fold1 in P["slab"]:
        assert (item0, fold0) == (at_i, at_f) and item1 > item0 and fold1 > fold0
        at_i, at_f = item1, fold1
        cv = Canvas(G, np.zeros(slab_max, dtype=np.int64), 3)
        leaf_of = np.full(slab_max, -1, dtype=np.int64)
        for it in items[item0:item1]:
            leaf_of[cv.paint(it[7], 0, it[6], *item_ok(G, it, step))] = it[0]
        used, keys = 0, set()
        for i in range(fold0, fold1):
            nt, rows, cols, src = folds[i][0], folds[i][1], folds[i][2], folds[i][key["src"]]
            n = nt * rows * cols
            assert n > 0 and src == used and src + n <= slab_max and nt <= fold_nt
            used += n
            assert (cv.cnt[src:src + n] == 1).all(), "a slab element decoded twice or never"
            leaf = leaf_of[src]
            assert (leaf_of[src:src + n] == leaf).all()
            ids = cv.got[src:src + n].reshape(nt, rows, cols)
            t, r, c = ids // (G.R * G.C), ids // G.C % G.R, ids % G.C
            assert (t == t[0, 0, 0] + np.arange(nt)[:, None, None]).all()
            assert (r == r[0, 0, 0] + np.arange(rows)[None, :, None]).all() and (c == c[0, 0, 0] + np.arange(cols)[None, None, :]).all()
            out[i] = (int(leaf), t[:, 0, 0], r[0, :, 0], c[0, 0, :])
            piece = (int(leaf), int(folds[i][key["id"]]))  # the leaf, and the cube's cells by where they are written or masked
            assert piece not in keys, "two parts of one piece in one slab"
            keys.add(piece)
        assert cv.cnt.sum() == used, "items outside every fold's block"
        assert used <= slab_cap or (fold1 - fold0 == 1 and folds[fold0][0] == 1)
    assert (at_i, at_f) == (len(items), len(folds))
    return out


def stats_ok(P, painted):
    np.testing.assert_array_equal(P["stats"][0], [painted["bulk"], painted["walk"], painted["const"]])


def check_decode(G, B, P, step):
    cv = Canvas(G, B.want(G, B.b_dec, B.n_dec, 3), 3)
    n = dict(bulk=0, walk=0, const=0)
    for u in P["unit"]:
        n["bulk"] += cv.paint(u[11], u[10], u[9], *unit_ok(G, u)).size
    for it in P["item"]:
        n["walk"] += cv.paint(it[7], 0, it[6], *item_ok(G, it, step)).size
    for leaf, ls, le, rows, cols, out_sr, out_off, out_st in P["const"]:
        assert G.kind(leaf) == "const"
        n["const"] += cv.paint(out_off, out_st, out_sr, G.instants(leaf, ls, le), rows, cols, leaf=leaf).size
    cv.check()
    stats_ok(P, n)
    assert sum(n.values()) == B.cells.sum()


def check_time(G, B, P, slab_cap, step):
    walks = walk_sources(G, P, slab_cap, step, dict(src=8, id=9))
    want, want_s = B.want(G, B.b_time, B.n_time, 2), B.want(G, B.s_time, B.n_scr, 2)
    first, last, psz = (np.full(B.n_time, -1, dtype=np.int64) for _ in range(3))
    for q in np.nonzero(B.cells)[0]:
        sl = slice(B.b_time[q], B.b_time[q] + B.plane[q])
        first[sl], last[sl], psz[sl] = B.cubes[q, 0], B.cubes[q, 1], B.plane[q]
    next_t = first.copy()
    n = dict(bulk=0, walk=0, const=0)
    at = [0, 0, 0]
    prev_seg = -1
    for unit0, unit1, const0, const1, slab0, slab1 in P["range"]:
        assert [unit0, const0, slab0] == at and (unit1 > unit0 or const1 > const0 or slab1 > slab0)
        at = [unit1, const1, slab1]
        cv, cs_ = Canvas(G, want, 2), Canvas(G, want_s, 2)
        records = []  # kind, leaf, instants, rows, cols, (sr, init, o_off, s_off, psz)
        for u in P["unit"][unit0:unit1]:
            ts, rs, cs = unit_ok(G, u)
            records.append(("bulk", u[0], ts, rs, cs, u[9:14]))
        for f in P["cfold"][const0:const1]:
            nt, rows, cols, sr, init, enc, fbits, elided, src, o_off, s_off, z = f
            fold_leaf_ok(G, src // G.cs, "const", enc, fbits, elided)
            records.append(("const", src // G.cs, G.instants(src // G.cs, src % G.cs, src % G.cs + nt), rows, cols, (sr, init, o_off, s_off, z)))
        for s in range(slab0, slab1):
            for i in range(P["slab"][s][2], P["slab"][s][3]):
                nt, rows, cols, sr, init, enc, fbits, elided, src, o_off, s_off, z = P["wfold"][i]
                leaf, ts, rs, cs = walks[i]
                fold_leaf_ok(G, leaf, "walk", enc, fbits, elided)
                records.append(("walk", leaf, ts, rs, cs, (sr, init, o_off, s_off, z)))
        segs = set()
        for kind, leaf, ts, rs, cs, (sr, init, o_off, s_off, z) in records:
            segs.add(G.where(leaf)[0])
            one = np.zeros(1, dtype=np.int64)
            idx = cv.paint(o_off, 0, sr, one, rs, cs, leaf=leaf if kind == "const" else None, weight=len(ts))
            cs_.paint(s_off, 0, sr, one, rs, cs, leaf=leaf if kind == "const" else None, weight=len(ts))
            assert (next_t[idx] == ts[0]).all(), "a cell's instants out of order"
            next_t[idx] = ts[-1] + 1
            assert (init == (first[idx] == ts[0])).all() and (psz[idx] == z).all()
            n[kind] += idx.size * len(ts)
        assert len(segs) == 1 and min(segs) > prev_seg, "a range of more than one segment, or out of order"
        prev_seg = min(segs)
        t0, t1 = prev_seg * G.cs, (prev_seg + 1) * G.cs
        # every cell of every cube as often as the cube has instants in this segment (a piece cut in time: once per part's instant)
        cv.check(np.where(first >= 0, np.clip(np.minimum(last, t1) - np.maximum(first, t0), 0, None), 0))
        live_s = np.zeros(B.n_scr, dtype=np.int64)
        for q in np.nonzero(B.cells)[0]:
            live_s[B.s_time[q]:B.s_time[q] + B.plane[q]] = max(0, min(B.cubes[q, 1], t1) - max(B.cubes[q, 0], t0))
        cs_.check(live_s)
    assert at == [len(P["unit"]), len(P["cfold"]), len(P["slab"])]
    np.testing.assert_array_equal(next_t, last, err_msg="instants missing")
    live = np.nonzero(B.cells)[0]
    np.testing.assert_array_equal(P["mean"].reshape(-1, 3), np.stack([B.b_time[live], B.s_time[live], B.plane[live]], axis=1))
    stats_ok(P, n)


def cube_canvas(G, B):
    return Canvas(G, B.want(G, B.b_cube, B.n_cube, 3), 3)


def paint_masked(G, B, cv, q, t_rel, m_off, m_sr, ts, rs, cs, leaf=None):
    """A record of a masked call: its mask bytes are those of cube q's cells, which it reads at the cube's instants t_rel on."""
    p = m_off - B.moff[q]
    assert 0 <= p < B.plane[q] and m_sr == B.wc[q] and B.cubes[q, 0] + t_rel == ts[0] and t_rel + len(ts) <= B.nt[q]
    return cv.paint(B.b_cube[q] + t_rel * B.plane[q] + p, B.plane[q], m_sr, ts, rs, cs, leaf=leaf).size


def check_space(G, B, P, slab_cap, rec_cap, step):
    walks = walk_sources(G, P, slab_cap, step, dict(src=7, id=9))
    cv = cube_canvas(G, B)
    rec_max = P["rec_max"][0][0]
    series = np.zeros(B.n_space, dtype=np.int64)
    n = dict(bulk=0, walk=0, const=0)
    at = [0, 0, 0, 0]
    last_q, last_off = -1, -1
    for unit0, unit1, const0, const1, slab0, slab1, job0, job1, job_nt in P["batch"]:
        assert [unit0, const0, slab0, job0] == at and job1 > job0
        at = [unit1, const1, slab1, job1]
        jobs = P["job"][job0:job1]
        block, wrote = np.zeros(rec_max, dtype=np.int64), np.zeros(rec_max, dtype=np.int64)
        job_q = []
        for rec, n_slots, nt, o_off, o_stride in jobs:
            assert 0 < nt <= job_nt and rec + n_slots * nt <= rec_max
            block[rec:rec + n_slots * nt] += 1
            q = B.cube_at(B.b_space, o_off, B.nt)
            assert o_stride == B.nt[q] and o_off + nt <= B.b_space[q] + B.nt[q]
            assert (q, o_off) > (last_q, last_off), "jobs out of order"
            last_q, last_off = q, o_off
            series[o_off:o_off + nt] += 1
            job_q.append(q)
            if B.plane[q] == 0:
                assert n_slots == 0
        assert block.max(initial=0) <= 1, "two jobs of a batch share records"
        assert max(j[2] for j in jobs) == job_nt
        assert sum(j[1] * j[2] for j in jobs) <= rec_cap or len(jobs) == 1

        def place(rec, nt):  # the job a record's records lie in, and the instant of the cube its first one is of
            j = int(np.searchsorted(jobs[:, 0], rec, "right")) - 1
            while jobs[j][1] == 0:
                j -= 1
            j_rec, n_slots, j_nt, o_off, _ = jobs[j]
            assert j_rec <= rec and rec + nt <= j_rec + n_slots * j_nt and (rec - j_rec) % j_nt + nt <= j_nt
            wrote[rec:rec + nt] += 1
            return job_q[j], o_off - B.b_space[job_q[j]] + (rec - j_rec) % j_nt
        for u in P["unit"][unit0:unit1]:
            q, t_rel = place(u[10], u[2] - u[1])
            n["bulk"] += paint_masked(G, B, cv, q, t_rel, u[11], u[9], *unit_ok(G, u))
        for nt, rows, cols, m_sr, enc, fbits, elided, src, rec, m_off in P["cfold"][const0:const1]:
            fold_leaf_ok(G, src // G.cs, "const", enc, fbits, elided)
            q, t_rel = place(rec, nt)
            n["const"] += paint_masked(G, B, cv, q, t_rel, m_off, m_sr, G.instants(src // G.cs, src % G.cs, src % G.cs + nt), rows, cols, leaf=src // G.cs)
        for s in range(slab0, slab1):
            for i in range(P["slab"][s][2], P["slab"][s][3]):
                nt, rows, cols, m_sr, enc, fbits, elided, src, rec, m_off = P["wfold"][i]
                leaf, ts, rs, cs = walks[i]
                fold_leaf_ok(G, leaf, "walk", enc, fbits, elided)
                q, t_rel = place(rec, nt)
                n["walk"] += paint_masked(G, B, cv, q, t_rel, m_off, m_sr, ts, rs, cs)
        np.testing.assert_array_equal(wrote, block, err_msg="a job's slots are not each written once")
    assert at == [len(P["unit"]), len(P["cfold"]), len(P["slab"]), len(P["job"])]
    live = np.zeros(B.n_space, dtype=np.int64)
    for q in np.nonzero(B.nt)[0]:
        live[B.b_space[q]:B.b_space[q] + B.nt[q]] = 1
    np.testing.assert_array_equal(series, live, err_msg="a cube's instants not once each")
    cv.check()
    stats_ok(P, n)


def check_hist(G, B, P, slab_cap, step):
    walks = walk_sources(G, P, slab_cap, step, dict(src=7, id=9))
    cv = cube_canvas(G, B)
    n = dict(bulk=0, walk=0, const=0)

    def row(o_off):  # the cube, and its instant, whose row of bins starts at o_off
        q = B.cube_at(B.b_hist, o_off, B.nt * N_BINS)
        assert (o_off - B.b_hist[q]) % N_BINS == 0
        return q, (o_off - B.b_hist[q]) // N_BINS
    tab, thr_of = 8, {}  # 2^hist_steps(4)
    for u in P["unit"]:
        m_sr, thr, rev, o_off, m_off = u[9:14]
        enc, fbits = G.leaves[u[0], 2:4]
        assert thr % tab == 0 and thr < P["thr"][0][0] and thr_of.setdefault((enc, fbits), thr) == thr and rev == (enc in (F32, F64) and fbits == 62)
        n["bulk"] += paint_masked(G, B, cv, *row(o_off), m_off, m_sr, *unit_ok(G, u))
    assert P["thr"][0][0] == tab * len(thr_of)
    for nt, rows, cols, m_sr, enc, fbits, elided, src, o_off, m_off in P["cfold"]:
        fold_leaf_ok(G, src // G.cs, "const", enc, fbits, elided)
        n["const"] += paint_masked(G, B, cv, *row(o_off), m_off, m_sr, G.instants(src // G.cs, src % G.cs, src % G.cs + nt), rows, cols, leaf=src // G.cs)
    for i, (nt, rows, cols, m_sr, enc, fbits, elided, src, o_off, m_off) in enumerate(P["wfold"]):
        leaf, ts, rs, cs = walks[i]
        fold_leaf_ok(G, leaf, "walk", enc, fbits, elided)
        n["walk"] += paint_masked(G, B, cv, *row(o_off), m_off, m_sr, ts, rs, cs)
    cv.check()
    stats_ok(P, n)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
WIDTHS = dict(decode=dict(unit=12, item=8, const=8), time=dict(unit=14, cfold=12, wfold=12, item=8, slab=4, range=6, mean=3),
              space=dict(unit=12, cfold=10, wfold=10, item=8, slab=4, job=5, batch=9), hist=dict(unit=14, cfold=10, wfold=10, item=8, slab=4))


def parse(text):
    cases, cur, call = [], None, None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            cur = {}
            cases.append(cur)
        elif w[0] == "bounds":
            cur["bounds"] = int(w[1])
        elif w[0] in WIDTHS:
            call = cur[w[0]] = {"code": int(w[1])}
        elif w[0] != "end":
            call.setdefault(w[0], []).append([int(x) for x in w[1:]])
    for c in cases:
        for name, widths in WIDTHS.items():
            if name in c:
                for k in (set(widths) | set(c[name])) - {"code"}:
                    rows = c[name].get(k, [])
                    c[name][k] = np.array(rows, dtype=np.int64).reshape(-1, widths[k] if k in widths else len(rows[0]))
    return cases


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", path, os.path.join(HERE, "sim", "plan_check.cpp")])
    return path


def run(exe, tmp_path, cases):
    """cases: (raster, batch, step, slab_cap, rec_cap, wanted)"""
    lines = []
    for G, B, step, slab_cap, rec_cap, wanted in cases:
        lines.append("%d %d %d %d %d %d %d %d %d %d %s" % (G.T, G.R, G.C, G.tile, G.cs, step, slab_cap, rec_cap, wanted, N_BINS, " ".join(map(repr, EDGES))))
        lines.append(str(len(G.leaves)))
        lines += [" ".join(map(str, L)) for L in G.leaves.tolist()]
        lines.append(str(len(B.raw)))
        for q, c in enumerate(B.raw):
            lines.append(" ".join(map(str, list(c) + [B.b_dec[q], B.b_time[q], B.s_time[q], B.b_space[q], B.b_hist[q], B.moff[q]])))
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = parse(out.stdout)
    assert len(got) == len(cases)
    return got


def matrix(G, inner):
    """(raster, batch, walk step, slab cap, record cap, wanted units): the whole raster, one cell, a cube inside, the same with every pair
    of bounds reversed, a cube of no instants and one of no rows between them; both steps with both caps small and with none, each
    cap alone, the batch in both orders."""
    s, e, t, b, l, r = inner
    cubes = [[0, G.T, 0, G.R, 0, G.C], [G.T - 2, G.T - 1, G.R // 2, G.R // 2 + 1, G.C - 1, G.C], [4, 4, 0, G.R, 0, G.C], inner,
             [0, G.T, 7, 7, 1, G.C], [e, s, b, t, r, l]]
    A, Z = Batch(G, cubes), Batch(G, cubes[::-1])
    D, E = SLAB_DEFAULT, REC_DEFAULT
    return [(G, A, step, slab, rec, wanted) for step in (64, 32) for slab, rec, wanted in ((100, 50, 1000), (D, E, 1))] + \
           [(G, A, 64, 100, E, 1), (G, A, 64, D, 50, 1), (G, A, 64, D, E, 1000), (G, Z, 32, 100, 50, 1000), (G, Z, 64, D, E, 1)]


def check_all(G, B, got, step, slab_cap, rec_cap):
    assert got["bounds"] == OK and all(got[k]["code"] == OK for k in WIDTHS)
    check_decode(G, B, got["decode"], step)
    check_time(G, B, got["time"], slab_cap, step)
    check_space(G, B, got["space"], slab_cap, rec_cap, step)
    check_hist(G, B, got["hist"], slab_cap, step)


@pytest.mark.parametrize("table", ["bulk", "walk", "checker"])
def test_plain_raster(exe, tmp_path, table):
    """T = 20 in segments of 9, 9, 2; tiles of 96 over 100 x 200: chunk coordinates cross the 64-grid, 9 instants can be split in time
    and 2 cannot."""
    G = plain(table)
    cases = matrix(G, [1, 19, 33, 99, 63, 193])
    got = run(exe, tmp_path, cases)
    for (G, B, step, slab, rec, wanted), g in zip(cases, got):
        check_all(G, B, g, step, slab, rec)
    by = {(c[1] is cases[0][1], c[2], c[3], c[4], c[5]): g for c, g in zip(cases, got)}
    if table != "walk":  # the caps bite: more units after a time split, none in the segment of 2 instants; more batches
        few, many = by[(True, 64, SLAB_DEFAULT, REC_DEFAULT, 1000)], by[(True, 64, SLAB_DEFAULT, REC_DEFAULT, 1)]
        assert len(few["decode"]["unit"]) > len(many["decode"]["unit"]) and len(few["hist"]["unit"]) > len(many["hist"]["unit"])
        assert len(few["space"]["unit"]) > len(many["space"]["unit"])
        short = lambda P: sorted(map(tuple, P["unit"][P["unit"][:, 0] >= 12][:, :9].tolist()))  # noqa: E731
        assert short(few["decode"]) == short(many["decode"]) and len(short(few["decode"])) > 0
    assert len(by[(True, 64, SLAB_DEFAULT, 50, 1)]["space"]["batch"]) > len(by[(True, 64, SLAB_DEFAULT, REC_DEFAULT, 1)]["space"]["batch"]) == 1
    if table != "bulk":  # pieces cut in time: more slabs than segment ranges
        cut, whole = by[(True, 64, 100, REC_DEFAULT, 1)], by[(True, 64, SLAB_DEFAULT, REC_DEFAULT, 1)]
        assert len(cut["time"]["slab"]) > len(whole["time"]["slab"]) == len(whole["time"]["range"])
        assert len(cut["hist"]["slab"]) > len(whole["hist"]["slab"]) == 1


def test_tiled_raster(exe, tmp_path):
    G = tiled()
    cases = matrix(G, [1, 19, 5, 39, 20, 90])
    got = run(exe, tmp_path, cases)
    for (G, B, step, slab, rec, wanted), g in zip(cases, got):
        check_all(G, B, g, step, slab, rec)
        assert all((g[k]["stats"][0] > 0).all() for k in WIDTHS)  # all three kinds of leaf are met


def test_plan_bounds_refuses_a_bad_cube_anywhere_in_the_batch(exe, tmp_path):
    """plan_bounds, the check every region call makes before it plans: BOUNDS for a cube out of range at any place of the batch, an
    empty one included.  (That no plan is made then is the entry points' order of calls, and plan_check's: not what is tested here.)"""
    G = plain("checker")
    good = [[0, 3, 0, 10, 0, 10], [5, 9, 50, 60, 100, 200]]
    bad = [[0, 21, 0, 1, 0, 1], [0, 1, 0, 101, 0, 1], [0, 1, 0, 1, 201, 0], [25, 25, 0, 1, 0, 1]]  # (the last: empty, and still out of bounds)
    cases = [(G, Batch(G, good[:i] + [b] + good[i:]), 64, SLAB_DEFAULT, REC_DEFAULT, 1) for b in bad for i in range(3)]
    cases.append((G, Batch(G, good), 64, SLAB_DEFAULT, REC_DEFAULT, 1))
    got = run(exe, tmp_path, cases)
    for g in got[:-1]:
        assert g["bounds"] == BOUNDS and not any(k in g for k in WIDTHS)
    assert got[-1]["bounds"] == OK and all(k in got[-1] for k in WIDTHS)
