"""Grouped reduce over time without a GPU: the model, the Python wrappers' argument checks, and tests/sim/group_check.cpp -- a
stand-alone program built with AddressSanitizer and UBSan -- for the merge-on-change step, the label gather and the planner.  The plan's records are
painted as tests/test_raster_plan_host.py paints reduce_time's: every record says what it reads (leaf, instants, a rectangle) and
where group 0's cell of it lies in the cube's arrays."""
import os
import subprocess

import numpy as np
import pytest

from dcdf_amd import dataset
from dcdf_amd.raster import EncodedRaster

import group_model as GM
import reduce_model as M
import test_raster_plan_host as PH

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def test_model_against_a_per_cell_loop():
    rng = np.random.default_rng(11)
    a = rng.normal(size=(9, 3, 4)).astype(np.float32)
    a[rng.random(a.shape) < 0.3] = np.nan
    labels = np.array([0, 2, GM.NONE, 0, 7, 2, 2, 0, GM.NONE])
    got = GM.reduce_time_groups(a, labels, 4)  # group 1 has no instant, group 3 neither; label 7 is in no group
    for g in range(4):
        for r in range(3):
            for c in range(4):
                s, n, lo, hi = 0.0, 0, np.nan, np.nan
                for t in range(9):
                    x = float(a[t, r, c])
                    if labels[t] == g and x == x:
                        s, n = s + x, n + 1
                        lo, hi = (x if lo != lo or x < lo else lo), (x if hi != hi or x > hi else hi)
                want = dict(min=lo, max=hi, sum=s, count=float(n), mean=s / n if n else np.nan)
                for name in GM.NAMES:
                    assert np.array([got[name][g, r, c]]).view(np.uint64) == np.array([want[name]]).view(np.uint64), (g, r, c, name)
    assert np.isnan(got["min"][1]).all() and (got["sum"][1] == 0).all() and not np.signbit(got["sum"][1]).any() and (got["count"][3] == 0).all()


def test_one_group_is_reduce_time():
    a = np.random.default_rng(3).integers(-50, 50, size=(6, 2, 5)).astype(np.int32)
    got, want = GM.reduce_time_groups(a, np.zeros(6, dtype=np.uint16), 1), M.reduce_time(a)
    for n in GM.NAMES:
        np.testing.assert_array_equal(got[n][0].view(np.uint64), want[n].view(np.uint64))


# ---- the declarations and the wrappers --------------------------------------------------------------------------------------------
def test_symbol_declared_and_listed():
    from dcdf_amd import _lib
    text = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    assert "int dcdf_raster_reduce_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint16_t* labels," in text
    assert "#define DCDF_GROUP_NONE 0xffffu" in text
    assert "dcdf_raster_reduce_time_groups_batch" in _lib.SYMBOLS and _lib.GROUP_NONE == 0xffff == GM.NONE


class FakeRaster(EncodedRaster):
    """EncodedRaster's wrappers over a _region_call that answers from the model: what they pass down and how they shape the result."""

    def __init__(self, a):
        self.a, self.shape, self.calls, self._native = a, a.shape, [], None

    def _region_call(self, name, q, counts, dtype, args, zeroed=False, stats=True, out_device_ptr=None, out_offset=None):
        import ctypes as C
        own = args(len(q), None, 0, None, None)
        assert name == "reduce_time_groups" and dtype == np.float64 and len(own) == 9
        n, mask, l_ptr, l_off, n_groups = own[0], own[1].value, own[2], own[3], own[4].value
        vol = counts()
        loff = np.ctypeslib.as_array(C.cast(l_off, C.POINTER(C.c_uint64)), (len(q),))
        flat, off = [], np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.uint64)
        for i, c in enumerate(q.astype(int)):
            t0, t1, r0, r1, c0, c1 = PH.norm(c)
            lab = np.ctypeslib.as_array(C.cast(l_ptr.value + 2 * int(loff[i]), C.POINTER(C.c_uint16)), (max(1, t1 - t0),))[:t1 - t0]
            self.calls.append((mask, n_groups, lab.copy()))
            if vol[i]:
                x = GM.reduce_time_groups(self.a[t0:t1, r0:r1, c0:c1], lab, n_groups)
                flat += [x[name_].ravel() for name_ in M.names_of(mask)]
        return np.concatenate(flat + [np.zeros(1)]), off, 0.0, np.zeros(3, dtype=np.uint64)


def test_wrappers_lay_out_groups_and_refuse_bad_labels():
    a = np.random.default_rng(5).integers(-9, 9, size=(7, 4, 5)).astype(np.int32)
    R = FakeRaster(a)
    lab = np.array([1, 0, GM.NONE, 1, 3, 0, 1], dtype=np.uint16)
    got = R.reduce_time_groups(("sum", "min"), lab)
    want = GM.reduce_time_groups(a, lab, 4)  # n_groups: the largest label present, NONE apart, plus 1
    assert list(got) == ["min", "sum"] and got["sum"].shape == (4, 4, 5)
    for n in got:
        np.testing.assert_array_equal(got[n].view(np.uint64), want[n].view(np.uint64))
    got = R.reduce_time_groups("mean", lab[2:6], 2, 6, window=(1, 3, 0, 5), n_groups=2)
    np.testing.assert_array_equal(got["mean"].view(np.uint64), GM.reduce_time_groups(a[2:6, 1:3], lab[2:6], 2)["mean"].view(np.uint64))
    # two cubes, the second with reversed bounds: its labels are those of the normalised cube
    flat, off, _, _ = R.reduce_time_groups_flat([[0, 7, 0, 4, 0, 5], [5, 1, 3, 0, 4, 2]], 31, [lab, lab[1:5]], 3)
    assert off.tolist() == [0, 5 * 3 * 20]
    p = GM.planes(flat, off, 1, 31, 3, 3, 2)
    np.testing.assert_array_equal(p["count"], GM.reduce_time_groups(a[1:5, 0:3, 2:4], lab[1:5], 3)["count"])
    # without instants or cells: the none values, n_groups planes of the window's rows and columns
    none = R.reduce_time_groups(("count", "max"), np.zeros(0, dtype=np.uint16), 3, 3)
    assert none["count"].shape == (1, 4, 5) and (none["count"] == 0).all() and np.isnan(none["max"]).all()
    none = R.reduce_time_groups("sum", lab, window=(2, 2, 0, 5), n_groups=6)
    assert none["sum"].shape == (6, 0, 5)
    assert R.reduce_time_groups("sum", np.full(7, GM.NONE, dtype=np.uint16))["sum"].shape == (1, 4, 5)
    for bad, kw in ((lab.astype(np.int32), {}), (lab[:6], {}), (lab, dict(n_groups=0)), (lab, dict(n_groups=65536)), (lab.reshape(7, 1), {})):
        with pytest.raises(ValueError):
            R.reduce_time_groups("sum", bad, **kw)
    for labels, ng in (([lab.astype(np.int64)], 2), ([lab[:3]], 2), ([lab, lab], 2), ([lab], 0), ([lab], 65536)):
        with pytest.raises(ValueError):
            R.reduce_time_groups_flat([[0, 7, 0, 4, 0, 5]], 1, labels, ng)
    with pytest.raises(ValueError):
        R.reduce_time_groups("median", lab)


def test_variable_maps_ids_and_refuses_too_many():
    class FakeVar(dataset.Variable):
        def __init__(self, a):
            self.a, self.R = a, FakeRaster(a)

        def _region(self, start, stop, top, bottom, left, right):
            T, Rr, Cc = self.a.shape
            return (T if stop is None else stop), (Rr if bottom is None else bottom), (Cc if right is None else right)

        def raster(self):
            return self.R

    a = np.random.default_rng(8).integers(-9, 9, size=(8, 3, 4)).astype(np.int32)
    v = FakeVar(a)
    ids_in = np.array([12, -1, 3, 12, 700000, 3, -5, 12])
    ids, got = v.reduce_time_groups(ids_in, ("sum", "count"))
    assert ids.tolist() == [3, 12, 700000] and got["sum"].shape == (3, 3, 4)
    for i, g in enumerate(ids):
        np.testing.assert_array_equal(got["sum"][i], a[ids_in == g].astype(np.float64).sum(0))
        np.testing.assert_array_equal(got["count"][i], (ids_in == g).sum())
    assert v.R.calls[-1][1] == 3 and v.R.calls[-1][2].tolist() == [1, GM.NONE, 0, 1, 2, 0, GM.NONE, 1]
    assert list(v.reduce_time_groups(ids_in)[1]) == ["mean"]
    ids, got = v.reduce_time_groups(np.full(8, -1), ("min",))
    assert ids.size == 0 and got["min"].shape == (0, 3, 4)
    ids, got = v.reduce_time_groups(np.zeros(0, dtype=np.int64), ("min",), 4, 4)
    assert ids.size == 0 and got["min"].shape == (0, 3, 4)
    with pytest.raises(ValueError):
        v.reduce_time_groups(ids_in.astype(np.float64))
    with pytest.raises(ValueError):
        v.reduce_time_groups(ids_in[:7])
    big = FakeVar(np.zeros((65536, 1, 1), dtype=np.int32))
    with pytest.raises(ValueError, match="65536 distinct"):
        big.reduce_time_groups(np.arange(65536))


# ---- the stand-alone program ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("group") / "group_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", path, os.path.join(HERE, "sim", "group_check.cpp")])
    return path


def test_merge_on_change_equals_the_model_at_every_cut(exe):
    """Every label series up to 8 instants over {0, 1, NONE}, every cut into consecutive parts, stepping part by part through stored
    state: the sum over len of 3^len * 2^(len - 1) cases with all five statistics, a fifth of them with four other sets."""
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    full = 1 + sum(3 ** n * 2 ** (n - 1) for n in range(1, 9))
    assert out.stdout.split()[:2] == ["ok", "cuts"] and int(out.stdout.split()[2]) > full


def test_label_gather_in_the_sanitized_program(exe):
    """gather_time_labels over five cubes -- two of them without cells, their labels outside the array -- and without labels."""
    out = subprocess.run([exe, "--gather"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == ["ok", "gather"], (out.stdout + out.stderr)[-3000:]


WIDTHS = dict(unit=16, cfold=14, wfold=14, item=8, slab=4, range=6, mean=3)


class GroupBatch(PH.Batch):
    """Batch with the arrays of the grouped call: n_groups planes per cube, gaps between the cubes; labels one cube after the other."""

    def __init__(self, G, cubes, n_groups):
        super().__init__(G, cubes)
        self.n_groups = n_groups
        live = self.cells > 0
        size = np.where(live, self.plane * n_groups, 0)
        at = np.concatenate([[0], np.cumsum(size + 5)])
        self.b_grp, self.n_grp = at[:-1] + 5, int(at[-1]) + 7
        at = np.concatenate([[0], np.cumsum(size + 2)])
        self.s_grp, self.n_gscr = at[:-1] + 2, int(at[-1]) + 7
        self.loff = np.concatenate([[0], np.cumsum(np.where(live, self.nt, 0))[:-1]]) + 11


def run(exe, tmp_path, cases):
    lines = []
    for G, B, step, slab_cap in cases:
        lines.append("%d %d %d %d %d %d %d %d" % (G.T, G.R, G.C, G.tile, G.cs, step, slab_cap, B.n_groups))
        lines.append(str(len(G.leaves)))
        lines += [" ".join(map(str, L)) for L in G.leaves.tolist()]
        lines.append(str(len(B.raw)))
        for q, c in enumerate(B.raw):
            lines.append(" ".join(map(str, list(c) + [B.b_grp[q], B.s_grp[q], B.loff[q]])))
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:] + out.stderr[-3000:])
    got, cur = [], None
    for line in out.stdout.split("\n"):
        w = line.split()
        if not w or w[0] == "end":
            continue
        if w[0] == "case":
            cur = {}
            got.append(cur)
        elif w[0] == "groups":
            cur["code"] = int(w[1])
        else:
            cur.setdefault(w[0], []).append([int(x) for x in w[1:]])
    for c in got:
        for k in (set(WIDTHS) | set(c)) - {"code"}:
            rows = c.get(k, [])
            c[k] = np.array(rows, dtype=np.int64).reshape(-1, WIDTHS[k] if k in WIDTHS else len(rows[0]))
    assert len(got) == len(cases)
    return got


def check_groups(G, B, P, slab_cap, step):
    assert P["code"] == PH.OK
    walks = PH.walk_sources(G, P, slab_cap, step, dict(src=8, id=9))
    # group 0's plane of every cube carries the cells' ids; the other groups' planes must never be named by a record
    want, want_s = np.full(B.n_grp, -1, dtype=np.int64), np.full(B.n_gscr, -1, dtype=np.int64)
    first, last, cube_of = (np.full(B.n_grp, -1, dtype=np.int64) for _ in range(3))
    for q in np.nonzero(B.cells)[0]:
        c = B.cubes[q]
        r, cc = np.meshgrid(np.arange(c[2], c[3]), np.arange(c[4], c[5]), indexing="ij")
        ids = (r * G.C + cc).ravel()
        want[B.b_grp[q]:B.b_grp[q] + B.plane[q]] = ids
        want_s[B.s_grp[q]:B.s_grp[q] + B.plane[q]] = ids
        sl = slice(B.b_grp[q], B.b_grp[q] + B.plane[q])
        first[sl], last[sl], cube_of[sl] = c[0], c[1], q
    next_t = first.copy()
    n = dict(bulk=0, walk=0, const=0)
    at, prev_seg = [0, 0, 0], -1
    for unit0, unit1, const0, const1, slab0, slab1 in P["range"]:
        assert [unit0, const0, slab0] == at and (unit1 > unit0 or const1 > const0 or slab1 > slab0)
        at = [unit1, const1, slab1]
        cv, cs_ = PH.Canvas(G, want, 2), PH.Canvas(G, want_s, 2)
        records = []  # kind, leaf, instants, rows, cols, (sr, init, o_off, s_off, psz, lab, gsz)
        for u in P["unit"][unit0:unit1]:
            ts, rs, cs = PH.unit_ok(G, u)
            records.append(("bulk", u[0], ts, rs, cs, u[9:16]))
        for f in P["cfold"][const0:const1]:
            nt, rows, cols, sr, init, enc, fbits, elided, src, o_off, s_off, z, lab, gsz = f
            PH.fold_leaf_ok(G, src // G.cs, "const", enc, fbits, elided)
            records.append(("const", src // G.cs, G.instants(src // G.cs, src % G.cs, src % G.cs + nt), rows, cols, (sr, init, o_off, s_off, z, lab, gsz)))
        for s in range(slab0, slab1):
            for i in range(P["slab"][s][2], P["slab"][s][3]):
                nt, rows, cols, sr, init, enc, fbits, elided, src, o_off, s_off, z, lab, gsz = P["wfold"][i]
                leaf, ts, rs, cs = walks[i]
                PH.fold_leaf_ok(G, leaf, "walk", enc, fbits, elided)
                records.append(("walk", leaf, ts, rs, cs, (sr, init, o_off, s_off, z, lab, gsz)))
        segs = set()
        for kind, leaf, ts, rs, cs, (sr, init, o_off, s_off, z, lab, gsz) in records:
            segs.add(G.where(leaf)[0])
            one = np.zeros(1, dtype=np.int64)
            idx = cv.paint(o_off, 0, sr, one, rs, cs, leaf=leaf if kind == "const" else None, weight=len(ts))
            cs_.paint(s_off, 0, sr, one, rs, cs, leaf=leaf if kind == "const" else None, weight=len(ts))
            assert (next_t[idx] == ts[0]).all(), "a cell's instants out of order"
            next_t[idx] = ts[-1] + 1
            q = int(cube_of[idx.ravel()[0]])
            assert q >= 0 and (cube_of[idx] == q).all()
            assert init == 0 and sr == B.wc[q] and gsz == B.plane[q] and z == B.n_groups * B.plane[q]
            assert lab == B.loff[q] + ts[0] - B.cubes[q, 0], "the label index is not the first instant's offset in its cube"
            assert lab + len(ts) <= B.loff[q] + B.nt[q]
            # every group's copy of the record's cells lies inside the cube's arrays (cv.check: its group 0 cells are in plane 0)
            assert o_off - B.b_grp[q] == s_off - B.s_grp[q] and idx.max() + (B.n_groups - 1) * gsz < B.b_grp[q] + z
            n[kind] += idx.size * len(ts)
        assert len(segs) == 1 and min(segs) > prev_seg, "a range of more than one segment, or out of order"
        prev_seg = min(segs)
        t0, t1 = prev_seg * G.cs, (prev_seg + 1) * G.cs
        cv.check(np.where(first >= 0, np.clip(np.minimum(last, t1) - np.maximum(first, t0), 0, None), 0))
        live_s = np.zeros(B.n_gscr, dtype=np.int64)
        for q in np.nonzero(B.cells)[0]:
            live_s[B.s_grp[q]:B.s_grp[q] + B.plane[q]] = max(0, min(B.cubes[q, 1], t1) - max(B.cubes[q, 0], t0))
        cs_.check(live_s)
    assert at == [len(P["unit"]), len(P["cfold"]), len(P["slab"])]
    np.testing.assert_array_equal(next_t, last, err_msg="instants missing")
    live = np.nonzero(B.cells)[0]
    # what the fill and MEAN run over: every live cube's arrays, all groups
    np.testing.assert_array_equal(P["mean"].reshape(-1, 3), np.stack([B.b_grp[live], B.s_grp[live], B.n_groups * B.plane[live]], axis=1))
    PH.stats_ok(P, n)


def matrix(G, inner, n_groups):
    """The cubes of the plan test's matrix -- the whole raster, one cell, no instants, an unaligned cube inside, no rows, the same
    with every pair of bounds reversed --, both walk steps, the slab small (pieces cut in time) and at its default, both orders."""
    s, e, t, b, l, r = inner
    cubes = [[0, G.T, 0, G.R, 0, G.C], [G.T - 2, G.T - 1, G.R // 2, G.R // 2 + 1, G.C - 1, G.C], [4, 4, 0, G.R, 0, G.C], inner,
             [0, G.T, 7, 7, 1, G.C], [e, s, b, t, r, l]]
    A, Z = GroupBatch(G, cubes, n_groups), GroupBatch(G, cubes[::-1], n_groups)
    return [(G, A, step, slab) for step in (64, 32) for slab in (100, PH.SLAB_DEFAULT)] + [(G, Z, 32, 100), (G, Z, 64, PH.SLAB_DEFAULT)]


@pytest.mark.parametrize("table", ["bulk", "walk", "checker"])
def test_plan_of_a_plain_raster(exe, tmp_path, table):
    G = PH.plain(table)
    cases = matrix(G, [1, 19, 33, 99, 63, 193], 3)
    for (G, B, step, slab), g in zip(cases, run(exe, tmp_path, cases)):
        check_groups(G, B, g, slab, step)
        if table != "bulk" and slab == 100:  # pieces cut in time: more slabs than segment ranges
            assert len(g["slab"]) > len(g["range"])


def test_plan_of_a_tiled_raster(exe, tmp_path):
    G = PH.tiled()
    cases = matrix(G, [1, 19, 5, 39, 20, 90], 7)
    for (G, B, step, slab), g in zip(cases, run(exe, tmp_path, cases)):
        check_groups(G, B, g, slab, step)
        assert (g["stats"][0] > 0).all()  # bulk, walk and elided leaves are all met
