"""Zonal statistics without a GPU: the entry points are declared and exported and refuse bad arguments, the Python wrappers lay out
labels, offsets and matrices (the library call stubbed), the model is reduce_space per zone, and the K2R_HD arithmetic of
k2r_zonal.h -- limbs, ordered keys, the ranking of a unit's labels -- and plan_zonal run on the CPU: through the pure-host export
and in a stand-alone program (tests/sim/zonal_check.cpp) built with AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import space_model as SM
import zonal_model as ZM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ONE = 1 << 63
ZL = 16  # ZONAL_ZL
I32, I64, F32 = 4, 8, 32
M64 = (1 << 64) - 1


def bits(x):
    return int(np.float64(x).view(np.uint64))


def test_symbols_declared_exported_and_bad_arguments():
    from dcdf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dcdf_k2r.h")).read()
    m = re.search(r"int dcdf_raster_zonal_batch\(([^;]*)\);", hdr)
    assert m, "dcdf_raster_zonal_batch is not declared"
    assert re.sub(r"\s+", " ", m.group(1)) == (
        "const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint16_t* labels, const uint64_t* label_offset, "
        "int label_mem, uint32_t n_zones, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms")
    assert re.search(r"#define DCDF_ZONE_NONE 0xffffu", hdr) and re.search(r"int dcdf_zonal_fold_limbs\(const int64_t limbs\[6\], double\* sum\);", hdr)
    assert "-0.0 is the minimum and +0.0 the maximum" in re.sub(r"\s+\*?\s*", " ", hdr)  # the header states the rule for signed zeros
    assert "dcdf_raster_zonal_batch" in _lib.SYMBOLS and "dcdf_zonal_fold_limbs" in _lib.SYMBOLS and _lib.ZONE_NONE == 0xFFFF
    assert os.path.exists(_lib.LIB_PATH), "library not built"
    lib = C.CDLL(_lib.LIB_PATH)  # (loading needs no GPU)
    assert lib.dcdf_raster_zonal_batch and lib.dcdf_zonal_fold_limbs
    assert lib.dcdf_abi_version() == 3  # added entry points: the ABI version stays
    # what is refused before anything touches a GPU: no raster, and the pure-host function's NULLs
    lib.dcdf_raster_zonal_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    q = np.array([[0, 1, 0, 1, 0, 1]], dtype=np.uint32)
    lab, off, out = np.zeros(1, dtype=np.uint16), np.zeros(1, dtype=np.uint64), np.zeros(8)
    for nq in (0, 1):
        assert lib.dcdf_raster_zonal_batch(None, q.ctypes.data, nq, 1, lab.ctypes.data, off.ctypes.data, 0, 1, out.ctypes.data, 0, off.ctypes.data, None, None) == -1
    lib.dcdf_zonal_fold_limbs.argtypes = [C.c_void_p, C.c_void_p]
    six, d = np.zeros(6, dtype=np.int64), C.c_double()
    assert lib.dcdf_zonal_fold_limbs(None, C.byref(d)) == -1 and lib.dcdf_zonal_fold_limbs(six.ctypes.data, None) == -1
    assert lib.dcdf_zonal_fold_limbs(six.ctypes.data, C.byref(d)) == 0 and bits(d.value) == 0  # +0.0
    six[5] = 1 << 31  # 2^191: one beyond the 192-bit integers
    assert lib.dcdf_zonal_fold_limbs(six.ctypes.data, C.byref(d)) == -1


# ---- the limbs ---------------------------------------------------------------------------------------------------------------
def limb_cases():
    """[six Python ints within int64] whose total sum(l[i] << 32 i) is within 192 signed bits."""
    rng = np.random.default_rng(72)
    cases = [[0] * 6, [1, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, -1], [0, 0, 0, 0, 0, (1 << 31) - 1], [0, 0, 0, 0, 0, -(1 << 31)]]
    for i in range(5):  # a carry across every limb boundary, up and down, and counters far beyond 32 bits
        for v in ((1 << 32) - 1, 1 << 32, (1 << 62) + 12345, -(1 << 32), -(1 << 62) - 1, (1 << 63) - 1, -(1 << 63)):
            c = [0] * 6
            c[i] = v
            c[(i + 1) % 5] += 1
            cases.append(c)
        c = [0] * 6
        c[i], c[i + 1] = -(1 << 32), 1  # cancels to zero across the boundary
        cases.append(c)
    cases.append([(1 << 53) + 1, 0, 0, 0, 0, 0])                  # tie: down to even
    cases.append([(1 << 53) + 3, 0, 0, 0, 0, 0])                  # tie: up to even
    cases.append([-(1 << 53) - 1, 0, 0, 0, 0, 0])                 # negative tie
    cases.append([1, 0, (1 << 21) + 0, 1 << 10, 0, 0])            # the half bit and the sticky bit in other limbs
    cases.append([0, 1 << 31, 0, (1 << 22) | 1, 0, 0])            # a tie at bit 63 under a 54-bit value from bit 96
    cases.append([1, 1 << 31, 0, (1 << 22) | 1, 0, 0])            # just above it
    cases.append([-1, 1 << 31, 0, (1 << 22) | 1, 0, 0])           # just below it
    cases.append([(1 << 54) - 1, 0, 0, 0, 0, 0])                  # rounds up across a power of two
    for _ in range(400):
        c = [int(rng.integers(-(1 << 63), (1 << 63) - 1, endpoint=True)) >> int(rng.integers(0, 64)) for _ in range(5)]
        c.append(int(rng.integers(-(1 << 30), 1 << 30)))
        cases.append(c)
    for _ in range(200):  # near ties: a 54-bit odd integer at some shift, plus or minus one far below
        q = int(rng.integers(1 << 53, 1 << 54)) | 1
        s = int(rng.integers(1, 100))
        v = (q << s) + int(rng.integers(-1, 2))
        v = -v if rng.random() < 0.5 else v
        c = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(5)] + [v >> 160]
        cases.append(c)
    return cases


def total(c):
    return sum(int(v) << (32 * i) for i, v in enumerate(c))


def test_fold_limbs_rounds_once_to_nearest_even():
    from dcdf_amd import _lib
    for c in limb_cases():
        assert -(1 << 191) <= total(c) < (1 << 191)
        got, want = _lib.zonal_fold_limbs(c), float(Fraction(total(c), ONE))  # (Fraction -> float is correctly rounded, ties to even)
        assert bits(got) == bits(want), (c, got, want)
    with pytest.raises(_lib.DcdfError):
        _lib.zonal_fold_limbs([0, 0, 0, 0, 0, 1 << 40])


# ---- the stand-alone program ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("zonal") / "zonal_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-o", path, os.path.join(HERE, "sim", "zonal_check.cpp")])
    return path


def run(exe, tmp_path, lines):
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.split("\n")[:-1]


def test_limbs_in_the_sanitized_program(exe, tmp_path):
    """The same counters through zonal_fold / space_round, and the cut of space_scaled into limbs for every shift and both signs:
    the low five limbs unsigned 32-bit values, the top one signed, their weighted sum the scaled integer."""
    cases = limb_cases()
    lines = ["L " + " ".join(map(str, c)) for c in cases]
    rng = np.random.default_rng(5)
    cuts = []
    for sh in range(64):
        for neg in (0, 256):
            for v in (1, -1, (1 << 42) + 977, -(1 << 42) - 977, (1 << 127) - 1, -(1 << 127), int(rng.integers(-(1 << 62), 1 << 62))):
                cuts.append((v, sh | neg))
    lines += ["S %d %d %d" % ((v >> 64) & M64, v & M64, sc) for v, sc in cuts]
    got = run(exe, tmp_path, lines)
    assert len(got) == len(cases) + len(cuts)
    for c, line in zip(cases, got):
        ok, b = (int(w, 16) for w in line.split())
        assert ok == 1 and b == bits(float(Fraction(total(c), ONE))), (c, line)
    for (v, sc), line in zip(cuts, got[len(cases):]):
        w = [int(x, 16) for x in line.split()]
        limbs = [x - (1 << 64) if x >> 63 else x for x in w[1:]]
        scaled = (-v if sc & 256 else v) << (sc & 255)
        assert w[0] == 1 and all(0 <= x < (1 << 32) for x in limbs[:5]) and -(1 << 31) <= limbs[5] < (1 << 31), (v, sc, line)
        assert total(limbs) == scaled, (v, sc, limbs)
        if abs(v) < (1 << 43) and not (sc & 256) and v > 0:  # a bulk unit's sum: at most three limbs, adjacent
            nz = [i for i, x in enumerate(limbs) if x]
            assert len(nz) <= 3 and nz[-1] - nz[0] <= 2


def test_ordered_keys_are_monotone(exe, tmp_path):
    tiny = np.float64(5e-324)
    vals = [-np.inf, -1.7976931348623157e308, -2.0, np.nextafter(-1.0, -2.0), -1.0, np.nextafter(-1.0, 0.0), -2.2250738585072014e-308,
            -2.225073858507201e-308, -2 * tiny, -tiny, -0.0, 0.0, tiny, 2 * tiny, 2.225073858507201e-308, 2.2250738585072014e-308,
            np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 2.0 ** 63, 1.7976931348623157e308, np.inf]
    assert all(a < b or (a == 0 and b == 0) for a, b in zip(vals, vals[1:]))
    (line,) = run(exe, tmp_path, ["K %d %s" % (len(vals), " ".join("%x" % bits(v) for v in vals))])
    w = [int(x, 16) for x in line.split()]
    keys, back = w[0::2], w[1::2]
    assert all(a < b for a, b in zip(keys, keys[1:]))  # strictly: -0.0 below +0.0
    assert back == [bits(v) for v in vals]
    assert all(0 < k < M64 for k in keys)  # 0 and ~0 are free to say "none"


def test_label_ranking_is_np_unique(exe, tmp_path):
    rng = np.random.default_rng(16)
    sets = {
        "one": np.full(4096, 77),
        "zl": rng.permutation(np.repeat(rng.choice(60000, ZL, replace=False), 256)),
        "zl+1": rng.permutation(np.repeat(rng.choice(60000, ZL + 1, replace=False), 240))[:4096],
        "4096": rng.permutation(rng.choice(65535, 4096, replace=False)),
        "none": np.full(4096, 0xFFFF),
        "edges": np.concatenate([[0, 65534, 31, 32, 63, 64, 0xFFFF], rng.integers(0, 65535, 3000)]),
        "short": rng.integers(100, 140, 37),
    }
    lines, want = [], []
    for name, lab in sets.items():
        named = lab[lab != 0xFFFF]
        uniq = np.unique(named)
        for r0 in sorted({0, ZL, (max(len(uniq), 1) - 1) // ZL * ZL}):
            lines.append("R %d %d %s" % (r0, len(lab), " ".join(map(str, lab.tolist()))))
            rank = np.searchsorted(uniq, lab).astype(np.int64) - r0
            slot = np.where((lab != 0xFFFF) & (rank >= 0) & (rank < ZL), rank, 0xFFFFFFFF)
            want.append((name, r0, len(uniq), slot))
    got = run(exe, tmp_path, lines)
    assert len(got) == len(want)
    for line, (name, r0, n, slot) in zip(got, want):
        w = [int(x, 16) for x in line.split()]
        assert w[0] == n, (name, r0)
        np.testing.assert_array_equal(np.array(w[1:], dtype=np.int64), slot, err_msg="%s round %d" % (name, r0))
    assert want[0][2] == 1 and {n for name, _, n, _ in want if name in ("zl", "zl+1", "4096", "none")} == {ZL, ZL + 1, 4096, 0}


# ---- plan_zonal ----------------------------------------------------------------------------------------------------------------
def plan_case(acc_cap, wanted, n_zones, slab_cap=1 << 22, step=64):
    """T = 20 in segments of 9, 9, 2; tiles of 96 over 100 x 200; per segment and tile a bulk leaf, a walk leaf or an elided one."""
    T, R, Cc, tile, cs = 20, 100, 200, 96, 9
    leaves = []
    for seg in range(3):
        for ti in range(2):
            for tj in range(3):
                kind = (seg + ti + tj) % 3
                leaves.append([0, 0, [I32, I64, F32][kind], [0, 0, 3][kind], int(kind == 2), int(kind == 0)])
    cubes = [[0, T, 0, R, 0, Cc], [T - 2, T - 1, 50, 51, Cc - 1, Cc], [4, 4, 0, R, 0, Cc], [1, 19, 33, 99, 63, 193], [0, T, 7, 7, 1, Cc], [19, 1, 99, 33, 193, 63]]
    c = np.array([[min(a, b), max(a, b), min(d, e), max(d, e), min(f, g), max(f, g)] for a, b, d, e, f, g in cubes], dtype=np.int64)
    nt, plane = c[:, 1] - c[:, 0], (c[:, 3] - c[:, 2]) * (c[:, 5] - c[:, 4])
    base = np.concatenate([[3], 3 + np.cumsum(5 * n_zones * nt + 3)[:-1]])
    moff = np.concatenate([[9], 9 + np.cumsum(np.where(nt > 0, plane, 0) + 9)[:-1]])
    lines = ["P %d %d %d %d %d %d %d %d %d %d" % (T, R, Cc, tile, cs, step, slab_cap, acc_cap, wanted, n_zones), str(len(leaves))]
    lines += [" ".join(map(str, L)) for L in leaves]
    lines.append(str(len(cubes)))
    lines += [" ".join(map(str, list(q) + [int(base[i]), int(moff[i])])) for i, q in enumerate(cubes)]
    return lines, dict(c=c, nt=nt, plane=plane, base=base, moff=moff, n_zones=n_zones, cs=cs, leaves=leaves)


def parse_plan(lines):
    P = {}
    for line in lines:
        w = line.split()
        P.setdefault(w[0], []).append([int(x) for x in w[1:]])
    return P


@pytest.mark.parametrize("acc_cap,wanted", [(128 << 20, 1), (128 << 20, 1000), (72 * 7 * 5, 1), (72 * 7 * 5 + 71, 1000), (72 * 7, 1), (1, 1000), (72 * 7 * 23, 1)])
def test_plan_zonal_batches_cover_every_instant_once(exe, tmp_path, acc_cap, wanted):
    n_zones = 7
    lines, B = plan_case(acc_cap, wanted, n_zones, slab_cap=500)
    P = parse_plan(run(exe, tmp_path, lines))
    assert P["plan"] == [[0]] and P["end"] == [[]]
    room = max(1, acc_cap // (72 * n_zones))  # instants of a batch
    spans, batches = P["span"], P["batch"]
    # the spans cover every (cube, instant) exactly once, in order, and write inside the cube's matrices
    seen = [np.zeros(n, dtype=np.int64) for n in B["nt"]]
    span_q, span_a = [], []
    for acc, nt, o_off, o_zone, o_stat in spans:
        q = int(np.searchsorted(B["base"], o_off, "right")) - 1
        while B["nt"][q] == 0:
            q -= 1
        a = o_off - B["base"][q]
        assert 0 <= a and a + nt <= B["nt"][q] and nt > 0 and o_zone == B["nt"][q] and o_stat == n_zones * B["nt"][q]
        seen[q][a:a + nt] += 1
        span_q.append(q)
        span_a.append(a)
    assert all((s == 1).all() for s in seen)
    # the batches: consecutive ranges of every list; the entries fit the cap (or the batch is one instant); spans lie side by side
    at = [0, 0, 0, 0]
    for unit0, unit1, const0, const1, slab0, slab1, span0, span1, entries in batches:
        assert [unit0, const0, slab0, span0] == at and span1 > span0
        at = [unit1, const1, slab1, span1]
        inst = sum(spans[s][1] for s in range(span0, span1))
        assert entries == inst * n_zones and (inst <= room) and (entries * 72 <= acc_cap or inst == 1)
        used = 0
        for s in range(span0, span1):
            assert spans[s][0] == used * n_zones
            used += spans[s][1]
        # every record of the batch adds to one span's entries, inside its instants, and reads labels inside its cube's plane;
        # per (span, instant) the records' cells are the cube's plane
        cells = {s: np.zeros(spans[s][1], dtype=np.int64) for s in range(span0, span1)}

        def place(acc, a_st, nt, m_off, m_sr, rows, cols):
            s = max(s for s in range(span0, span1) if spans[s][0] <= acc)
            i = acc - spans[s][0]
            q = span_q[s]
            assert a_st == spans[s][1] and 0 <= i and i + nt <= a_st and m_sr == B["c"][q, 5] - B["c"][q, 4]
            p = m_off - B["moff"][q]
            assert 0 <= p and p + (rows - 1) * m_sr + cols <= B["plane"][q]
            cells[s][i:i + nt] += rows * cols
        for u in P.get("unit", [])[unit0:unit1]:
            chunk, t0, t1, rr, rc, top, bottom, left, right, m_sr, a_st, acc, m_off = u
            assert B["leaves"][chunk][5] == 1 and rr % 64 == 0 and rc % 64 == 0 and rr <= top < bottom <= rr + 64 and rc <= left < right <= rc + 64
            assert 0 <= t0 < t1 <= B["cs"]
            place(acc, a_st, t1 - t0, m_off, m_sr, bottom - top, right - left)
        for f in P.get("cfold", [])[const0:const1]:
            nt, rows, cols, m_sr, enc, fbits, elided, a_st, src, acc, m_off = f
            assert elided == 1 and B["leaves"][src // B["cs"]][4] == 1
            place(acc, a_st, nt, m_off, m_sr, rows, cols)
        for s in range(slab0, slab1):
            for f in P["wfold"][P["slab"][s][2]:P["slab"][s][3]]:
                nt, rows, cols, m_sr, enc, fbits, elided, a_st, src, acc, m_off = f
                assert elided == 0
                place(acc, a_st, nt, m_off, m_sr, rows, cols)
        for s, got in cells.items():
            assert (got == B["plane"][span_q[s]]).all(), "a span's instants are not each covered by the cube's cells once"
    assert at == [len(P.get("unit", [])), len(P.get("cfold", [])), len(P.get("slab", [])), len(spans)]
    assert P["max"][0][0] == max(b[8] for b in batches) and P["max"][0][1] == max(s[1] for s in spans)
    assert sum(P["stats"][0]) == int((B["nt"] * B["plane"]).sum()) and all(x > 0 for x in P["stats"][0])
    if acc_cap < 72 * n_zones * 2:  # a cap below one instant's entries (or of exactly one): one-instant batches
        assert len(batches) == int(B["nt"].sum()) and all(b[8] == n_zones for b in batches)
    if acc_cap >= 128 << 20:
        assert len(batches) == 1


def test_plan_zonal_splits_few_units_in_time(exe, tmp_path):
    few = parse_plan(run(exe, tmp_path, plan_case(128 << 20, 1000, 3)[0]))
    many = parse_plan(run(exe, tmp_path, plan_case(128 << 20, 1, 3)[0]))
    assert len(few["unit"]) > len(many["unit"]) and few["stats"] == many["stats"]


# ---- the model and the wrappers ------------------------------------------------------------------------------------------------
def test_model_is_reduce_space_per_zone_with_the_signed_zero_rule():
    from dcdf_amd import _lib
    assert ZM.NONE == _lib.ZONE_NONE  # the model's "no zone" is the library's
    rng = np.random.default_rng(4)
    a = (rng.integers(-40, 40, size=(6, 12, 15)) / 8.0).astype(np.float32)
    a[1, 3, 4] = np.nan
    a[:, 7, 7] = np.nan
    lab = rng.integers(0, 5, size=(12, 15)).astype(np.uint16)
    lab[0, :3] = 0xFFFF
    lab[7, 7] = 5  # a zone of one cell, NaN at every instant
    lab[11, 14] = 6  # a zone of one cell
    w = ZM.zonal(a, lab, 9)  # zones 7 and 8: no cell
    for z in range(9):
        r = SM.reduce_space(a, lab == z)
        for n in SM.NAMES:
            if n in ("min", "max") and (r[n] == 0).any():
                continue  # (fmin / fmax of signed zeros: checked below)
            np.testing.assert_array_equal(w[n][z].view(np.uint64), r[n].view(np.uint64), err_msg="%s of zone %d" % (n, z))
    z = np.zeros((2, 1, 4))
    z[0, 0] = [-0.0, 0.0, 0.0, -0.0]
    z[1, 0] = [0.0, -0.0, 3.0, -0.0]
    w = ZM.zonal(z, np.array([[0, 0, 1, 1]], dtype=np.uint16), 2)
    assert [bits(x) for x in w["min"][0]] == [bits(-0.0)] * 2 and [bits(x) for x in w["max"][0]] == [bits(0.0)] * 2
    assert [bits(x) for x in w["min"][1]] == [bits(-0.0)] * 2 and [bits(x) for x in w["max"][1]] == [bits(0.0), bits(3.0)]
    m = ZM.matrices(np.arange(100, dtype=np.float64), [0, 10], 1, 1 | 16, 3, 4)
    assert list(m) == ["min", "mean"] and m["mean"][2].tolist() == [30, 31, 32, 33]


class _Stub:
    """Stands in for the loaded library: records what the entry point is called with."""

    def __init__(self):
        self.calls = []

    def dcdf_raster_zonal_batch(self, h, cubes, nq, ops, labels, loff, lmem, n_zones, out, mem, off, stats, ms):
        nq = nq.value
        q = np.ctypeslib.as_array(C.cast(cubes, C.POINTER(C.c_uint32)), shape=(max(nq, 1) * 6,))[:nq * 6].reshape(-1, 6).copy()
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        lo = np.ctypeslib.as_array(C.cast(loff, C.POINTER(C.c_uint64)), shape=(max(nq, 1),))[:nq].copy()
        lb = None
        if lmem == 0:
            n = np.abs((q[:, 3].astype(np.int64) - q[:, 2]) * (q[:, 5].astype(np.int64) - q[:, 4]))
            lb = [np.ctypeslib.as_array(C.cast(labels, C.POINTER(C.c_uint16)), shape=(int(lo[i] + n[i]) + 1,))[int(lo[i]):int(lo[i] + n[i])].copy()
                  for i in range(nq)]
        self.calls.append(dict(q=q, off=o, ops=ops.value, mem=mem, out=out.value, labels=labels.value, loff=lo, lmem=lmem, lab=lb, n_zones=n_zones.value))
        np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_uint64)), shape=(3,))[:] = [5, 6, 7]
        return 0


def test_wrappers_lay_out_labels_and_matrices(monkeypatch):
    from dcdf_amd import _lib
    from dcdf_amd.raster import EncodedRaster
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    R = EncodedRaster((10, 50, 60), [None], tile=256, chunk_size=32)
    R._native = C.c_void_p(1)  # (never dereferenced: the library is stubbed)
    try:
        rng = np.random.default_rng(2)
        #        3 instants         reversed: 3         none             1 instant, no rows
        cubes = [[0, 3, 0, 5, 0, 7], [4, 1, 9, 2, 30, 10], [2, 2, 0, 5, 0, 5], [1, 2, 3, 3, 4, 9]]
        labs = [rng.integers(0, 9, size=s).astype(np.uint16) for s in ((5, 7), (7, 20), (5, 5), (0, 5))]
        for ops, bits_ in ((31, 31), (("mean",), 16), (["count", "min"], 9)):
            stub.calls.clear()
            n = bin(bits_).count("1")
            flat, off, ms, stats = R.zonal_flat(cubes, ops, labs, 4)
            c = stub.calls[0]
            assert (c["ops"], c["mem"], c["lmem"], c["n_zones"]) == (bits_, _lib.MEM_HOST, _lib.MEM_HOST, 4)
            np.testing.assert_array_equal(c["q"], cubes)
            np.testing.assert_array_equal(off, [0, 12 * n, 24 * n, 24 * n])
            assert c["loff"].tolist() == [0, 35, 175, 200] and flat.size == 28 * n and stats.tolist() == [5, 6, 7]
            for got, want in zip(c["lab"], labs):
                np.testing.assert_array_equal(got, want.ravel())
        for bad in (labs[:3], [labs[0].T] + labs[1:], [labs[0].astype(np.int32)] + labs[1:]):
            with pytest.raises(ValueError):
                R.zonal_flat(cubes, 16, bad, 4)
        for nz in (0, 65536):
            with pytest.raises(ValueError):
                R.zonal_flat(cubes, 16, labs, nz)
        stub.calls.clear()
        ms, stats = R.zonal_flat(cubes, ("sum", "max"), (8192, [0, 64, 128, 192]), 65535, out_device_ptr=4096, out_offset=[9, 20, 70, 71])
        c = stub.calls[0]
        assert (c["ops"], c["mem"], c["out"], c["labels"], c["lmem"], c["n_zones"]) == (6, _lib.MEM_DEVICE, 4096, 8192, _lib.MEM_DEVICE, 65535)
        assert c["off"].tolist() == [9, 20, 70, 71] and c["loff"].tolist() == [0, 64, 128, 192]
        # zonal(): one cube, a dict of matrices in bit order; n_zones from the labels, NONE apart
        stub.calls.clear()
        lab = rng.integers(0, 12, size=(50, 60)).astype(np.uint16)
        lab[3, 3] = 0xFFFF
        d = R.zonal(("mean", "min"), lab, 2, 7)
        assert list(d) == ["min", "mean"] and all(v.shape == (12, 5) and v.dtype == np.float64 for v in d.values())
        assert stub.calls[0]["q"].tolist() == [[2, 7, 0, 50, 0, 60]] and (stub.calls[0]["ops"], stub.calls[0]["n_zones"]) == (17, 12)
        d = R.zonal(8, lab[3:10, 20:60], window=(3, 10, 20, 60), n_zones=40)
        assert d["count"].shape == (40, 10) and stub.calls[1]["lab"][0].size == 280
        d = R.zonal(31, np.full((50, 60), 0xFFFF, dtype=np.uint16), 3, 3)  # no instants: nothing to read; no zone named: one zone
        assert len(stub.calls) == 2 and list(d) == list(SM.NAMES) and all(v.shape == (1, 0) for v in d.values())
        for bad in (dict(start=5, stop=4), dict(stop=11), dict(window=(0, 51, 0, 60)), dict(window=(0, 5, 0, 5)), dict(n_zones=0)):
            with pytest.raises(ValueError):
                R.zonal("mean", lab, **bad)
        with pytest.raises(ValueError):
            R.zonal("mean", lab.astype(np.int64))
    finally:
        R._native = None
