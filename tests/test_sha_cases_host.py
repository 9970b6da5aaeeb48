"""The SHA-256 case table (tests/sha_cases.py) delivers the coverage the GPU test relies on -- asserted here, on the CPU, from
the oracle's lengths alone, so that a recipe that stops delivering it fails before anything runs on a card."""
import sha_cases as S


def test_table_covers_every_tail_and_fast_path_count():
    table = S.table()
    by_residue = {}
    for c in table:
        by_residue.setdefault(c.residue, []).append(c)
    print("residues covered: %d of 64; lengths %d .. %d over %d cases" % (len(by_residue), min(c.length for c in table),
                                                                        max(c.length for c in table), len(table)))
    assert sorted(by_residue) == list(range(64)), "len %% 64 not covered: %s" % sorted(set(range(64)) - set(by_residue))
    for r, why in S.CRITICAL.items():
        print("len %% 64 == %d (%s): lengths %s" % (r, why, [c.length for c in by_residue.get(r, [])]))
        assert by_residue.get(r), "no chunk with len %% 64 == %d (%s)" % (r, why)
        assert all((c.length + 8) % 64 == (r + 8) % 64 for c in by_residue[r])
    fast = sorted({S.fast_blocks(c.length) for c in table})
    print("word-wise block counts: %s" % fast)
    assert 0 in fast and 1 in fast and any(f >= 2 for f in fast)
    # the restated count is the kernel's own condition, block by block
    for c in table[:70]:
        total = c.length + 8
        nblk = (total + 1 + 8 + 63) // 64
        assert S.fast_blocks(c.length) == sum(1 for b in range(nblk) if b > 0 and 64 * b + 64 <= total)
    # the named extras are what they are named for
    named = {c.name.split("-")[0]: c for c in table[64:]}
    assert named["uniform"].length == min(c.length for c in table) and named["uniform"].length + 8 < 128
    assert 128 <= named["one"].length + 8 < 192
    assert named["noise"].array.shape == (1, 64, 64) and S.fast_blocks(named["noise"].length) >= 200
    assert named["synth"].array.shape == (2, 256, 256)
    assert {c.array.dtype.name for c in table[64:]} == {"int32", "int64", "float32", "float64"}
    assert all(c.array.dtype.name == "int32" for c in table[:64])
    # what the lockstep test fills its waves with: chunks of 3 to 100 blocks
    assert all(3 <= (c.length + 8 + 9 + 63) // 64 <= 100 for c in table[:64])


def test_table_is_deterministic():
    a, b = S.generate(), S.generate()
    assert [c.key() for c in a] == [c.key() for c in b]
    assert [c.key() for c in a] == [c.key() for c in S.table()]


def test_k3_cases_fall_on_different_residues():
    cs = S.k3_cases()
    assert len(cs) == 3 and len({c.residue for c in cs}) == 3 and all(c.k == 3 for c in cs)
    assert [c.key() for c in cs] == [c.key() for c in S.k3_cases()]
