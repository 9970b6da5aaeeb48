"""Content addressing on the device: k_object_sha256 (k2r_cid.hip, one lane per chunk) against hashlib at every tail and in every
state a session can be in.  Run on a real MI355X: pytest -m gpu.

A stored object is named by CIDv1(codec 0x12, sha2-256(8-byte header + Chunk::write_to bytes)); a wrong digest is silent -- the
bytes still equal the oracle's and every query still answers.  Every expected digest here is hashlib.sha256(header + ORACLE bytes);
the digest of header + enc.fetch(i) must agree with it, and object_cids() must be 01 12 12 20 || digest.  The tiles come from
tests/sha_cases.py, whose coverage (every len % 64, the five critical ones, 0 / 1 / many word-wise blocks) is asserted on the CPU by
tests/test_sha_cases_host.py; sessions run in-process on memory from DeviceBuffer (test_object_sha256_on_device of
test_gpu_encode.py stays the check on memory torch allocated).

Deliberately NOT tested:
  * the high word of the bit count (w[14]): it is zero below a chunk of 512 MB;
  * the `aligned == false` branch of the kernel: no session path reaches it.  Every `out` the kernel sees is a tile's own slot --
    d_out + slot_off[i] with every slot_off a sum of capacities rounded up to 256 (dcdf_encoder_create); a spliced tile's bytes are
    gathered by k_stitch into that same first slot (the parts' own slots in d_out_b, also at multiples of 256, are never hashed:
    the kernel reads args[0 .. n) only); a retried tile gets an allocation of its own (run_generic, dcdf_encoder_run) -- and
    d_out, d_out_b and the retry slots each start a hipMalloc block (DevBuf::alloc, pooled blocks are handed out whole), which is
    at least 256-byte aligned.  Hence (uintptr_t)out % 8 == 0 always, and the byte-wise fallback for unaligned data stays
    unvisited."""
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import sha_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


class Tile:
    """A tile the session must refuse: no bytes, digest 32 zero bytes, CID None."""

    def __init__(self, name, array, bits=0):
        self.name, self.array, self.bits, self.round, self.ref = name, np.ascontiguousarray(array), bits, False, None


class Session:
    """The tiles' arrays in ONE device allocation (256-byte aligned starts), an Encoder over them."""

    def __init__(self, tiles, k=2, out_cap_per_tile=0):
        from dcdf_amd.encoder import DeviceBuffer, Encoder
        self.tiles = list(tiles)
        offs, total = [], 0
        for c in self.tiles:
            offs.append(total)
            total += (c.array.nbytes + 255) & ~255
        self.buf = DeviceBuffer(total)
        descs = []
        for c, o in zip(self.tiles, offs):
            a = c.array
            self.buf.write(o, a)
            descs.append((self.buf.ptr + o, O.ENC[a.dtype], tuple(s // a.itemsize for s in a.strides), a.shape, c.bits, c.round))
        self.enc = Encoder(descs, k=k, out_cap_per_tile=out_cap_per_tile)

    def close(self):
        self.enc.close()
        self.buf.free()

    def wrong_digests(self, dig):
        """[(index, tile)] whose device digest is not hashlib's over header + oracle bytes (32 zero bytes for a refused tile)."""
        assert dig.shape == (len(self.tiles), 32) and dig.dtype == np.uint8
        return [(i, c) for i, c in enumerate(self.tiles) if dig[i].tobytes() != (bytes(32) if c.ref is None else c.digest)]

    def check_digests(self, dig, what=""):
        bad = self.wrong_digests(dig)
        if bad:
            by = {}
            for i, c in bad:
                by.setdefault(c.length % 64, []).append("%d:%s(len %d)" % (i, c.name, c.length))
            raise AssertionError("%s%d of %d digests wrong, at len %% 64 = %s: %s" % (what, len(bad), len(self.tiles), sorted(by),
                                                                                  "; ".join("%d -> %s" % (r, ", ".join(v[:4])) for r, v in sorted(by.items()))))

    def check_bytes_and_cids(self):
        """enc.fetch(i) is the oracle's bytes (so its digest is the expected one too) and the CIDs frame the digests."""
        cids = self.enc.object_cids()
        for i, c in enumerate(self.tiles):
            if c.ref is None:
                assert self.enc.result(i)[0] != 0 and cids[i] is None, (i, c.name)
                continue
            data = self.enc.fetch(i)
            assert data == c.ref, (i, c.name)
            assert hashlib.sha256(S.HEADER + data).digest() == c.digest
            assert cids[i] == S.CID_PREFIX + c.digest, (i, c.name)


def test_every_tail(dc):
    """Every case of the table in one session of 150 tiles: three workgroups, the last wave partly empty (the t >= n lanes)."""
    table = S.table()
    tiles = (table * 3)[:150]
    assert len(tiles) >= 130 and len(tiles) % 64 != 0 and len(tiles) > 128 and set(map(id, table)) <= set(map(id, tiles))
    assert {c.residue for c in tiles} == set(range(64))
    s = Session(tiles)
    s.enc.run()
    dig, _ = s.enc.object_sha256()
    s.check_digests(dig)
    s.check_bytes_and_cids()
    s.close()


def lockstep_orders():
    """The tile set of the lockstep test in two orders: indices into one list of 128 tiles (two full waves)."""
    table = S.table()
    fill = table[:64]                                      # 3 to 100 blocks each (asserted by the host test)
    noise = next(c for c in table if c.name == "noise-1x64x64")      # ~400 blocks
    big = next(c for c in table if c.name == "synth-2x256x256")      # ~2600 blocks
    tiles = [fill[i % 64] for i in range(128)]
    for at, c in ((0, noise), (31, big), (63, noise), (64, big), (100, noise), (127, big)):  # lane 0, the middle, lane 63
        tiles[at] = c
    first = list(range(128))
    second = [int(i) for i in np.random.default_rng(63).permutation(128)]
    # in the second order the long chunks sit in other lanes, and the two waves hold other sets
    assert [second.index(i) % 64 for i in (0, 31, 63, 64, 100, 127)] != [0, 31, 63, 0, 36, 63]
    return tiles, first, second


def test_lockstep_lanes(dc):
    """Lanes with very different block counts in one wave: the long chunks at lane 0, lane 63 and in the middle of waves otherwise
    full of short ones (the prefetch condition differs from lane to lane and block to block); the same tiles in another order give
    the same digests."""
    tiles, first, second = lockstep_orders()
    got = []
    for order in (first, second):
        s = Session([tiles[i] for i in order])
        s.enc.run()
        dig, _ = s.enc.object_sha256()
        s.check_digests(dig)
        by_tile = np.zeros_like(dig)
        by_tile[order] = dig
        got.append(by_tile)
        s.close()
    np.testing.assert_array_equal(got[0], got[1])


def test_failed_tiles_among_good_ones(dc):
    """A tile refused on the host (sidelen 2048) and one refused by the kernel (an infinity) inside a wave of good tiles: their
    digests are 32 zero bytes, their CIDs None, and every neighbour's digest is still right."""
    tiles = list(S.table()[:64])
    inf = (np.arange(3 * 16 * 16).reshape(3, 16, 16) / 8.0).astype(np.float32)
    inf[1, 7, 3] = np.inf
    tiles[5] = Tile("host-refused-1x1500x8", np.zeros((1, 1500, 8), dtype=np.int32))
    tiles[40] = Tile("kernel-refused-inf", inf, bits=3)
    s = Session(tiles)
    s.enc.run()
    assert s.enc.result(5)[0] != 0 and s.enc.result(40)[0] == -2
    dig, _ = s.enc.object_sha256()
    assert not dig[5].any() and not dig[40].any()
    good = [c for c in tiles if c.ref is not None]
    assert len(good) == 62
    bad = [(i, c.name) for i, c in s.wrong_digests(dig)]
    assert not bad, bad
    s.check_bytes_and_cids()
    s.close()


@pytest.fixture(scope="module")
def split_tiles():
    """The long tiles of sha_cases.split_cases() and the table's side-16 tiles of four instants and more.  plan_split
    (k2r_session_plan.h) splits the tiles of a kernel class only when EVERY tile of the class has at least four instants, so no
    shorter tile of side 16 or 256 may join this session; the side-8 tiles (universal kernel, never split) ride along whole."""
    table = S.table()[:64]
    small = [c for c in table if c.array.shape[1] == 16 and c.array.shape[0] >= 4]
    whole = [c for c in table if c.array.shape[1] == 8][:6]
    assert len(small) >= 8 and len({c.residue for c in small}) == len(small) and len(whole) == 6
    return S.split_cases() + small + whole


@pytest.mark.parametrize("parts", ["2", "8"])
def test_first_accessor_of_an_unspliced_session(dc, monkeypatch, split_tiles, parts):
    """K2R_SPLIT=all: long tiles are encoded in speculative parts whose bytes are made contiguous only when somebody asks for them
    (materialize()).  object_sha256() is the FIRST accessor after run() here; fetch comes after."""
    monkeypatch.setenv("K2R_SPLIT", "all")
    monkeypatch.setenv("K2R_PARTS", parts)
    s = Session(split_tiles)
    s.enc.run()
    dig, _ = s.enc.object_sha256()
    s.check_digests(dig, "first accessor, %s parts: " % parts)
    s.check_bytes_and_cids()
    s.close()


def test_retried_slots_and_a_second_run(dc):
    """out_cap_per_tile = 256: all but the shortest tiles are re-encoded into slots of their own; digests after the first run() and
    again after a second."""
    tiles = S.table()
    assert sum(c.length > 256 for c in tiles) > 60 and any(c.length <= 256 for c in tiles)
    s = Session(tiles, out_cap_per_tile=256)
    for run in (1, 2):
        s.enc.run()
        dig, _ = s.enc.object_sha256()
        s.check_digests(dig, "run %d: " % run)
    s.check_bytes_and_cids()
    s.close()


def test_two_consecutive_calls_agree(dc):
    s = Session(S.table())
    s.enc.run()
    a, _ = s.enc.object_sha256()
    b, _ = s.enc.object_sha256()
    np.testing.assert_array_equal(a, b)
    s.check_digests(a)
    s.close()


def test_universal_kernel_k3(dc):
    """Another encoder, the same header: a k = 3 session (the universal kernel) over three tiles on three residues."""
    tiles = S.k3_cases()
    assert len({c.residue for c in tiles}) == 3
    s = Session(tiles, k=3)
    s.enc.run()
    assert all(s.enc.tile_kernel(i)[3] >> 8 == 3 for i in range(3))
    dig, _ = s.enc.object_sha256()
    s.check_digests(dig)
    s.check_bytes_and_cids()
    s.close()


def retry_tiles():
    """Side-16 int32 tiles of 8 instants -- with K2R_PARTS=4 each is cut into [0, 4), [4, 6), [6, 8) -- on one base image, named
    by what happens to their parts, plus a side-8 tile for the universal kernel.  `snap`: the instants the oracle stores as
    Snapshots."""
    rng = np.random.default_rng(0x5E55)
    base = np.zeros((8, 16, 16), dtype=np.int32) + 7
    base[:, :8, :8] = 9

    def noise_at(t, span):
        a = base.copy()
        a[t] = rng.integers(0, span, size=(16, 16))
        return a
    tiles = [S.Case("smooth", base), S.Case("snapshot-in-first-part", noise_at(2, 50)), S.Case("snapshot-in-middle-part", noise_at(5, 50)),
             S.Case("middle-part-then-too-big", noise_at(5, 1 << 20)), S.Case("too-big", rng.integers(0, 1 << 20, size=(8, 16, 16)).astype(np.int32)),
             S.Case("universal-5x8x8", rng.integers(-9, 9, size=(5, 8, 8)).astype(np.int32))]
    for c in tiles:
        c.snap = O.chunk_build(c.array, want_snapshots=True)[3]
    return tiles


@pytest.mark.parametrize("cap", [256, 1024])
def test_split_session_retries_and_runs_twice(dc, monkeypatch, cap):
    """One session, split tiles, small slots, run() twice: the retry loop of dcdf_encoder_run and the plan's book-keeping behind it
    (plan_retry, drop_parts: the parts of a tile that is whole from now on leave the queues and the splice tables) between two runs.
    After each run digests, bytes, CIDs, counters and a gather must equal the oracle's.

    cap = 256 is smaller than ANY 8-instant chunk of side 16 (the smallest, a constant tile, takes 334 bytes): every tile of the
    class comes back ST_OUT_CAPACITY and is whole, in a worst-case slot, from the first retry on; the second run has no parts.
    cap = 1024 is where the parts do different things, asserted below from the oracle's Snapshot positions and lengths: `smooth`
    splices in both runs; a Snapshot in [1, 4) or in [4, 6) is ST_RESPLIT and the tile then fits whole; a wider one in [4, 6) is
    ST_RESPLIT and then ST_OUT_CAPACITY (the second pass); `too-big` is ST_OUT_CAPACITY at once.  Nothing in the ABI tells a
    spliced tile from a whole one: which tiles the plan splits is pinned on the CPU (tests/test_session_plan_host.py)."""
    monkeypatch.setenv("K2R_SPLIT", "all")
    monkeypatch.setenv("K2R_PARTS", "4")
    tiles = retry_tiles()
    smooth, first, middle, middle_big, big, universal = tiles
    if cap == 1024:
        assert smooth.snap == [0] and smooth.length <= cap
        assert any(1 <= t < 4 for t in first.snap) and first.length <= cap
        assert all(t == 0 or t >= 4 for t in middle.snap) and any(4 <= t < 6 for t in middle.snap) and middle.length <= cap
        assert all(t == 0 or t >= 4 for t in middle_big.snap) and any(4 <= t < 6 for t in middle_big.snap) and middle_big.length > cap
        assert big.length > cap
    else:
        assert all(c.length > cap for c in tiles[:5])
    s = Session(tiles, out_cap_per_tile=cap)
    assert [s.enc.tile_kernel(i) for i in range(6)] == [(4, 0, 1, 0)] * 5 + [(-1, -1, -1, (2 << 8) | 3)]
    for run in (1, 2):
        s.enc.run()
        dig, _ = s.enc.object_sha256()
        s.check_digests(dig, "cap %d, run %d: " % (cap, run))
        s.check_bytes_and_cids()
        buf, offs, lens, mm = s.enc.gather()
        at = 0
        for i, c in enumerate(tiles):
            want = O.chunk_build(c.array, want_snapshots=True)
            assert s.enc.result(i) == (0, c.length, want[1], want[2]), (run, c.name)
            assert bytes(buf[int(offs[i]):int(offs[i]) + int(lens[i])]) == c.ref, (run, c.name)
            flat = c.array.reshape(c.array.shape[0], -1)
            np.testing.assert_array_equal(mm[at:at + len(flat)], np.stack([flat.min(1), flat.max(1)], axis=1), err_msg=c.name)
            at += len(flat)
        assert s.enc.total_bytes() == sum(c.length for c in tiles)
    s.close()
