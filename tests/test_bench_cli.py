"""bench.py's options and its --dump-outputs writer, without a GPU (the encoder session is a stand-in)."""
import hashlib
import os

import numpy as np

import bench


def test_plain_run_leaves_the_side_measurements_off():
    a = bench.parse_args(["--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full) == (7, 3, False)
    assert (a.cpu_sample, a.verify, a.host_sample, a.decode_queries, a.also) == (0, 0, 0, 0, "")
    assert bench.parse_args(["--verify", "2"]).verify == 2  # an explicit value still holds


def test_full_run_keeps_the_former_defaults():
    a = bench.parse_args(["--full"])
    assert (a.cpu_sample, a.verify, a.host_sample, a.decode_queries, a.also) == (24, 4, 1024, 200000, "i64,f32,f64")
    assert bench.parse_args(["--full", "--also="]).also == ""


class _Session:
    """What bench.py's dump reads from an Encoder: results, and the gathered {bytes, offsets, lengths, minmax}."""

    def __init__(self, n, seed=1):
        rng = np.random.default_rng(seed)
        self.n = n
        self.lens = rng.integers(200_000, 1_500_000, n).astype(np.uint64)
        self.offs = np.zeros(n, dtype=np.uint64)
        self.offs[1:] = np.cumsum((self.lens[:-1] + np.uint64(15)) & ~np.uint64(15))
        self.buf = rng.integers(0, 256, int(self.offs[-1] + self.lens[-1]), dtype=np.uint8)
        self.mm = rng.integers(-4096, 4096, (n * 32, 2)).astype(np.int64)

    def gather(self):
        return self.buf, self.offs, self.lens, self.mm

    def result(self, i):
        return 0, int(self.lens[i]), 1, 31

    def chunk(self, i):
        return self.buf[int(self.offs[i]):int(self.offs[i] + self.lens[i])]


def test_dump_outputs(tmp_path):
    s = _Session(200)
    ids = list(range(1000, 1200))
    bench.dump_outputs(str(tmp_path / "a"), s, ids)
    bench.dump_outputs(str(tmp_path / "b"), s, ids)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in ("chunk_ids", "chunk_results", "minmax", "chunk_sha256", "encoded_sample",
                                                 "encoded_sample_chunks"))
    load = lambda d, k: np.load(str(tmp_path / d / (k + ".npy")))
    for f in names:
        a, b = load("a", f[:-4]), load("b", f[:-4])
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)  # the same inputs give the same files
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in names) <= 64_000_000
    assert np.array_equal(load("a", "minmax"), s.mm)
    assert np.array_equal(load("a", "chunk_results")[:, 1], s.lens.astype(np.float64))
    for i in (0, 57, 199):
        assert bytes(load("a", "chunk_sha256")[i].astype(np.uint8)) == hashlib.sha256(s.chunk(i)).digest()
    picked = load("a", "encoded_sample_chunks").astype(int) - 1000
    assert len(picked) > 0
    want = np.concatenate([s.chunk(i) for i in picked])
    assert np.array_equal(load("a", "encoded_sample"), want.astype(np.float32))
    assert want.size <= bench.DUMP_SAMPLE_BYTES
