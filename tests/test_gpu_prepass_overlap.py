"""The tiles of tests/prepass_overlap_cases.py on the card: from device memory through dcdf_amd.encoder.Encoder, against the CPU
oracle byte for byte.  The int32 tiles take k_encode<7, 0, 1> and k_encode<8, 0, 1> (four and sixteen waves, four and five levels
of the tree top) and k_encode<6, 0, 1> (one wave: the control); the float32 and int64 views of one sidelen-128 tile take the
other loaders' kernels through the same phase; one tile goes through the speculative parts, whose continuations have
to build the snapshot side of the top in their first instant.  tests/test_prepass_overlap_host.py checks the table and runs it
through the host simulator."""
import numpy as np
import pytest

import oracle_lib as O
import prepass_overlap_cases as P

pytestmark = pytest.mark.gpu

FBITS = 3  # the float view stores exact multiples of 2^-3: its stored integers are the int32 tile's


def variants():
    out = [(c.name + "-int32", c.array, 0, 1) for c in P.cases()]
    a = P.loader_case().array
    out.append((P.loader_case().name + "-float32", (a.astype(np.float64) / 2.0 ** FBITS).astype(np.float32), FBITS, 2))
    out.append((P.loader_case().name + "-int64", a.astype(np.int64), 0, 3))
    return out


VARIANTS = variants()


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


@pytest.fixture(scope="module")
def refs():
    """id -> (bytes, snapshots, logs, snapshot instants) of the oracle, computed once."""
    return {name: O.chunk_build(array, fractional_bits=bits, want_snapshots=True) for name, array, bits, _ in VARIANTS}


def encode_on_device(array, bits):
    from dcdf_amd.encoder import DeviceBuffer, Encoder
    T, S, _ = array.shape
    buf = DeviceBuffer(array.nbytes)
    try:
        assert buf.ptr % 16 == 0
        buf.write(0, array)
        enc = Encoder([(buf.ptr, O.ENC[array.dtype], (S * S, S, 1), (T, S, S), bits, False)], k=2)
        try:
            enc.run()
            return enc.tile_kernel(0), enc.result(0), enc.fetch(0)
        finally:
            enc.close()
    finally:
        buf.free()


def same_bytes(data, ref):
    if data != ref:
        n = min(len(data), len(ref))
        first = next((j for j in range(n) if data[j] != ref[j]), n)
        raise AssertionError("bytes differ: len %d vs %d, first diff at %d" % (len(data), len(ref), first))


@pytest.mark.parametrize("name,array,bits,loader", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_device_tile_matches_the_oracle(dc, refs, name, array, bits, loader):
    T, S, _ = array.shape
    if bits:
        assert ((array.astype(np.float64) * 2.0 ** bits).astype(np.int32) == P.loader_case().array).all()
    ref, rs, rl, _ = refs[name]
    kernel, (st, ln, ns, nl), data = encode_on_device(array, bits)
    assert kernel == (S.bit_length() - 1, 0, loader, 0)
    assert st == 0 and (ns, nl) == (rs, rl)
    same_bytes(data, ref)


@pytest.mark.parametrize("parts", ["2", "4"])
def test_continuation_parts_build_the_snapshot_side(dc, refs, monkeypatch, parts):
    """K2R_SPLIT=all: the tile is encoded as [0, 4) [4, 8) or [0, 4) [4, 6) [6, 8) by different workgroups and spliced.  A
    continuation compares with a snapshot it never encoded: its first instant has to build smin / smax, its later ones reuse them."""
    monkeypatch.setenv("K2R_SPLIT", "all")
    monkeypatch.setenv("K2R_PARTS", parts)
    c = P.case("parts128")
    ref, rs, rl, _ = refs["parts128-int32"]
    assert (rs, rl) == (1, 7)  # the speculation holds: no block boundary after instant 0
    kernel, (st, ln, ns, nl), data = encode_on_device(c.array, 0)
    assert kernel == (7, 0, 1, 0)
    assert st == 0 and (ns, nl) == (rs, rl)
    same_bytes(data, ref)
