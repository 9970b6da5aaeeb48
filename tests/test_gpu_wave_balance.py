"""The tiles of tests/wave_balance_cases.py on the card: from device memory through dcdf_amd.encoder.Encoder, against the CPU
oracle byte for byte.  The int32 tiles take k_encode<L, 0, 1> for L = 4, 6, 7, 8 -- a workgroup with no full wave, one wave, four
and sixteen, the last with every record count and placement of the table --; the float32 and int64 views of the one-wave tile
take the float and the wide-row kernel through the same code.  tests/test_wave_balance_host.py checks the table and runs it
through the host simulator."""
import numpy as np
import pytest

import oracle_lib as O
import wave_balance_cases as W

pytestmark = pytest.mark.gpu

FBITS = 3  # the float view stores exact multiples of 2^-3: its stored integers are the int32 tile's


def variants():
    out = [(c.name + "-int32", c.array, 0, 1) for c in W.cases()]
    a = W.case("S64").array
    out.append(("S64-float32", (a.astype(np.float64) / 2.0 ** FBITS).astype(np.float32), FBITS, 2))
    out.append(("S64-int64", a.astype(np.int64), 0, 3))
    return out


VARIANTS = variants()


@pytest.fixture(scope="module")
def dc():
    import dcdf_amd
    from dcdf_amd import _lib
    assert _lib.lib().dcdf_device_name(), "no GPU"
    return dcdf_amd


@pytest.mark.parametrize("name,array,bits,loader", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_device_tile_matches_the_oracle(dc, name, array, bits, loader):
    from dcdf_amd.encoder import DeviceBuffer, Encoder
    T, S, _ = array.shape
    if bits:
        assert ((array.astype(np.float64) * 2.0 ** bits).astype(np.int32) == W.case("S64").array).all()
    ref, rs, rl, _ = O.chunk_build(array, fractional_bits=bits, want_snapshots=True)
    assert (rs, rl) == (1, T - 1)
    buf = DeviceBuffer(array.nbytes)
    try:
        assert buf.ptr % 16 == 0
        buf.write(0, array)
        enc = Encoder([(buf.ptr, O.ENC[array.dtype], (S * S, S, 1), (T, S, S), bits, False)], k=2)
        try:
            enc.run()
            assert enc.tile_kernel(0) == (S.bit_length() - 1, 0, loader, 0)
            st, ln, ns, nl = enc.result(0)
            assert st == 0 and (ns, nl) == (rs, rl)
            data = enc.fetch(0)
            if data != ref:
                n = min(len(data), len(ref))
                first = next((j for j in range(n) if data[j] != ref[j]), n)
                raise AssertionError("bytes differ: len %d vs %d, first diff at %d" % (len(data), len(ref), first))
        finally:
            enc.close()
    finally:
        buf.free()
