"""The tiles of tests/wave_priority_cases.py on the card: all of them in ONE Encoder session, run three times, every tile fetched
after every run and compared with the CPU oracle byte for byte.  Wave priorities change timing only; a result that moved with
them -- or from one run to the next -- would mean that a barrier-free group of phases around phase 1 depends on which wave gets
there first."""
import numpy as np
import pytest

import oracle_lib as O
import wave_priority_cases as P

pytestmark = pytest.mark.gpu

RUNS = 3


@pytest.fixture(scope="module")
def refs():
    """name -> the oracle's bytes; every tile is one Snapshot and three Logs."""
    out = {}
    for name, a, bits, _ in P.tiles():
        data, ns, nl, _ = O.chunk_build(a, fractional_bits=bits, want_snapshots=True)
        assert (ns, nl) == (1, P.INSTANTS - 1), name
        out[name] = data
    return out


def test_one_session_three_runs_match_the_oracle(refs):
    import dcdf_amd  # noqa: F401
    from dcdf_amd import _lib as L
    from dcdf_amd.encoder import DeviceBuffer, Encoder, synth_fill
    assert L.lib().dcdf_device_name(), "no GPU"
    tiles = P.tiles()
    bufs, enc = [], None
    try:
        descs = []
        for name, a, bits, _ in tiles:
            T, S, _ = a.shape
            buf = DeviceBuffer(a.nbytes)
            bufs.append(buf)
            assert buf.ptr % 16 == 0
            if name.startswith("model") and a.dtype == np.int32:  # the model raster comes from the device generator
                i, j = (int(x) for x in name.split("-")[1:3])
                synth_fill(buf.ptr, L.DCDF_I32, P.SEED, 0, T, S * i, S * i + S, S * j, S * j + S)
                assert (buf.read(0, a.nbytes, np.int32).reshape(a.shape) == a).all(), name
            else:
                buf.write(0, a)
            descs.append((buf.ptr, O.ENC[a.dtype], (S * S, S, 1), (T, S, S), bits, False))
        enc = Encoder(descs, k=2)
        for run in range(RUNS):
            enc.run()
            for n, (name, a, bits, loader) in enumerate(tiles):
                assert enc.tile_kernel(n) == (a.shape[1].bit_length() - 1, 0, loader, 0), name
                st, ln, ns, nl = enc.result(n)
                assert st == 0 and (ns, nl) == (1, P.INSTANTS - 1), (name, run, st, ns, nl)
                data, ref = enc.fetch(n), refs[name]
                if data != ref:
                    m = min(len(data), len(ref))
                    first = next((j for j in range(m) if data[j] != ref[j]), m)
                    raise AssertionError("%s, run %d: bytes differ: len %d vs %d, first diff at %d" % (name, run, len(data), len(ref), first))
    finally:
        if enc is not None:
            enc.close()
        for b in bufs:
            b.free()
