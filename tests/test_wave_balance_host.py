"""The tiles of tests/wave_balance_cases.py without a GPU: the table holds what it claims (its own check, and its model of a Log
against the oracle's), and the kernel bodies (host simulator, which walks the same thread-to-work mapping as the card) give
the oracle's bytes for every tile, every Log from the stash.  tests/test_gpu_wave_balance.py runs the same tiles on the card."""
import ctypes

import numpy as np
import pytest

import emit_group_cases as G
import oracle_lib as O
import sim_lib as S
import wave_balance_cases as W

NAMES = [c.name for c in W.cases()]


@pytest.fixture(scope="module")
def refs():
    """name -> (bytes, snapshots, logs) of the oracle, computed once."""
    out = {}
    for c in W.cases():
        data, ns, nl, _ = O.chunk_build(c.array, want_snapshots=True)
        out[c.name] = (data, ns, nl)
    return out


def stash_logs():
    S.lib().sim_last_stash_logs.restype = ctypes.c_uint32
    return S.lib().sim_last_stash_logs()


def test_table_holds_the_wanted_counts():
    got = W.check_table()
    assert got["I"] >= set(W.I_COUNTS) and got["Q"] >= set(W.Q_COUNTS)


def test_rotated_items_are_a_permutation_that_keeps_waves_whole():
    """The mapping of k2r_exec.h restated: wave v takes the items of wave (v + rot) % NW, lanes keep their place."""
    for nt in (4, 64, 256, 1024):
        nw = max(1, nt // 64)
        tid = np.arange(nt)
        for rot in range(nw):
            item = tid if nt <= 64 else (((tid >> 6) + rot) % nw) * 64 + (tid & 63)
            assert sorted(item.tolist()) == tid.tolist()
            assert ((item & 63) == (tid & 63)).all() or nt < 64
            if nt <= 64:
                assert (item == tid).all()


@pytest.mark.parametrize("name", ["S64", "I1025-Q1024-spread", "top256"])
def test_model_of_a_log_is_the_oracles(name):
    a = W.case(name).array
    for t in range(1, a.shape[0]):
        L = G.LogStreams(a[0], a[t])
        d = O.log_dump(a[0], a[t])
        zmax = np.concatenate([L.zmax[h][L.visited[h]] for h in range(L.H, -1, -1)])
        zmin = np.concatenate([L.zmin[h][L.internal[h]] for h in range(L.H, 0, -1)])
        assert (G.zigzag(np.asarray(d["max"])) == zmax).all()
        assert (G.zigzag(np.asarray(d["min"])) == zmin).all()


@pytest.mark.parametrize("name", NAMES)
def test_simulator_emits_the_oracles_bytes_from_the_stash(name, refs):
    c = W.case(name)
    ref, rs, rl = refs[name]
    assert (rs, rl) == (1, c.logs)  # every instant after the first is a Log
    st, data, ns, nl = S.encode(c.array)
    assert st == 0 and (ns, nl) == (rs, rl)
    assert stash_logs() == c.logs  # the path under test was the one taken
    assert data == ref
