"""The tiles of tests/emit_group_cases.py without a GPU: the table reaches what the emission of stash Logs can get wrong (its
own coverage check, and its model of a Log against the oracle's), and the kernel bodies (host simulator) give the oracle's
bytes for every tile -- from the stash, and with a stash too small to hold an instant, through the fallback.
tests/test_gpu_emit_groups.py runs the same tiles on the card."""
import ctypes

import numpy as np
import pytest

import emit_group_cases as G
import oracle_lib as O
import sim_lib as S

NAMES = [c.name for c in G.cases()]


@pytest.fixture(scope="module")
def refs():
    """name -> (bytes, snapshots, logs) of the oracle, computed once."""
    out = {}
    for c in G.cases():
        data, ns, nl, _ = O.chunk_build(c.array, want_snapshots=True)
        out[c.name] = (data, ns, nl)
    return out


def stash_logs():
    S.lib().sim_last_stash_logs.restype = ctypes.c_uint32
    return S.lib().sim_last_stash_logs()


def test_table_covers_the_grouped_forms():
    cov = G.check_table()
    assert cov.logs == sum(c.logs for c in G.cases())


@pytest.mark.parametrize("name", NAMES)
def test_model_of_a_log_is_the_oracles(name):
    """The coverage is computed from a restatement of Log::build on arrays: its streams are the oracle's."""
    a = G.case(name).array
    for t in range(1, a.shape[0]):
        L = G.LogStreams(a[0], a[t])
        d = O.log_dump(a[0], a[t])
        zmax = np.concatenate([L.zmax[h][L.visited[h]] for h in range(L.H, -1, -1)])
        zmin = np.concatenate([L.zmin[h][L.internal[h]] for h in range(L.H, 0, -1)])
        assert (G.zigzag(np.asarray(d["max"])) == zmax).all()
        assert (G.zigzag(np.asarray(d["min"])) == zmin).all()


@pytest.mark.parametrize("name", NAMES)
def test_every_instant_after_the_first_is_a_log(name, refs):
    _, ns, nl = refs[name]
    assert (ns, nl) == (1, G.case(name).logs)


@pytest.mark.parametrize("name", NAMES)
def test_simulator_emits_the_oracles_bytes_from_the_stash(name, refs):
    c = G.case(name)
    ref, rs, rl = refs[name]
    st, data, ns, nl = S.encode(c.array)
    assert st == 0 and (ns, nl) == (rs, rl)
    assert stash_logs() == c.logs  # the path under test was the one taken
    assert data == ref


@pytest.mark.parametrize("words", ["1", "4000"])
@pytest.mark.parametrize("name", NAMES)
def test_fallback_is_still_exact(name, words, refs, monkeypatch):
    c = G.case(name)
    ref, rs, rl = refs[name]
    monkeypatch.setenv("K2R_SIM_STASH_WORDS", words)
    st, data, ns, nl = S.encode(c.array)
    assert st == 0 and (ns, nl) == (rs, rl) and data == ref
    if words == "1":
        assert stash_logs() == 0
