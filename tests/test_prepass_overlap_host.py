"""The tiles of tests/prepass_overlap_cases.py without a GPU: the table holds what it claims (its own check, and its model of a Log
against the oracle's), and the kernel bodies (host simulator, which builds the snapshot side of the tree top once per block as
the card does) give the oracle's bytes for every tile, every Log from the stash.
tests/test_gpu_prepass_overlap.py runs the same tiles on the card."""
import ctypes

import numpy as np
import pytest

import emit_group_cases as G
import oracle_lib as O
import prepass_overlap_cases as P
import sim_lib as S

NAMES = [c.name for c in P.cases()]


@pytest.fixture(scope="module")
def refs():
    """name -> (bytes, snapshots, logs, snapshot instants) of the oracle, computed once."""
    return {c.name: O.chunk_build(c.array, want_snapshots=True) for c in P.cases()}


def stash_logs():
    S.lib().sim_last_stash_logs.restype = ctypes.c_uint32
    return S.lib().sim_last_stash_logs()


def test_table_holds_what_it_claims():
    seen = P.check_table()
    assert set(seen) == set(P.SIDES) | {64}  # (64: the control)


@pytest.mark.parametrize("name", ["S128-I1024-Q4096-mix", "resnap128"])
def test_model_of_a_log_is_the_oracles(name):
    c = P.case(name)
    a, snap = c.array, 0
    for t in range(1, a.shape[0]):
        if t in c.snapshots:
            snap = t
            continue
        L = G.LogStreams(a[snap], a[t])
        d = O.log_dump(a[snap], a[t])
        zmax = np.concatenate([L.zmax[h][L.visited[h]] for h in range(L.H, -1, -1)])
        zmin = np.concatenate([L.zmin[h][L.internal[h]] for h in range(L.H, 0, -1)])
        assert (G.zigzag(np.asarray(d["max"])) == zmax).all()
        assert (G.zigzag(np.asarray(d["min"])) == zmin).all()


@pytest.mark.parametrize("name", NAMES)
def test_simulator_emits_the_oracles_bytes_from_the_stash(name, refs):
    c = P.case(name)
    ref, rs, rl, snaps = refs[name]
    assert (rs, rl) == (len(c.snapshots), c.logs) and tuple(snaps) == c.snapshots
    st, data, ns, nl = S.encode(c.array)
    assert st == 0 and (ns, nl) == (rs, rl)
    assert stash_logs() == c.logs  # the path under test was the one taken
    assert data == ref
