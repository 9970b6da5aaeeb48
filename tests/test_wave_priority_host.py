"""Wave priorities (k2r_exec.h: prio) without a GPU.

  * The sequential context has no waves to arbitrate: SimExec::prio<P>() is empty, and since the host compiler knows no
    __builtin_amdgcn_s_setprio the simulator builds only if nothing of the priority code reaches it.  It builds from the same
    headers, and gives the oracle's bytes for a sidelen-256 and a sidelen-128 tile of tests/wave_priority_cases.py.
  * The built objects hold the priority instructions the kept steps imply, and only where a SIMD holds several waves of the
    workgroup (sidelen 256): the ladder of the lean phase 1 is four instructions -- s_setprio 3, 2, 1, 0 at the head of its four
    passes -- in every unpadded sidelen-256 kernel; the padded one never takes the lean phase 1 and has none; the kernels for
    sidelens 16 to 128 have none."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
import sim_lib as S
import wave_priority_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "dcdf_amd", "csrc", "_build")
sys.path.insert(0, os.path.join(ROOT, "tools"))

LADDER = ["s_setprio 3", "s_setprio 2", "s_setprio 1", "s_setprio 0"]  # what each unpadded sidelen-256 kernel holds, in this order


def test_views_hold_the_int32_tile():
    t = {name: a for name, a, _, _ in P.tiles()}
    assert ((t["model-0-0-float32"].astype(np.float64) * 2.0 ** P.FBITS).astype(np.int32) == t["model-0-0-int32"]).all()
    assert (t["model-0-0-int64"] == t["model-0-0-int32"]).all()
    assert sum(1 for name, a, _, _ in P.tiles() if a.shape[1] == 256 and a.dtype == np.int32) >= 20


@pytest.mark.parametrize("name", ["model-1-2-int32", "S128-int32"])
def test_simulator_builds_without_priorities_and_matches_the_oracle(name):
    S.lib()  # make -C tests/sim: the host compiler sees every header the kernels are built from
    a, bits = next((a, bits) for n, a, bits, _ in P.tiles() if n == name)
    ref, rs, rl, _ = O.chunk_build(a, fractional_bits=bits, want_snapshots=True)
    assert (rs, rl) == (1, P.INSTANTS - 1)
    st, data, ns, nl = S.encode(a, fractional_bits=bits)
    assert st == 0 and (ns, nl) == (rs, rl)
    assert data == ref


def priority_instructions(obj):
    """The s_setprio instructions of an object's gfx950 code, in address order (extracted as tools/check_codegen.py does)."""
    import check_codegen as K
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([f"{K.LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj])
        subprocess.check_call([f"{K.LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}", "--unbundle"])
        dis = subprocess.check_output([f"{K.LLVM}/llvm-objdump", "-d", co], text=True)
    return [" ".join(m.group(0).split()) for m in re.finditer(r"\bs_setprio\s+\d+", dis)]


@pytest.mark.skipif(not glob.glob(os.path.join(BUILD, "enc_L*.o")), reason="no built encoder objects (dcdf_amd/csrc/_build)")
def test_priority_instructions_of_the_built_objects():
    objs = sorted(glob.glob(os.path.join(BUILD, "enc_L*.o")))
    assert len(objs) == 30
    with ThreadPoolExecutor(8) as pool:  # (the work is in the LLVM tools' processes)
        got = list(pool.map(priority_instructions, objs))
    for o, g in zip(objs, got):
        name = os.path.basename(o)
        want = LADDER if name.startswith("enc_L8_P0_") else []
        assert g == want, name
