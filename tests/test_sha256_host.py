"""The host SHA-256 (dcdf_amd/csrc/k2r_sha256_host.h: the hash of every object dcdf_superchunk_build returns to host memory) against
hashlib, without a GPU: tests/sim/sha256_check.cpp, a stand-alone program over the header alone, built with AddressSanitizer and
UBSan and run as its own process.  Messages of every length 0..300 at three misalignments, the lengths around every padding
boundary, one of 1 MiB -- each read from an allocation that ends with the message; both block functions (the portable one and the
x86 SHA extensions) on the same random states."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def messages():
    """[(offset, bytes)]: every length 0..300 at offsets 0, 1 and 7; 64 n - 9, 64 n - 8, 64 n, 64 n + 1 for n = 1..4 by name
    (total % 64 == 55: the last one-block padding; 56: the first two-block one; 0 and 1: around a block's end); 1 MiB."""
    rng = np.random.default_rng(256)
    out = [(off, rng.bytes(n)) for n in range(301) for off in (0, 1, 7)]
    for n in range(1, 5):
        out += [(off, rng.bytes(ln)) for ln in (64 * n - 9, 64 * n - 8, 64 * n, 64 * n + 1) for off in (0, 1, 7)]
    out.append((1, rng.bytes(1 << 20)))
    return out


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """The program built and run once: (stdout lines, the lengths it was given)."""
    tmp_path = tmp_path_factory.mktemp("sha256_check")
    exe = str(tmp_path / "sha256_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-o", exe, os.path.join(HERE, "sim", "sha256_check.cpp")])
    msgs = messages()
    src = tmp_path / "cases.txt"
    with open(src, "w") as f:
        for off, m in msgs:
            f.write("%d %d %s %s\n" % (off, len(m), hashlib.sha256(m).hexdigest(), m.hex() or "-"))
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])  # (a sanitizer report ends the program with its own status)
    lines = out.stdout.split("\n")[:-1]
    print("\n".join(l for l in lines if not l.startswith("MISMATCH")))
    assert "messages %d" % len(msgs) in lines and "states 300" in lines, lines[-5:]
    lens = {len(m) for _, m in msgs}
    assert set(range(301)) <= lens and {64 * n + d for n in range(1, 5) for d in (-9, -8, 0, 1)} <= lens and (1 << 20) in lens
    return lines


def mismatches(lines, checks):
    """The MISMATCH lines of the given checks; each names the message's length and offset."""
    bad = [l for l in lines if l.startswith("MISMATCH") and l.split()[1] in checks]
    assert all(re.match(r"MISMATCH \S+ len=\d+ offset=\d+", l) for l in bad)
    return bad


def test_portable_leg(report):
    """Must pass everywhere: sha256_host (the padding, over whichever block function this CPU dispatches to) gives hashlib's digest
    for every message; blocks_portable gives it too; blocks_portable and the dispatching blocks leave identical states."""
    assert "impl portable ran" in report
    assert "dispatch shani" in report or "dispatch portable" in report
    bad = mismatches(report, ("host", "portable", "state-dispatch", "state-zero-blocks"))
    assert not bad, "%d wrong, at lengths %% 64 = %s:\n%s" % (len(bad), sorted({int(re.search(r"len=(\d+)", l).group(1)) % 64 for l in bad}),
                                                            "\n".join(bad[:12]))


def test_sha_extension_leg(report):
    """blocks_shani gives hashlib's digest for every message and leaves the states blocks_portable leaves -- skipped only where the
    program reports that this CPU has no SHA extensions."""
    if "impl shani absent" in report:
        pytest.skip("tests/sim/sha256_check reports no x86 SHA extensions (sha, sse4.1, ssse3) on this CPU: blocks_shani cannot run here")
    assert "impl shani ran" in report and "dispatch shani" in report
    bad = mismatches(report, ("shani", "state-shani"))
    assert not bad, "%d wrong, at lengths %% 64 = %s:\n%s" % (len(bad), sorted({int(re.search(r"len=(\d+)", l).group(1)) % 64 for l in bad}),
                                                            "\n".join(bad[:12]))
