#!/usr/bin/env python3
"""Per-kernel resources of built objects, from the gfx950 code object's notes: VGPRs, AGPRs, SGPRs, scratch bytes per lane,
LDS bytes, how many ds_ / flat_ instructions the kernel has, and a hash of its instruction text (the disassembly without the
address and encoding columns and without the s_nop / zero padding behind its end, which depends on what follows the kernel in its
object: equal hashes = the same instructions).  One JSON object per object file on stdout:

    tools/kernel_resources.py dcdf_amd/csrc/_build/k2r_open.o dcdf_amd/csrc/_build/k2r_query.o dcdf_amd/csrc/_build/k2r_raster.o

Two builds are compared by diffing the output (the query kernels before and after the bulk decoder)."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def resources(obj):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}", "--unbundle"])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
        dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", co], text=True)
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        blk = ".agpr_count:" + blk
        f = {k: int(v) for k, v in re.findall(r"\.(agpr_count|group_segment_fixed_size|private_segment_fixed_size|sgpr_count|vgpr_count|"
                                              r"sgpr_spill_count|vgpr_spill_count):\s*(\d+)", blk)}
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        out[name] = {"vgpr": f.get("vgpr_count"), "agpr": f.get("agpr_count"), "sgpr": f.get("sgpr_count"),
                     "scratch": f.get("private_segment_fixed_size"), "lds": f.get("group_segment_fixed_size"),
                     "vgpr_spill": f.get("vgpr_spill_count", 0), "sgpr_spill": f.get("sgpr_spill_count", 0), "ds": 0, "flat": 0}
    cur = None
    text = {name: [] for name in out}
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
        elif cur in out:
            out[cur]["ds"] += bool(re.search(r"\sds_", line))
            out[cur]["flat"] += bool(re.search(r"\sflat_(load|store|atomic)", line))
            text[cur].append(line.split("//")[0].strip())
    for name, lines in text.items():
        while lines and lines[-1] in ("", "s_nop 0", "..."):
            lines.pop()
        out[name]["text_sha"] = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
    return out


if __name__ == "__main__":
    for o in sys.argv[1:]:
        print(json.dumps({os.path.basename(o): resources(o)}, indent=1, sort_keys=True))
