#!/usr/bin/env python3
"""Carry profiles/pmc_latest.json over a source change that leaves the scene
kernels' machine code unchanged (comments, diagnostic-only code).

    python tools/restamp_pmc.py <git-rev the summary was profiled at> [names.json]

Compiles the frame kernels (rt_kernels.hip, and rt_compat.hip and
rt_records.hip where the tree has them) to gfx950 assembly at <rev> and in the working tree (the Makefile's
device flags) and restamps every entry with this tree's kernel_source_id only
if tools/isa_diff.py finds every kernel identical (names.json: its table of
renamed kernels).  Records the old stamp and the reason.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FLAGS = ["-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
         "-munsafe-fp-atomics", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp",
         "-fno-slp-vectorize", "--offload-device-only", "-S"]


def isa(src_dir: str) -> str:
    text = []
    for unit in ("rt_kernels", "rt_compat", "rt_records"):
        if os.path.exists(os.path.join(src_dir, unit + ".hip")):
            out = os.path.join(src_dir, unit + ".restamp.s")
            subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, unit + ".hip", "-o", out], cwd=src_dir,
                                  stderr=subprocess.DEVNULL)
            text.append(open(out).read())
            os.remove(out)
    return "\n".join(text)


def main():
    rev = sys.argv[1]
    names = json.load(open(sys.argv[2])) if len(sys.argv) > 2 else {}
    from raytracingstudy_amd._lib import kernel_source_id
    from isa_diff import compare
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(f"git -C {ROOT} archive {rev} raytracingstudy_amd/csrc include | tar x -C {td}",
                              shell=True)
        old = isa(os.path.join(td, "raytracingstudy_amd", "csrc"))
    new = isa(os.path.join(ROOT, "raytracingstudy_amd", "csrc"))
    got = compare(old, new, names, out=open(os.devnull, "w"))
    if got.count("identical") != len(got):
        print(f"machine code differs from {rev}: re-profile (tools/profile.sh)")
        return 1
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    pm = json.load(open(path))
    sid = kernel_source_id()
    for ent in (pm.values() if "config" not in pm else [pm]):
        if ent.get("kernel_source_id") != sid:
            ent.setdefault("restamped", []).append(
                {"from": ent["kernel_source_id"], "rev": rev,
                 "reason": "gfx950 ISA of the frame kernels identical (tools/restamp_pmc.py)"})
            ent["kernel_source_id"] = sid
    json.dump(pm, open(path, "w"), indent=1)
    print(f"restamped to {sid}: {len(got)} kernels identical to {rev}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
