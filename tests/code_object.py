"""Metadata of the gfx950 code objects of a library build, read once: what the register / scratch / LDS pins of the CPU tests look at."""
import os
import re
import shutil
import subprocess

import pytest

from realtimepathtracingresearchframework_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def kernel_regs(lib_path=None):
    """{mangled kernel name (as tools/kernel_regs.sh prints it: the first 70 characters): (vgpr, sgpr, scratch bytes, lds bytes)} of every
    kernel of the library (default: the product, built first if it is missing). Skips the calling test without llvm-objdump. One run of the
    tool per library file and modification time; callers must not change the dictionary."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or shutil.which("bash") is None:
        pytest.skip("no llvm-objdump")
    if lib_path is None:
        lib_path = build.LIB_PATH
        if not os.path.exists(lib_path):
            build.build_library()
    key = (os.path.abspath(lib_path), os.path.getmtime(lib_path))
    if key not in _cache:
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), lib_path], stdout=subprocess.PIPE, universal_newlines=True,
                             check=True, cwd=ROOT, timeout=300).stdout
        regs = {}
        for line in out.splitlines():
            m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+lds\s+(\d+)", line)
            if m:
                regs[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
        _cache[key] = regs
    return _cache[key]
