"""Builds the device shading probes (shade_probe.hip) -- TEST INFRASTRUCTURE, not linked into librptr_hip.so.

shade_probe.hip includes csrc/dshade.h and calls its functions on chosen inputs; it is compiled with the product's own flags
(build.FLAGS: -ffp-contract=off, -fno-slp-vectorize, ...) once per build of the shading arithmetic: libshade_probe.so (IEEE,
-DRP_FAST_MATH=0) and libshade_probe_fast.so (-DRP_FAST_MATH=1). csrc_dir names the directory dshade.h / dmath.h are read from, so that
a modified copy of csrc/ can be probed."""
import os
import subprocess

from realtimepathtracingresearchframework_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "shade_probe.hip")
LIBS = {0: "libshade_probe.so", 1: "libshade_probe_fast.so"}
DEPENDS = ("dshade.h", "dmath.h")
# the ABI headers dshade.h includes: the probe passes RptrBaseMaterial / RptrSkyModelParams by value
ABI_HEADERS = [os.path.join(os.path.dirname(B.HERE), "include", f) for f in ("rptr_hip.h", "rptr_bvh.h")]


def lib_paths(out_dir=HERE):
    return {m: os.path.join(out_dir, name) for m, name in LIBS.items()}


def needs_build(out_dir=HERE, csrc_dir=B.CSRC):
    newest = max(os.path.getmtime(p) for p in [SOURCE] + ABI_HEADERS + [os.path.join(csrc_dir, f) for f in DEPENDS])
    return any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in lib_paths(out_dir).values())


def build(out_dir=HERE, csrc_dir=B.CSRC, verbose=False):
    """hipcc both probe libraries into out_dir; returns {fast_math: path}"""
    os.makedirs(out_dir, exist_ok=True)
    hipcc = B._hipcc()
    out = lib_paths(out_dir)
    # csrc_dir first: its dshade.h / dmath.h are the ones probed; the product's csrc/ after it resolves dshade.h's "../../include/..."
    # for a copy of csrc/ that lies elsewhere
    inc = ["-I" + os.path.abspath(csrc_dir), "-I" + B.CSRC]
    for m, path in out.items():
        cmd = [hipcc] + B.FLAGS + ["-DRP_FAST_MATH=%d" % m] + inc + ["-shared", SOURCE, "-o", path]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (path, r.stdout))
    return out
