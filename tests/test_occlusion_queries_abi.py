"""Occlusion queries without a GPU: the C ABI, the parameter block in the header, in ctypes and in the C++ mirror, the refusals that need
neither a handle nor a device, the bit packing of the Python methods and the code-object facts of the kernel
(tests/test_gpu_occlusion_queries.py runs it)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from code_object import kernel_regs
from realtimepathtracingresearchframework_amd import abi, backend, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rptr_hip_occlusion_defaults": 1, "rptr_hip_trace_occlusion": 5, "rptr_hip_trace_occlusion_device": 6}  # argument counts of the header's prototypes


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    L = backend.load_library()
    assert re.search(r"^void rptr_hip_occlusion_defaults\(RptrOcclusionParams \*out\);", hdr, re.M)
    for name in ("rptr_hip_trace_occlusion", "rptr_hip_trace_occlusion_device"):
        assert re.search(r"^int %s\(rptr_hip_t \*h," % name, hdr, re.M), name
    for name, nargs in NEW.items():
        assert name in abi.EXPORTED_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == nargs, name
    assert "#define RPTR_HIP_ABI_VERSION 5" in hdr and abi.ABI_VERSION == 5 and L.rptr_hip_abi_version() == 5
    assert L.rptr_hip_option_count() == 22
    assert re.search(r"^#define RPTR_OCCLUSION_ALPHA_CUTOUT 1u$", hdr, re.M) and abi.OCCLUSION_ALPHA_CUTOUT == 1


def test_the_parameter_block_has_one_layout_in_c_in_ctypes_and_in_the_cpp_mirror(tmp_path):
    """sizeof == 16 and the same offsets in a C program compiled against the header and in ctypes; host/render_hip.hpp asserts the size"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rptr_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu", sizeof(RptrOcclusionParams), offsetof(RptrOcclusionParams, flags), offsetof(RptrOcclusionParams, alpha_cutoff),\n'
                   '           offsetof(RptrOcclusionParams, reserved));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [16, 0, 4, 8]
    P = abi.OcclusionParams
    assert C.sizeof(P) == 16 and [n for n, _ in P._fields_] == ["flags", "alpha_cutoff", "reserved"]
    assert (P.flags.offset, P.alpha_cutoff.offset, P.reserved.offset, P.reserved.size) == (0, 4, 8, 8)
    hpp = open(os.path.join(os.path.dirname(build.LIB_PATH), "host", "render_hip.hpp")).read()
    assert re.search(r"static_assert\(sizeof\(RptrOcclusionParams\) == 16,", hpp)


def test_cpp_overloads_compile_and_link(tmp_path):
    """RenderHip::render_occlusion_queries beside the surface-query overloads (this compiles the mirror's static_assert too): the backend's
    query buffer into device words, and host arrays"""
    src = tmp_path / "oq.cpp"
    src.write_text('''#include "render_hip.hpp"
int main(int argc, char **) {
    if (argc < 100) return 0; // (compiled and linked, not run: no device here)
    rptr::RenderHip b;
    RptrRenderRayQuery q[40] = {};
    uint32_t bits[2] = {};
    b.enable_ray_queries(64);
    bool ok = b.render_occlusion_queries(40, bits) && b.render_occlusion_queries(40, bits, 0.5f, nullptr) && b.render_occlusion_queries(q, 40, bits) &&
              b.render_occlusion_queries(q, 40, bits, 0.25f);
    return ok ? 0 : 1;
}
''')
    exe = str(tmp_path / "oq")
    libdir = os.path.dirname(build.LIB_PATH)
    if not os.path.exists(build.LIB_PATH):
        build.build_library()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), str(src), "-o", exe, "-L" + libdir, "-lrptr_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.call([exe]) == 0


def test_defaults():
    L = backend.load_library()
    p = abi.OcclusionParams(0xFFFFFFFF, 7.0, (9, 9))
    L.rptr_hip_occlusion_defaults(C.byref(p))
    assert (p.flags, p.alpha_cutoff, list(p.reserved)) == (0, 0.5, [0, 0])
    L.rptr_hip_occlusion_defaults(None)  # (nothing to fill: no fault)


def test_python_methods_have_the_documented_signature():
    p = inspect.signature(backend.RenderHip.render_occlusion_queries).parameters
    assert list(p) == ["self", "queries", "alpha_cutoff", "results"]
    assert (p["alpha_cutoff"].default, p["results"].default) == (None, None)
    d = inspect.signature(backend.RenderHip.render_occlusion_queries_device).parameters
    assert list(d) == ["self", "num_queries", "alpha_cutoff", "device_queries", "device_bits", "stream"]
    assert all(d[k].default is None for k in list(d)[2:])


def test_arguments_are_checked_before_the_device_is_touched():
    """every refusal that needs no handle: n < 0, NULL buffers with n > 0, reserved words, unknown flags, cutoffs 0, < 0, > 1, NaN, inf,
    NULL handle -- RPTR_E_INVALID with a message, the result words untouched"""
    L = backend.load_library()
    q = np.zeros((40, 8), np.float32)
    bits = np.full(2, 0xA5A5A5A5, np.uint32)
    qp, bp = q.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p)

    def refused(what, rc):
        assert rc == abi.RPTR_E_INVALID, (what, rc)
        assert what in L.rptr_hip_last_error(None).decode(), (what, L.rptr_hip_last_error(None))

    def P(flags=0, cutoff=0.5, reserved=(0, 0)):
        return C.byref(abi.OcclusionParams(flags, cutoff, reserved))

    CUT = abi.OCCLUSION_ALPHA_CUTOUT
    for device in (False, True):
        tail = (None,) if device else ()
        fn = L.rptr_hip_trace_occlusion_device if device else L.rptr_hip_trace_occlusion
        refused("n must be >= 0", fn(None, qp, -1, None, bp, *tail))
        refused("NULL query or result buffer", fn(None, qp, 40, None, None, *tail))
        refused("reserved words must be 0", fn(None, qp, 40, P(reserved=(0, 1)), bp, *tail))
        refused("reserved words must be 0", fn(None, qp, 40, P(reserved=(5, 0)), bp, *tail))
        refused("unknown flag bits 0x2", fn(None, qp, 40, P(flags=2), bp, *tail))
        refused("unknown flag bits 0x80000000", fn(None, qp, 40, P(flags=0x80000001), bp, *tail))
        for bad in (0.0, -0.25, 1.5, float("nan"), float("inf"), float("-inf")):
            refused("alpha_cutoff must be finite and in (0, 1]", fn(None, qp, 40, P(CUT, bad), bp, *tail))
        # well-formed arguments reach the handle check -- without the flag the cutoff is not read
        for ok in (None, P(), P(CUT, 0.5), P(CUT, 1.0), P(CUT, 2.0 ** -20), P(0, float("nan"))):
            refused("NULL handle", fn(None, qp, 40, ok, bp, *tail))
        refused("NULL handle", fn(None, None, 0, None, None, *tail))  # (n == 0 needs no buffers, but a handle)
    refused("NULL query or result buffer", L.rptr_hip_trace_occlusion(None, None, 40, None, bp))
    assert (bits == 0xA5A5A5A5).all()


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 64, 65])
def test_python_pack_and_unpack_round_trip_in_little_endian_bit_order(n):
    R = backend.RenderHip
    rng = np.random.default_rng(100 + n)
    b = rng.integers(0, 2, n).astype(bool)
    w = R.pack_occlusion_bits(b)
    assert w.dtype == np.uint32 and w.shape == ((n + 31) // 32,)
    for k in range(n):  # query q is bit q & 31 of word q >> 5
        assert bool((int(w[k >> 5]) >> (k & 31)) & 1) == bool(b[k]), k
    if n % 32:
        assert int(w[-1]) >> (n % 32) == 0  # the padding is clear
    back = R.unpack_occlusion_bits(w, n)
    assert back.dtype == np.bool_ and np.array_equal(back, b)
    # the bools of skipped queries survive a run that answers the others: what render_occlusion_queries does around the C call
    skipped = rng.integers(0, 2, n).astype(bool)
    answers = rng.integers(0, 2, n).astype(bool)
    words = R.pack_occlusion_bits(b)
    for k in np.flatnonzero(~skipped):  # (the kernel's rule: set or clear the query's own bit)
        words[k >> 5] = (int(words[k >> 5]) & ~(1 << (k & 31))) | (int(answers[k]) << (k & 31))
    assert np.array_equal(R.unpack_occlusion_bits(words, n), np.where(skipped, b, answers))


def test_the_kernels_are_present_and_free_of_scratch():
    """rp_k_trace_occlusion<ALPHA, SINGLE>: the opaque and the cutout instantiation, each for scenes with one instance record and for the
    two-level walk, without a private segment and inside the VGPR budget of their launch bounds (csrc/occlusion_query.h: eight, six and
    five waves per SIMD -- 64, 80 and 96 registers). Metadata of the gfx950 code object only."""
    regs = kernel_regs()
    k = {name[len("_Z20rp_k_trace_occlusionIL"):][:8]: v for name, v in regs.items() if name.startswith("_Z20rp_k_trace_occlusionILb")}
    assert sorted(k) == ["b0ELb0EE", "b0ELb1EE", "b1ELb0EE", "b1ELb1EE"], sorted(regs)[:4]
    budget = {"b0ELb1EE": 64, "b0ELb0EE": 80, "b1ELb1EE": 96, "b1ELb0EE": 96}
    for inst, (vgpr, _, scratch, lds) in k.items():
        assert scratch == 0 and vgpr <= budget[inst], (inst, vgpr, scratch)
        assert lds >= 20 * 256 * 4, (inst, lds)  # the traversal stacks
