"""Surface queries without a GPU: the C ABI, the record layout in the header, in ctypes and in numpy, the Python methods, the C++
adapter overloads and the code-object facts of the two kernels (tests/test_gpu_surface_queries.py runs them)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from code_object import kernel_regs
from realtimepathtracingresearchframework_amd import abi, backend, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rptr_hip_trace_surface", "rptr_hip_trace_surface_device"]
FIELDS = ["position", "t", "geo_normal", "instance_geometry", "normal", "primitive", "base_color", "roughness", "emission", "ior", "uv", "material_id", "metallic"]
OFFSETS = [0, 12, 16, 28, 32, 44, 48, 60, 64, 76, 80, 88, 92]  # six 16-byte rows (include/rptr_hip.h RptrSurfaceHit)


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rptr_hip.h")).read()
    L = backend.load_library()
    for name in NEW:
        assert re.search(r"^int %s\(rptr_hip_t \*h," % name, hdr, re.M), name
        assert name in abi.EXPORTED_SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert len(L.rptr_hip_trace_surface.argtypes) == 6 and len(L.rptr_hip_trace_surface_device.argtypes) == 7
    assert "#define RPTR_HIP_ABI_VERSION 5" in hdr and abi.ABI_VERSION == 5 and L.rptr_hip_abi_version() == 5
    assert L.rptr_hip_option_count() == 22


def test_the_record_has_one_layout_in_the_header_in_ctypes_and_in_numpy(tmp_path):
    """sizeof == 96 and the same field offsets three times"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rptr_hip.h"\nint main(void) {\n    printf("%zu", sizeof(RptrSurfaceHit));\n'
                   + "".join('    printf(" %%zu", offsetof(RptrSurfaceHit, %s));\n' % f for f in FIELDS) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[0] == 96 and got[1:] == OFFSETS
    assert C.sizeof(abi.SurfaceHit) == 96 and [n for n, _ in abi.SurfaceHit._fields_] == FIELDS
    assert [getattr(abi.SurfaceHit, f).offset for f in FIELDS] == OFFSETS
    dt = abi.SURFACE_HIT_DTYPE
    assert dt.itemsize == 96 and list(dt.names) == FIELDS and [dt.fields[f][1] for f in FIELDS] == OFFSETS
    for f in FIELDS:
        want = np.int32 if f in ("instance_geometry", "primitive", "material_id") else np.float32
        assert dt.fields[f][0].base == np.dtype(want), f
        assert dt.fields[f][0].itemsize == getattr(abi.SurfaceHit, f).size, f


def test_python_methods_have_the_documented_signature():
    p = inspect.signature(backend.RenderHip.render_surface_queries).parameters
    assert list(p) == ["self", "queries", "camera", "variant", "results"]
    assert (p["variant"].default, p["results"].default) == (abi.VARIANT_GLTF, None)
    d = inspect.signature(backend.RenderHip.render_surface_queries_device).parameters
    assert list(d) == ["self", "num_queries", "camera", "variant", "device_queries", "device_results", "stream"]
    assert (d["device_queries"].default, d["stream"].default) == (None, None)


def test_arguments_are_checked_before_the_device_is_touched():
    """NULL camera, NULL buffers, n < 0 and an unknown variant are refused with a message, without a handle or a GPU"""
    L = backend.load_library()
    cam = abi.Camera()
    q = np.zeros((2, 8), np.float32)
    out = np.zeros(2, abi.SURFACE_HIT_DTYPE)
    qp, op = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(what, rc):
        assert rc == abi.RPTR_E_INVALID, rc
        assert what in L.rptr_hip_last_error(None).decode(), L.rptr_hip_last_error(None)

    for device in (False, True):
        tail = (None,) if device else ()
        fn = L.rptr_hip_trace_surface_device if device else L.rptr_hip_trace_surface
        refused("NULL camera", fn(None, qp, 2, None, abi.VARIANT_GLTF, op, *tail))
        refused("n must be >= 0", fn(None, qp, -1, C.byref(cam), abi.VARIANT_GLTF, op, *tail))
        refused("NULL query or output buffer", fn(None, qp, 2, C.byref(cam), abi.VARIANT_GLTF, None, *tail))
        refused("unknown variant 17", fn(None, qp, 2, C.byref(cam), 17, op, *tail))
        refused("NULL handle", fn(None, qp, 2, C.byref(cam), abi.VARIANT_SIMPLE, op, *tail))
    refused("NULL query or output buffer", L.rptr_hip_trace_surface(None, None, 2, C.byref(cam), abi.VARIANT_GLTF, op))
    assert (out.view(np.uint8) == 0).all()


def test_cpp_overloads_compile_and_link(tmp_path):
    """RenderHip::render_surface_queries beside the radiance overloads: the backend's query buffer into a device buffer, and host arrays"""
    src = tmp_path / "sq.cpp"
    src.write_text('''#include "render_hip.hpp"
int main(int argc, char **) {
    if (argc < 100) return 0; // (compiled and linked, not run: no device here)
    rptr::RenderHip b;
    rptr::RenderCameraParams cam{};
    RptrRenderRayQuery q[2] = {};
    RptrSurfaceHit out[2] = {};
    static_assert(sizeof(out) == 192, "96 bytes per record");
    b.enable_ray_queries(16);
    bool ok = b.render_surface_queries(2, b.params, RPTR_VARIANT_GLTF, cam, out) && b.render_surface_queries(2, b.params, RPTR_VARIANT_SIMPLE, cam, out, nullptr) &&
              b.render_surface_queries(q, 2, b.params, RPTR_VARIANT_GLTF_TRANSMISSION, cam, out);
    return ok ? 0 : 1;
}
''')
    exe = str(tmp_path / "sq")
    libdir = os.path.dirname(build.LIB_PATH)
    if not os.path.exists(build.LIB_PATH):
        build.build_library()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), str(src), "-o", exe, "-L" + libdir, "-lrptr_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.call([exe]) == 0


def test_the_two_kernels_are_present_and_free_of_scratch():
    """rp_k_trace_surface<SINGLE>: both instantiations inside the traversal kernels' budget (six waves per SIMD: 80 VGPRs) without a
    private segment. rp_k_surface<VARIANT, TEX>: 3 x 2 instantiations, no private segment, no LDS; the ones without texture code are the
    small ones."""
    regs = kernel_regs()
    tr = {k: v for k, v in regs.items() if k.startswith("_Z18rp_k_trace_surfaceILb")}
    assert len(tr) == 2, sorted(tr)
    for k, v in tr.items():
        assert v[2] == 0 and v[0] <= 80, (k, v)
    de = {k: v for k, v in regs.items() if k.startswith("_Z12rp_k_surfaceILi")}
    assert len(de) == 6, sorted(de)
    for k, v in de.items():
        assert v[2] == 0 and v[3] == 0, (k, v)
    for variant in "012":
        tex, plain = de["_Z12rp_k_surfaceILi%sELb1E" % variant + _rest(de)], de["_Z12rp_k_surfaceILi%sELb0E" % variant + _rest(de)]
        assert plain[0] < tex[0], (variant, plain, tex)


def _rest(kernels):
    """what follows the template arguments in the (truncated) mangled names of the table"""
    name = next(iter(kernels))
    return name[len("_Z12rp_k_surfaceILi0ELb0E"):]
