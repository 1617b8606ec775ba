"""Generates the stored outputs of the reference's own programs (oracle/_ref, built by `make -C oracle ref` from the reference
checkout) that the tests hold the package against where oracle/_ref was not built:

  tests/golden/ref_abi.json               libabi_ref.so's report of the reference's struct layouts, defaults and constants
  tests/golden/ref_sobol.json             digests of sobol_tables.h's tables and of prepare_sobol's output
  tests/golden/vks/ref_reader_dumps.json  libvkr_ref.so's dumps of the .vks files the tests write (with a digest of their bytes),
                                          and which of tests/test_vks.py's broken files it accepts

Run in the build container only, from the repository root:

    make -C oracle ref && python tests/golden/gen_ref_fixtures.py
"""
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_abi  # noqa: E402
import test_pointsets as P  # noqa: E402
import test_vks as V  # noqa: E402
from realtimepathtracingresearchframework_amd import scenes, vks  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def write_json(path, doc):
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(path, ROOT))


def abi_report():
    L = C.CDLL(test_abi.ABI_REF)
    L.ref_abi_json.restype = C.c_char_p
    return json.loads(L.ref_abi_json())


def sobol_digests():
    ref_m, ref_inv = P.parse_sobol_header(open(P.REF_TABLE).read())
    return {"sobol_tables_h": {"matrix": P.digest(ref_m), "inversion": P.digest(ref_inv)}, "prepare_sobol": P.prepare_sobol_outputs()}


def vks_dumps(tmp):
    out = {}

    def add(key, path):
        d = V.live_dump(path, os.path.join(tmp, "dump.json"))
        assert d is not None, key
        out[key] = {"digest": V.tree_digest(path), "dump": d}

    for name in ("cornell32", "textured_test", "two_level_test", "alpha_test"):
        for version in (3, 4):
            sub = os.path.join(tmp, "%s_v%d" % (name, version))
            os.makedirs(sub)
            path = os.path.join(sub, name + ".vks")
            vks.write_vks(path, getattr(scenes, name)(), version=version)
            add("%s_v%d" % (name, version), path)
    for key, fname, write in (("lod_groups", "lod.vks", V.write_lod_file), ("wide_ids", "wide.vks", V.write_wide_ids_file),
                              ("mip_mapped", "m.vks", lambda p: vks.write_vks(p, V.mip_mapped_scene()))):
        sub = os.path.join(tmp, key)
        os.makedirs(sub)
        write(os.path.join(sub, fname))
        add(key, os.path.join(sub, fname))
    sub = os.path.join(tmp, "reject")
    os.makedirs(sub)
    import shutil
    shutil.copytree(os.path.join(GOLD, "vks", "alpha_v4_textures"), os.path.join(sub, "t_textures"))
    accepts = {}
    for tag, data in V.reject_cases().items():
        p = os.path.join(sub, "t.vks")
        open(p, "wb").write(data)
        accepts[tag] = V.live_dump(p, os.path.join(sub, "d.json")) is not None
    out["reference_accepts"] = accepts
    return out


if __name__ == "__main__":
    for need in (test_abi.ABI_REF, P.REF_TABLE, P.REF_TOOL, V.REF_LIB):
        if not os.path.exists(need):
            sys.exit("missing %s: build oracle/_ref from the reference checkout first (make -C oracle ref)" % need)
    write_json(test_abi.ABI_REF_JSON, abi_report())
    write_json(P.REF_SOBOL_JSON, sobol_digests())
    with tempfile.TemporaryDirectory() as tmp:
        write_json(V.REF_DUMPS, vks_dumps(tmp))
