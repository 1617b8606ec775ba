"""Checks shared by the scene-file tests: a .vks file against a dump of the reference's own reader (ext/libvkr/src/vkr.c compiled unmodified,
oracle/_ref/libvkr_ref.so), and two scenes' geometry streams against each other."""
import ctypes as C
import os

import numpy as np

from common import float_bits
from realtimepathtracingresearchframework_amd import vks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libvkr_ref.so")


def ref_reader():
    lib = C.CDLL(REF_LIB)
    lib.ref_vkr_dump.argtypes = [C.c_char_p, C.c_char_p]
    return lib


def compare_with_dump(path, ref):
    v = vks.read_vks_header(path)
    for key in ("version", "flags", "headerSize", "dataOffset", "numMaterials", "numTriangles", "numMeshes", "numInstances", "numLodGroups",
                "numFrames", "numStaticTransforms", "numAnimatedTransforms"):
        assert v[key] == ref[key], key
    if v["version"] >= 4:
        assert v["animationOffset"] == ref["animationOffset"]
    assert len(v["meshes"]) == len(ref["meshes"])
    for m, r in zip(v["meshes"], ref["meshes"]):
        assert float_bits(m["vertexScale"]).tolist() == r["vertexScale"] and float_bits(m["vertexOffset"]).tolist() == r["vertexOffset"]
        for key in ("name", "flags", "numSegments", "materialIdBufferBase", "numMaterialsInRange", "numTriangles", "lodGroup", "vertexBufferOffset",
                    "normalUvBufferOffset", "materialIdBufferOffset", "materialIdSize", "indexBufferOffset", "segmentNumTriangles",
                    "segmentMaterialBaseOffsets"):
            assert m[key] == r[key], key
    assert [(i["name"], i["meshId"], i["transformIndex"], i["flags"]) for i in v["instances"]] == [
        (i["name"], i["meshId"], i["transformIndex"], i["flags"]) for i in ref["instances"]]
    assert [(g["numLevelsOfDetail"], g["meshIds"]) for g in v["lodGroups"]] == [(g["numLevelsOfDetail"], g["meshIds"]) for g in ref["lodGroups"]]
    assert v["materialNames"] == [m["name"] for m in ref["materials"]]
    tdir = vks.texture_dir(path)
    for name, r in zip(v["materialNames"], ref["materials"]):
        m = vks._load_material_files(tdir, name)
        for key in ("emissionIntensity", "specularTransmission", "iorEta", "iorK", "translucency"):
            assert int(float_bits(m[key]).reshape(-1)[0]) == r[key], (name, key)
        assert float_bits(m["emitterBaseColor"]).tolist() == r["emitterBaseColor"]
        for mine, theirs in (("texBaseColor", "texBaseColor"), ("texNormal", "texNormal"), ("texSpecular", "texSpecular")):
            assert (m[mine] is None) == (r[theirs] is None), (name, mine)
            if m[mine] is not None:
                assert m[mine][0].shape[:2] == (r[theirs]["height"], r[theirs]["width"]) and m[mine][1] == r[theirs]["format"]
                assert 1 + len(m[mine][2]) == r[theirs]["numMipLevels"] and r[theirs]["dataOffset"] == 32 + 24 * r[theirs]["numMipLevels"], (name, mine)
    # the transform table as the reference dequantises it
    assert len(ref["transforms"]) == v["numStaticTransforms"]
    for k, r in enumerate(ref["transforms"]):
        mine = vks.dequantize_transform(v["transforms"][24 * k:24 * k + 24])
        assert float_bits(mine).reshape(-1).tolist() == r, "transform %d" % k
    return v


def same_streams(a, b):
    assert len(a.pmeshes) == len(b.pmeshes)
    for pa, pb in zip(a.pmeshes, b.pmeshes):
        ma, mb = a.meshes[pa.mesh], b.meshes[pb.mesh]
        assert ma.num_geometries == mb.num_geometries
        assert np.array_equal(pa.material_offsets, pb.material_offsets)
        assert (pa.tri_material_ids is None) == (pb.tri_material_ids is None)
        if pa.tri_material_ids is not None:
            assert np.array_equal(pa.tri_material_ids, pb.tri_material_ids)
        for j in range(ma.num_geometries):
            ga, gb = a.geometries[ma.first_geometry + j], b.geometries[mb.first_geometry + j]
            assert np.array_equal(ga.qpos, gb.qpos) and np.array_equal(float_bits(ga.scaling), float_bits(gb.scaling)) and np.array_equal(float_bits(ga.offset), float_bits(gb.offset))
            if ga.qnrm_uv is not None and ga.has_normals and ga.has_uvs:
                assert np.array_equal(ga.qnrm_uv, gb.qnrm_uv)
