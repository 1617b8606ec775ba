"""`.vks` scenes, `.vkt` textures and the material parameter `.txt` files of the reference's asset format
(SURVEY 8f rank 2): a reader that turns them into the `Scene` the backend consumes the way
`Scene::load_vkrs` does (librender/scene.cpp:544-977), and a writer so that the procedural scenes of
`scenes.py` can be handed to a real build of the reference (Vulkan-vs-HIP image comparison elsewhere).

File layout restated from the reference's reader, ext/libvkr/src/vkr.c:771-1145 (scene), :216-306 (texture),
:412-452 (parameter files); transform quantisation :1262-1411. Nothing of libvkr is linked here; tests compare this
module with libvkr itself compiled from the reference checkout (oracle/_ref/libvkr_ref.so, tests/test_vks.py) and
with fixtures generated from it (tests/golden/vks_*).

Block-compressed textures (BC1 / BC1A / BC3 / BC5, the formats `.vkt` carries) are decoded to RGBA8 level 0 on the
host: the backend samples RGBA8 (include/rptr_hip.h RptrTextureDesc). The decoders follow the published block
layouts (endpoints expanded by bit replication, palette entries rounded to nearest 8-bit); GPU decoders may differ
from that in the last bit -- "parity unpinned", like the filtering itself.
"""
import os
import struct

import numpy as np

from . import abi
from .scenes import Geometry, Instance, Mesh, ParameterizedMesh, Scene, SceneConfig, Texture, SKY_CONFIGS

f32 = np.float32

VKR_MAGIC = 0xABCABC            # vkr.c:40
VKT_MAGIC = 0xBC1BC1            # vkr.c:46
QUANTIZED_TRANSFORM_SIZE = 24   # vkr.h:15
MESH_FLAGS_INDICES = 0x1        # vkr.h:184

# VkFormat values a .vkt may carry (vkr.h:52-69) and VK_FORMAT_R8G8B8A8_SRGB (librender/scene.cpp:857)
FMT_BC1_RGB_UNORM, FMT_BC1_RGB_SRGB, FMT_BC1_RGBA_UNORM, FMT_BC1_RGBA_SRGB = 131, 132, 133, 134
FMT_BC3_UNORM, FMT_BC3_SRGB, FMT_BC5_UNORM, FMT_RGBA8_UNORM, FMT_RGBA8_SRGB = 137, 138, 141, 37, 43


class VksError(Exception):
    """≙ the reference's throw_error on a VkrResult != VKR_SUCCESS (scene.cpp:548-557)"""


# ------------------------------------------------------------------ transforms (vkr.c:1262-1411)
def _matrix_to_quaternion(m):
    """vkr.c:1267-1304, float32 arithmetic in the reference's order; m[3][3]"""
    q = np.zeros(4, f32)
    if m[0][0] + m[1][1] + m[2][2] > f32(0.1):
        q[0] = m[2][1] - m[1][2]
        q[1] = m[0][2] - m[2][0]
        q[2] = m[1][0] - m[0][1]
        q[3] = f32(1.0) + m[0][0] + m[1][1] + m[2][2]
    elif m[0][0] > m[1][1] and m[0][0] > m[2][2]:
        q[0] = f32(1.0) + m[0][0] - m[1][1] - m[2][2]
        q[1] = m[1][0] + m[0][1]
        q[2] = m[0][2] + m[2][0]
        q[3] = m[2][1] - m[1][2]
    elif m[1][1] > m[0][0] and m[1][1] > m[2][2]:
        q[0] = m[1][0] + m[0][1]
        q[1] = f32(1.0) + m[1][1] - m[0][0] - m[2][2]
        q[2] = m[2][1] + m[1][2]
        q[3] = m[0][2] - m[2][0]
    else:
        q[0] = m[0][2] + m[2][0]
        q[1] = m[2][1] + m[1][2]
        q[2] = f32(1.0) + m[2][2] - m[0][0] - m[1][1]
        q[3] = m[1][0] - m[0][1]
    length_sq = f32(0.0)
    for i in range(4):
        length_sq = f32(length_sq + q[i] * q[i])
    inv = f32(1.0) / np.sqrt(length_sq, dtype=f32)
    return (q * inv).astype(f32)


def quantize_transform(matrix):
    """vkr_quantize_transform (vkr.c:1346-1379): float matrix[4][3] (three basis vectors, then the translation) ->
    24 bytes = translation (3 floats), signed uniform scale (float), quaternion (4 x u16)."""
    m = np.asarray(matrix, dtype=f32).reshape(4, 3)
    scaling = f32(0.0)
    for i in range(3):
        scaling = f32(scaling + m[0][i] * m[0][i])
    scaling = np.sqrt(scaling, dtype=f32)
    a = m[:3]
    det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
           + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    if det < 0:
        scaling = f32(-scaling)
    normed = (a * (f32(1.0) / scaling)).astype(f32)
    q = _matrix_to_quaternion(normed)
    q[3] = -q[3]
    qq = np.floor((q * f32(0.5) + f32(0.5)).astype(f32) * f32(0xFFFF) - f32(0.5)).astype(f32)
    qq = (qq.astype(np.int64) & 0xFFFF).astype(np.uint16)   # (uint16_t) of a float in range
    return m[3].tobytes() + np.array([scaling], f32).tobytes() + qq.tobytes()


def dequantize_transform(raw):
    """vkr_dequantize_transform (vkr.c:1382-1411) -> float32 matrix[4][3]"""
    t = np.frombuffer(raw, dtype=f32, count=3, offset=0)
    scaling = np.frombuffer(raw, dtype=f32, count=1, offset=12)[0]
    qq = np.frombuffer(raw, dtype=np.uint16, count=4, offset=16)
    q = (qq.astype(f32) * f32(f32(2.0) / f32(0xFFFF)) - f32(1.0)).astype(f32)
    q[3] = -q[3]
    xx, xy, xz, xw = q[0] * q[0], q[0] * q[1], q[0] * q[2], q[0] * q[3]
    yy, yz, yw = q[1] * q[1], q[1] * q[2], q[1] * q[3]
    zz, zw = q[2] * q[2], q[2] * q[3]
    one, two = f32(1.0), f32(2.0)
    m = np.zeros((4, 3), f32)
    m[0] = [one - two * (yy + zz), two * (xy - zw), two * (xz + yw)]
    m[1] = [two * (xy + zw), one - two * (xx + zz), two * (yz - xw)]
    m[2] = [two * (xz - yw), two * (yz + xw), one - two * (xx + yy)]
    m[:3] = (m[:3] * scaling).astype(f32)
    m[3] = t
    return m


# vks_flip of AnimationData::dequantize (librender/scene.cpp:36-40), as a 3x3 acting on column vectors
VKS_FLIP = np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0]], dtype=f32)


def instance_transform(raw):
    """AnimationData::dequantize (scene.cpp:22-41): `vks_flip * mat4(tx)` as the row-major 3x4 object-to-world matrix of
    an instance. tx's columns are the rows of the dequantised float[4][3]."""
    m = dequantize_transform(raw)
    cols = np.stack([m[0], m[1], m[2], m[3]], axis=1)       # 3x4: column c = m[c]
    return (VKS_FLIP @ cols).astype(f32)


def storable_transform(object_to_world):
    """the float[4][3] whose `instance_transform` is (up to quantisation) `object_to_world`; raises for transforms the
    24-byte form cannot hold (anything but rotation x uniform scale, possibly mirrored)"""
    t = np.asarray(object_to_world, dtype=f32).reshape(3, 4)
    cols = (VKS_FLIP @ t).astype(f32)                       # vks_flip is its own inverse
    m = np.stack([cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]], axis=0)
    a = m[:3].astype(np.float64)
    s2 = (a[0] ** 2).sum()
    if s2 <= 0 or not np.allclose(a @ a.T, s2 * np.eye(3), rtol=0, atol=1e-4 * s2):
        raise VksError("transform is not a rotation with uniform scale: not representable in a .vks instance")
    return m


# ------------------------------------------------------------------ block compression
def _expand565(c):
    c = np.asarray(c, dtype=np.uint32)
    r, g, b = (c >> 11) & 31, (c >> 5) & 63, c & 31
    return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)], axis=-1).astype(np.float64)


def _bc1_palette(c0, c1, force4):
    """(n,) u16 endpoints -> (n,4,4) RGBA in [0,255] doubles. Three-colour mode (c0 <= c1): entry 3 is transparent black."""
    e0, e1 = _expand565(c0), _expand565(c1)
    four = np.ones_like(c0, dtype=bool) if force4 else (c0 > c1)
    pal = np.zeros(c0.shape + (4, 4), np.float64)
    pal[..., 0, :3], pal[..., 1, :3] = e0, e1
    pal[..., 2, :3] = np.where(four[..., None], (2 * e0 + e1) / 3.0, (e0 + e1) / 2.0)
    pal[..., 3, :3] = np.where(four[..., None], (e0 + 2 * e1) / 3.0, 0.0)
    pal[..., :, 3] = 255.0
    pal[..., 3, 3] = np.where(four, 255.0, 0.0)
    return pal


def _bc4_values(blocks):
    """(n,8) uint8 BC4 blocks -> (n,16) values in [0,255] doubles"""
    a0, a1 = blocks[:, 0].astype(np.float64), blocks[:, 1].astype(np.float64)
    bits = np.zeros(len(blocks), np.uint64)
    for k in range(6):
        bits |= blocks[:, 2 + k].astype(np.uint64) << np.uint64(8 * k)
    idx = np.stack([((bits >> np.uint64(3 * t)) & np.uint64(7)).astype(np.int64) for t in range(16)], axis=1)
    pal = np.zeros((len(blocks), 8), np.float64)
    pal[:, 0], pal[:, 1] = a0, a1
    eight = a0 > a1
    for i in range(1, 7):
        pal[:, 1 + i] = np.where(eight, ((7 - i) * a0 + i * a1) / 7.0, ((5 - i) * a0 + i * a1) / 5.0 if i < 5 else 0.0)
    pal[:, 6] = np.where(eight, pal[:, 6], 0.0)
    pal[:, 7] = np.where(eight, pal[:, 7], 255.0)
    return np.take_along_axis(pal, idx, axis=1)


def _blocks_to_image(texels, bw, bh, width, height):
    """(bh*bw, 16, 4) per-block texels (row-major inside the block) -> (height, width, 4) uint8"""
    img = texels.reshape(bh, bw, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)
    return np.clip(np.floor(img[:height, :width] + 0.5), 0, 255).astype(np.uint8)


def decode_texture(data, width, height, fmt):
    """level 0 of a .vkt payload -> (height, width, 4) uint8 RGBA"""
    if fmt in (FMT_RGBA8_UNORM, FMT_RGBA8_SRGB):
        return np.frombuffer(data, dtype=np.uint8, count=width * height * 4).reshape(height, width, 4).copy()
    bw, bh = (width + 3) // 4, (height + 3) // 4
    n = bw * bh
    if fmt in (FMT_BC1_RGB_UNORM, FMT_BC1_RGB_SRGB, FMT_BC1_RGBA_UNORM, FMT_BC1_RGBA_SRGB):
        b = np.frombuffer(data, dtype=np.uint8, count=n * 8).reshape(n, 8)
        colour, alpha_vals = b, None
    elif fmt in (FMT_BC3_UNORM, FMT_BC3_SRGB):
        b = np.frombuffer(data, dtype=np.uint8, count=n * 16).reshape(n, 16)
        colour, alpha_vals = b[:, 8:], _bc4_values(b[:, :8])
    elif fmt == FMT_BC5_UNORM:
        b = np.frombuffer(data, dtype=np.uint8, count=n * 16).reshape(n, 16)
        tex = np.zeros((n, 16, 4), np.float64)
        tex[..., 0], tex[..., 1], tex[..., 3] = _bc4_values(b[:, :8]), _bc4_values(b[:, 8:]), 255.0
        return _blocks_to_image(tex, bw, bh, width, height)
    else:
        raise VksError("unsupported texture format %d" % fmt)
    c0 = colour[:, 0].astype(np.uint32) | (colour[:, 1].astype(np.uint32) << 8)
    c1 = colour[:, 2].astype(np.uint32) | (colour[:, 3].astype(np.uint32) << 8)
    pal = _bc1_palette(c0, c1, force4=alpha_vals is not None)
    bits = colour[:, 4].astype(np.uint32) | (colour[:, 5].astype(np.uint32) << 8) | (colour[:, 6].astype(np.uint32) << 16) | (
        colour[:, 7].astype(np.uint32) << 24)
    idx = np.stack([((bits >> (2 * t)) & 3).astype(np.int64) for t in range(16)], axis=1)
    tex = np.take_along_axis(pal, idx[:, :, None].repeat(4, axis=2), axis=1)
    if alpha_vals is not None:
        tex[..., 3] = alpha_vals
    elif fmt in (FMT_BC1_RGB_UNORM, FMT_BC1_RGB_SRGB):
        tex[..., 3] = 255.0      # VK_FORMAT_BC1_RGB_*: the transparent entry decodes as opaque black
    return _blocks_to_image(tex, bw, bh, width, height)


def _image_to_blocks(img):
    h, w = img.shape[:2]
    bh, bw = (h + 3) // 4, (w + 3) // 4
    pad = np.zeros((bh * 4, bw * 4, img.shape[2]), img.dtype)
    pad[:h, :w] = img
    pad[h:, :w] = img[h - 1:h, :]                           # replicate the border into the padding
    pad[:, w:] = pad[:, w - 1:w]
    return pad.reshape(bh, 4, bw, 4, img.shape[2]).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, img.shape[2])


def encode_bc1(rgb):
    """(h,w,3) uint8 -> BC1 blocks (opaque, four-colour mode where the block has two distinct endpoints): endpoints = the
    corners of the block's colour bounding box, indices by nearest palette entry"""
    blk = _image_to_blocks(np.asarray(rgb, dtype=np.uint8)[..., :3]).astype(np.int64)
    lo, hi = blk.min(axis=1), blk.max(axis=1)

    def to565(c):
        return ((c[:, 0] * 31 + 127) // 255 << 11) | ((c[:, 1] * 63 + 127) // 255 << 5) | ((c[:, 2] * 31 + 127) // 255)
    c0, c1 = to565(hi).astype(np.uint32), to565(lo).astype(np.uint32)
    swap = c0 < c1
    c0, c1 = np.where(swap, c1, c0), np.where(swap, c0, c1)
    pal = _bc1_palette(c0, c1, force4=False)[..., :3]       # c0 == c1: three-colour mode, entries 0..2 equal, 3 is black
    d = ((blk[:, :, None, :].astype(np.float64) - pal[:, None, :, :]) ** 2).sum(axis=3)
    d[:, :, 3] = np.where((c0 > c1)[:, None], d[:, :, 3], np.inf)
    idx = d.argmin(axis=2).astype(np.uint32)
    bits = np.zeros(len(blk), np.uint32)
    for t in range(16):
        bits |= idx[:, t] << np.uint32(2 * t)
    out = np.zeros((len(blk), 8), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    for k in range(4):
        out[:, 4 + k] = (bits >> np.uint32(8 * k)) & 255
    return out.tobytes()


def _encode_bc4(vals):
    """(n,16) uint8 -> (n,8) uint8 blocks, eight-value mode (a0 > a1) or a flat block"""
    v = vals.astype(np.int64)
    a0, a1 = v.max(axis=1), v.min(axis=1)
    pal = np.zeros((len(v), 8), np.float64)
    pal[:, 0], pal[:, 1] = a0, a1
    for i in range(1, 7):
        pal[:, 1 + i] = ((7 - i) * a0 + i * a1) / 7.0
    idx = np.abs(v[:, :, None] - pal[:, None, :]).argmin(axis=2).astype(np.uint64)
    idx[a0 == a1] = 0                                        # flat block: entry 0 (six-value mode, a0 itself)
    bits = np.zeros(len(v), np.uint64)
    for t in range(16):
        bits |= idx[:, t] << np.uint64(3 * t)
    out = np.zeros((len(v), 8), np.uint8)
    out[:, 0], out[:, 1] = a0, a1
    for k in range(6):
        out[:, 2 + k] = (bits >> np.uint64(8 * k)) & np.uint64(255)
    return out


def encode_bc5(rg):
    blk = _image_to_blocks(np.asarray(rg, dtype=np.uint8)[..., :2])
    return np.concatenate([_encode_bc4(blk[..., 0]), _encode_bc4(blk[..., 1])], axis=1).tobytes()


def encode_bc3(rgba):
    rgba = np.asarray(rgba, dtype=np.uint8)
    colour = np.frombuffer(encode_bc1(rgba[..., :3]), np.uint8).reshape(-1, 8)
    alpha = _encode_bc4(_image_to_blocks(rgba[..., 3:4])[..., 0])
    # BC3 colour blocks are always decoded in four-colour mode; flat blocks (c0 == c1) only use entry 0 either way
    return np.concatenate([alpha, colour], axis=1).tobytes()


# ------------------------------------------------------------------ .vkt (vkr.c:216-306, header structs :1511-1531)
def write_vkt(path, rgba, fmt, mips=None):
    """level 0 and (`mips`) the levels behind it, back to back (vkr.c:1546-1558, 1997-2014). `fmt` picks the encoding: RGBA8 (37 / 43) raw,
    BC1 (131 / 132), BC3 (137 / 138), BC5 (141)."""
    def encode(px):
        px = np.asarray(px, dtype=np.uint8)
        if fmt in (FMT_RGBA8_UNORM, FMT_RGBA8_SRGB):
            return np.ascontiguousarray(px).tobytes()
        if fmt in (FMT_BC1_RGB_UNORM, FMT_BC1_RGB_SRGB):
            return encode_bc1(px)
        if fmt in (FMT_BC3_UNORM, FMT_BC3_SRGB):
            return encode_bc3(px)
        if fmt == FMT_BC5_UNORM:
            return encode_bc5(px)
        raise VksError("write_vkt: unsupported format %d" % fmt)
    levels = [np.asarray(rgba, dtype=np.uint8)] + [np.asarray(m, dtype=np.uint8) for m in (mips or [])]
    data = [encode(px) for px in levels]
    h, w = levels[0].shape[:2]
    with open(path, "wb") as f:
        f.write(struct.pack("<6iQ", VKT_MAGIC, 1, len(levels), w, h, fmt, sum(len(d) for d in data)))
        at = 32 + 24 * len(levels)
        for px, d in zip(levels, data):
            f.write(struct.pack("<iiQq", px.shape[1], px.shape[0], len(d), at))
            at += len(d)
        for d in data:
            f.write(d)


def read_vkt(path):
    """-> (rgba8 level 0, VkFormat, [rgba8 of the levels behind it]) or None when the file does not exist (textures are optional,
    vkr.c:475-489). The levels lie back to back behind the mip headers (the reference maps dataSize bytes from dataOffset and uploads
    every level: scene.cpp:866, vulkan/resource_utils.cpp:86-100)."""
    if not os.path.isfile(path):
        return None
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 32:
        raise VksError("%s is not a .vkt file." % path)
    magic, version, nmips, w, h, fmt, size = struct.unpack_from("<6iQ", raw, 0)
    if magic != VKT_MAGIC:
        raise VksError("%s is not a .vkt file." % path)
    if version != 1:
        raise VksError("Unsupported file version %d in %s" % (version, path))
    if nmips < 1 or len(raw) < 32 + 24 * nmips:
        raise VksError("Failed to read mip level header.")
    at = 32 + 24 * nmips                                      # t->dataOffset = ftell(f) after the mip headers
    levels = []
    for l in range(nmips):
        mw, mh, msize, _moff = struct.unpack_from("<iiQq", raw, 32 + 24 * l)
        if l and (mw, mh) != (max(1, levels[-1].shape[1] // 2), max(1, levels[-1].shape[0] // 2)):
            raise VksError("mip level %d of %s is %d x %d" % (l, path, mw, mh))
        if at + msize > len(raw):
            raise VksError("texture payload too short")
        levels.append(decode_texture(raw[at:at + msize], mw, mh, fmt))
        at += msize
    return levels[0], fmt, levels[1:]


# ------------------------------------------------------------------ material parameter files (vkr.c:412-452)
def _read_params(path, max_values):
    """one float per line; None when the file does not exist"""
    if not os.path.isfile(path):
        return None
    vals = []
    with open(path, "r") as f:
        for line in f.read().split("\n"):
            if len(vals) == max_values or line.strip() == "":
                break
            try:
                vals.append(float(np.float32(line.rstrip("\r"))))
            except ValueError:
                raise VksError("Invalid number format in vkr_parse_material_param_file")
    return vals


def texture_dir(scene_file):   # buildTextureDir, vkr.c:80-110
    dot = scene_file.rfind(".")
    return (scene_file[:dot] if dot >= 0 else scene_file) + "_textures/"


# ------------------------------------------------------------------ .vks reader (vkr.c:771-1145)
class _Cursor:
    def __init__(self, raw, name):
        self.raw, self.at, self.name = raw, 0, name

    def take(self, fmt):
        n = struct.calcsize(fmt)
        if self.at + n > len(self.raw):
            raise VksError("Failed to read header structure from %s." % self.name)
        v = struct.unpack_from(fmt, self.raw, self.at)
        self.at += n
        return v if len(v) > 1 else v[0]

    def string(self):            # vkr_load_string: u64 length, then length+1 bytes
        n = self.take("<Q")
        if self.at + n + 1 > len(self.raw):
            raise VksError("Failed to read string from %s." % self.name)
        s = self.raw[self.at:self.at + n].decode("utf-8", "replace")
        self.at += n + 1
        return s


def read_vks_header(path):
    """The fields `vkr_open_scene` fills (VkrScene / VkrMesh / VkrInstance / VkrLodGroup, vkr.h:186-303) as plain dicts,
    for file versions 3 and 4 (what the reference's exporter writes; versions 1-2 are legacy single-mesh files)."""
    with open(path, "rb") as f:
        raw = f.read()
    c = _Cursor(raw, path)
    if len(raw) < 8 or c.take("<i") != VKR_MAGIC:
        raise VksError("%s is not a .vks file." % path)
    version = c.take("<i")
    if version < 3 or version > 4:
        raise VksError("Unsupported version %d in %s." % (version, path))
    v = {"version": version}
    flags, v["headerSize"], v["dataOffset"] = c.take("<3Q")
    v["flags"] = flags & 0xFFFFFFFF
    if not (v["headerSize"] > 0 and v["dataOffset"] >= v["headerSize"]):
        raise VksError("Failed to read header size & data offset from %s." % path)
    v["numMeshes"], v["numInstances"], v["numMaterials"], v["numTriangles"], groups = c.take("<5Q")
    v["numLodGroups"], lod_offset = 1, 0
    v.update(numBoneIndexTuples=0, boneIndexTuplesOffset=0, animationStart=0.0, animationStep=0.0, numAnimatedTransforms=0, animationOffset=0)
    if version >= 4:
        (v["numLodGroups"], lod_offset, v["numBoneIndexTuples"], v["boneIndexTuplesOffset"], v["animationStart"], v["animationStep"],
         v["numFrames"], v["numStaticTransforms"], v["numAnimatedTransforms"], v["animationOffset"]) = c.take("<QqQqffQQQq")
    else:
        v["numFrames"], v["numStaticTransforms"] = 1, v["numInstances"]
    if v["numMeshes"] == 0 or v["numInstances"] == 0 or groups == 0 or v["numLodGroups"] == 0:
        raise VksError("Failed to read valid object counts from %s." % path)
    if v["headerSize"] != c.at:
        raise VksError("Mismatching header size in %s." % path)
    meshes = []
    for i in range(v["numMeshes"]):
        m = {}
        m["vertexScale"] = list(c.take("<3f"))
        m["vertexOffset"] = list(c.take("<3f"))
        mflags, header_end, m["vertexBufferOffset"] = c.take("<3Q")
        m["flags"] = mflags & 0xFFFFFFFF
        m["numSegments"], m["numTriangles"], m["materialIdBufferBase"], m["numMaterialsInRange"] = c.take("<QQiI")
        m["lodGroup"] = 0
        reserved = 5
        if version >= 4:
            m["lodGroup"] = c.take("<q")
            reserved -= 1
        c.take("<%dQ" % reserved)
        if m["lodGroup"] >= v["numLodGroups"]:
            raise VksError("Invalid LoD group specified for mesh %d from %s." % (i, path))
        ns = m["numSegments"]
        m["segmentNumTriangles"] = [c.take("<Q") for _ in range(ns)]
        m["segmentMaterialBaseOffsets"] = [c.take("<i") for _ in range(ns)]
        m["name"] = c.string()
        if header_end != c.at:
            raise VksError("Mismatching header offset for mesh %d from %s." % (i, path))
        meshes.append(m)
    instances, legacy_transforms = [], []
    for g in range(groups):
        iflags, mesh_id = c.take("<Ii")
        header_end, data_offset, count = c.take("<3Q")
        name = c.string()
        if data_offset != c.at:
            raise VksError("Mismatching data offset for instance group %d from %s." % (g, path))
        for _ in range(count):
            if version >= 4:
                ti = c.take("<I")
            else:      # version 3 stores the float[4][3] itself; the reader quantises it into the table (vkr.c:1027-1035)
                legacy_transforms.append(quantize_transform(np.array(c.take("<12f"), f32).reshape(4, 3)))
                ti = len(legacy_transforms) - 1
            instances.append({"name": name, "meshId": mesh_id, "flags": iflags, "transformIndex": ti})
        if header_end != c.at:
            raise VksError("Mismatching header offset for instance group %d from %s." % (g, path))
    if len(instances) != v["numInstances"]:
        raise VksError("Failed to read valid object counts from %s." % path)
    lods = [{"numLevelsOfDetail": 0, "meshIds": [], "detailReduction": []}]
    if version >= 4:
        if lod_offset != c.at:
            raise VksError("Read invalid LoD group offset from %s." % path)
        lods = []
        for _ in range(v["numLodGroups"]):
            n = c.take("<Q")
            ids = [c.take("<q") for _ in range(n)]
            red = [c.take("<f") for _ in range(n)]
            lods.append({"numLevelsOfDetail": n, "meshIds": ids, "detailReduction": red})
    if v["dataOffset"] != c.at:
        raise VksError("Mismatching body data offset %s." % path)
    v["materialNames"] = [c.string() for _ in range(v["numMaterials"])]
    offset = c.at
    for i, m in enumerate(meshes):      # vkr.c:1110-1138
        if m["vertexBufferOffset"] != offset:
            raise VksError("Mismatching data offset for mesh %d from %s." % (i, path))
        n = m["numTriangles"]
        offset += 24 * n
        m["normalUvBufferOffset"] = offset
        offset += 24 * n
        m["materialIdBufferOffset"] = offset
        m["materialIdSize"] = 1 if (m["numMaterialsInRange"] <= 0x100 or m["numSegments"] > 1) else 2
        offset += m["materialIdSize"] * n
        m["indexBufferOffset"] = 0
        if m["flags"] & MESH_FLAGS_INDICES:
            m["indexBufferOffset"] = offset
            offset += 12 * n
    v["meshes"], v["instances"], v["lodGroups"] = meshes, instances, lods
    n_tf = v["numStaticTransforms"] + v["numFrames"] * v["numAnimatedTransforms"]
    if version >= 4:
        a = v["animationOffset"]
        if a <= 0 or a + n_tf * QUANTIZED_TRANSFORM_SIZE > len(raw):
            raise VksError("Failed to read the transform table from %s." % path)
        v["transforms"] = raw[a:a + n_tf * QUANTIZED_TRANSFORM_SIZE]
    else:
        v["transforms"] = b"".join(legacy_transforms)
    v["_raw"] = raw
    return v


def transform_offset(index, num_static, num_animated, frame):   # vkr_get_transform_offset, vkr.c:197-208
    if index < num_static:
        return index
    return num_static + (index - num_static) + frame * num_animated


def _instanced(v, instance_pruning_probability=0.0):
    """The instances of an opened file that `read_vks` turns into scene instances, in its order: base levels of LoD groups only
    (scene.cpp:722-736), minus the pruned ones (:734-749). Yields (index in the file, VkrInstance dict, LoD group)."""
    for idx, vi in enumerate(v["instances"]):
        lod = v["lodGroups"][v["meshes"][vi["meshId"]]["lodGroup"]]
        if lod["numLevelsOfDetail"] != 0 and lod["meshIds"][0] != vi["meshId"]:
            continue
        if instance_pruning_probability and halton2(idx) < instance_pruning_probability:
            continue
        yield idx, vi, lod


def frame_transforms(v, frame, instance_pruning_probability=0.0):
    """The (n, 12) float32 object-to-world transforms (row-major 3x4, what `update_instances` takes) of frame `frame` of an OPENED
    scene -- `v` is what `read_vks_header` returned; nothing is loaded again -- for the instances `read_vks` made of it, in its order:
    `AnimationData::dequantize(index, frame)` (librender/scene.cpp:22-41) per instance. Equal to the instance transforms of
    `read_vks(path, frame=frame)` bit for bit."""
    if not 0 <= frame < max(1, v["numFrames"]):
        raise VksError("frame %d of %d" % (frame, v["numFrames"]))
    out = []
    for _, vi, _ in _instanced(v, instance_pruning_probability):
        at = transform_offset(vi["transformIndex"], v["numStaticTransforms"], v["numAnimatedTransforms"], frame) * QUANTIZED_TRANSFORM_SIZE
        out.append(np.asarray(instance_transform(v["transforms"][at:at + QUANTIZED_TRANSFORM_SIZE]), f32).reshape(12))
    return np.stack(out) if out else np.zeros((0, 12), f32)


def animated_instances(v, instance_pruning_probability=0.0):
    """indices (into the instance list `read_vks` makes) of the instances whose transform changes with the frame: transformIndex >=
    numStaticTransforms"""
    return [k for k, (_, vi, _) in enumerate(_instanced(v, instance_pruning_probability)) if vi["transformIndex"] >= v["numStaticTransforms"]]


def _load_material_files(tex_dir, name):
    """vkr_load_material (vkr.c:509-620): parameter files and the three standard textures of one material"""
    m = {"name": name, "emissionIntensity": 0.0, "emitterBaseColor": [0.0, 0.0, 0.0], "specularTransmission": 0.0, "iorEta": 1.5,
         "iorK": 0.0, "translucency": 0.0, "extended_name": name}
    ex = tex_dir + name + "_Ex.txt"
    if os.path.isfile(ex):
        with open(ex, "r") as f:
            m["extended_name"] = f.read()
    em = _read_params(tex_dir + name + "_EmissionIntensity.txt", 4)
    if em is not None:
        if len(em) == 1:
            col = _read_params(tex_dir + name + "_BaseColor.txt", 3)
            if col is not None and len(col) not in (0, 3):
                raise VksError("Three color components expected for emission base color")
            em = em + (col if col else [0.0, 0.0, 0.0])
        elif len(em) not in (0, 4):
            raise VksError("One or four components expected for emission intensity + base color")
        if em:
            m["emissionIntensity"], m["emitterBaseColor"] = em[0], em[1:4]
    tr = _read_params(tex_dir + name + "_SpecularTransmission.txt", 4)
    if tr:
        for key, val in zip(("specularTransmission", "iorEta", "iorK", "translucency"), tr):
            m[key] = val
    m["texBaseColor"] = read_vkt(tex_dir + name + "_BaseColor.vkt")
    m["texNormal"] = read_vkt(tex_dir + name + "_Normal.vkt")
    m["texSpecular"] = read_vkt(tex_dir + name + "_Specular.vkt")
    return m


def halton2(index):
    """util/compute_util.h:19-33: the bit-reversed index written into a float's mantissa"""
    r = int("{:032b}".format(index & 0xFFFFFFFF)[::-1], 2)
    return float(np.array([0x3F800000 | (r >> 9)], np.uint32).view(f32)[0] - f32(1.0))


def read_vks(path, ignore_textures=False, load_specularity=False, frame=0, remove_first_lods=0, instance_pruning_probability=0.0,
             small_deformation=False, ignore_animation=False, dynamic_meshes=True) -> Scene:
    """`Scene::load_vkrs` (librender/scene.cpp:544-977) for one file with the per-file override parameters of `SceneLoaderParams`
    (librender/scene.h:33-45) that change what is rendered: one mesh and one
    parameterized mesh per .vks mesh (a geometry per segment, per-triangle material ids when a single segment spans
    several materials), base-LoD instances with `vks_flip * dequantised transform`, and per material the three standard
    textures (1x1 defaults when a file is missing) wired into the `BaseMaterial` as texture handles.
    `dynamic_meshes` = a reference build with ENABLE_DYNAMIC_MESHES: a mesh with a segment whose material's extended name carries
    `_SHADERMESH_<name>` or `_SHADERSUBMESH_<name>` is flagged Mesh::Dynamic (Mesh::SubtlyDynamic with `small_deformation`), unless
    `ignore_animation` (scene.cpp:658-706; the named vertex shader itself is the host application's: `update_vertices`).
    `instance_pruning_probability`: instance i of the file is dropped when halton2(i) < p (scene.cpp:734-749).
    (`merge_partition_instances` only regroups geometries of equal-transform instances into one mesh: no effect on the image, not done.)"""
    v = read_vks_header(path)
    raw = v["_raw"]
    s = Scene(name=os.path.splitext(os.path.basename(path))[0])
    tex_dir = texture_dir(path)
    mat_files = [_load_material_files(tex_dir, name) for name in v["materialNames"]]
    dynamic_flag = abi.MESH_SUBTLY_DYNAMIC if small_deformation else abi.MESH_DYNAMIC
    for i, vm in enumerate(v["meshes"]):
        first = len(s.geometries)
        base = 0
        scale, offset = np.array(vm["vertexScale"], f32), np.array(vm["vertexOffset"], f32)
        kept_offsets = []
        for j in range(vm["numSegments"]):
            n = vm["segmentNumTriangles"][j]
            if n == 0:                   # "Removed %d empty geometry segments" (scene.cpp:641-646)
                continue
            qpos = np.frombuffer(raw, dtype=np.uint64, count=3 * n, offset=vm["vertexBufferOffset"] + 24 * base).copy()
            qnu = np.frombuffer(raw, dtype=np.uint64, count=3 * n, offset=vm["normalUvBufferOffset"] + 24 * base).copy()
            s.geometries.append(Geometry(qpos=qpos, qnrm_uv=qnu, num_tris=n, has_normals=True, has_uvs=True, scaling=scale.copy(),
                                         offset=offset.copy()))
            kept_offsets.append(vm["segmentMaterialBaseOffsets"][j])
            base += n
        s.meshes.append(Mesh(first_geometry=first, num_geometries=len(s.geometries) - first))
        if vm["numSegments"] == 1 and vm["numMaterialsInRange"] > 1:        # scene.cpp:654-658
            if vm["materialIdSize"] == 2:    # the backend keeps 8 bits per triangle: static_cast<uint8_t>(id), render_vulkan.cpp:1114-1126
                ids = (np.frombuffer(raw, dtype=np.uint16, count=vm["numTriangles"], offset=vm["materialIdBufferOffset"]) & 0xFF).astype(np.uint8)
            else:
                ids = np.frombuffer(raw, dtype=np.uint8, count=vm["numTriangles"], offset=vm["materialIdBufferOffset"]).copy()
            s.pmeshes.append(ParameterizedMesh(mesh=i, material_offsets=np.array([vm["materialIdBufferBase"]], np.int32), tri_material_ids=ids))
        else:
            s.pmeshes.append(ParameterizedMesh(mesh=i, material_offsets=np.array(kept_offsets, np.int32)))
            if dynamic_meshes and not ignore_animation and s.meshes[-1].num_geometries > 0:
                for off in vm["segmentMaterialBaseOffsets"][:vm["numSegments"]]:
                    ext = mat_files[off]["extended_name"] if 0 <= off < len(mat_files) else ""
                    if "_SHADERMESH_" in ext or "_SHADERSUBMESH_" in ext:
                        s.meshes[-1].dynamic = int(s.meshes[-1].dynamic) | dynamic_flag
    for idx, vi, lod in _instanced(v, instance_pruning_probability):   # scene.cpp:722-745: only the base level of a LoD group is instanced
        pmesh = vi["meshId"]
        if remove_first_lods > 0 and lod["numLevelsOfDetail"] > 1:
            # SceneLoaderParams::PerFile::remove_first_LODs (scene.cpp:801-815): the first n levels are replaced by level n (or the
            # coarsest), and unlink_pruned_lod_meshes (:229-246) re-aligns the instances of the group with its new first level
            pmesh = int(lod["meshIds"][min(remove_first_lods, lod["numLevelsOfDetail"] - 1)])
        at = transform_offset(vi["transformIndex"], v["numStaticTransforms"], v["numAnimatedTransforms"], frame) * QUANTIZED_TRANSFORM_SIZE
        s.instances.append(Instance(transform=instance_transform(v["transforms"][at:at + QUANTIZED_TRANSFORM_SIZE]), pmesh=pmesh))
        if vi["transformIndex"] >= v["numStaticTransforms"] and not ignore_animation:
            # an animated transform: the instances of this mesh move (`frame_transforms` + RenderHip.update_instances play the frames)
            mesh = s.meshes[s.pmeshes[pmesh].mesh]
            mesh.dynamic = int(mesh.dynamic) | abi.MESH_INSTANCES_MOVE
    for i, name in enumerate(v["materialNames"]):   # scene.cpp:818-975
        vm = mat_files[i]
        mat = abi.make_material(flags=0)
        tid = 3 * i
        col = None if ignore_textures else vm["texBaseColor"]
        has_alpha = False
        if col is not None:
            has_alpha = col[1] in (FMT_BC1_RGBA_UNORM, FMT_BC1_RGBA_SRGB, FMT_BC3_UNORM, FMT_BC3_SRGB, FMT_RGBA8_UNORM, FMT_RGBA8_SRGB)
            s.textures.append(Texture(rgba=col[0], srgb=True, mips=col[2] or None))
        else:
            s.textures.append(Texture(rgba=np.full((1, 1, 4), 255, np.uint8), srgb=True))
        if not has_alpha:
            mat.flags |= abi.BASE_MATERIAL_NOALPHA
        abi.set_float_bits(mat.base_color, 0, 0x80000000 | tid)
        nrm = None if ignore_textures else vm["texNormal"]
        s.textures.append(Texture(rgba=nrm[0] if nrm is not None else np.array([[[127, 127, 127, 255]]], np.uint8), srgb=False,
                                  mips=(nrm[2] or None) if nrm is not None else None))
        mat.normal_map = tid + 1
        spec = None if ignore_textures else vm["texSpecular"]
        s.textures.append(Texture(rgba=spec[0] if spec is not None else np.array([[[255, 127, 0, 255]]], np.uint8), srgb=False,
                                  mips=(spec[2] or None) if spec is not None else None))
        mat.roughness = abi.textured_param(tid + 2, 1)
        mat.metallic = abi.textured_param(tid + 2, 2)
        if load_specularity:
            mat.specular = abi.textured_param(tid + 2, 0)
        if vm["emissionIntensity"] > 0:
            if any(c != 0.0 for c in vm["emitterBaseColor"]):
                mat.base_color[:] = vm["emitterBaseColor"]
            mat.emission_intensity = vm["emissionIntensity"]
        mat.specular_transmission = vm["specularTransmission"]
        if vm["specularTransmission"] and not any(k in vm["extended_name"] for k in ("twosided", "doublesided", "TwoSided", "DoubleSided")):
            mat.flags |= abi.BASE_MATERIAL_ONESIDED
        mat.ior = vm["iorEta"]
        s.materials.append(mat)
    s.config = SceneConfig(**SKY_CONFIGS["default"])
    s.sky_key = "default"
    s.camera = _default_camera(s)
    s.prepare_lights()
    return s


def _default_camera(s):
    from .scenes import dequantize_positions
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in s.instances:
        mesh = s.meshes[s.pmeshes[inst.pmesh].mesh]
        for g in s.geometries[mesh.first_geometry:mesh.first_geometry + mesh.num_geometries]:
            p = dequantize_positions(g.qpos[:: max(1, len(g.qpos) // 4096)], g.scaling, g.offset).astype(np.float64)
            w = p @ np.asarray(inst.transform, np.float64)[:, :3].T + np.asarray(inst.transform, np.float64)[:, 3]
            lo, hi = np.minimum(lo, w.min(axis=0)), np.maximum(hi, w.max(axis=0))
    if not np.isfinite(lo).all():
        lo, hi = np.zeros(3), np.ones(3)
    c, r = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    return dict(eye=tuple(float(x) for x in c + np.array([0.0, 0.35 * r, 1.6 * r])), center=tuple(float(x) for x in c), up=(0, 1, 0), fov=50.0)


# ------------------------------------------------------------------ .vks writer
def _string(sv):
    b = sv.encode("utf-8")
    return struct.pack("<Q", len(b)) + b + b"\0"


def _solid(rgba, size=4):
    return np.tile(np.array(rgba, np.uint8).reshape(1, 1, 4), (size, size, 1))


def _linear_to_srgb8(c):
    c = np.clip(np.asarray(c, np.float64), 0.0, 1.0)
    e = np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(c, 1.0 / 2.4) - 0.055)
    return np.clip(np.floor(e * 255.0 + 0.5), 0, 255).astype(np.uint8)


def _normal_uv_stream(g):
    """.vks meshes always carry the normal / uv stream: a geometry without normals gets its triangles' geometric normals
    (what the shader falls back to, hit.glsl:72-84, now oct-quantised), one without uvs gets uv = (0, 0)"""
    from .scenes import dequantize_positions, quantize_normals, quantize_uvs
    have = None if g.qnrm_uv is None else np.asarray(g.qnrm_uv, np.uint64)
    if have is not None and g.has_normals and g.has_uvs:
        return have
    if have is not None and g.has_normals:
        qn = (have & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    else:
        p = dequantize_positions(g.qpos, g.scaling, g.offset).reshape(-1, 3, 3).astype(np.float64)
        gn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        ln = np.linalg.norm(gn, axis=1, keepdims=True)
        gn = np.where(ln > 0, gn / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
        qn = quantize_normals(np.repeat(gn, 3, axis=0).astype(f32))
    if have is not None and g.has_uvs:
        qu = (have >> np.uint64(32)).astype(np.uint32)
    else:
        qu = quantize_uvs(np.zeros((3 * g.num_tris, 2), f32))
    return qn.astype(np.uint64) | (qu.astype(np.uint64) << np.uint64(32))


def write_vks(path, scene: Scene, version=4, material_names=None, lod_groups=None, wide_material_ids=None, index_buffers=False, animation=None,
              animation_start=0.0, animation_step=1.0 / 30.0):
    """Writes `scene` as <path> (.vks, file version 3 or 4) plus <base>_textures/ with what `read_vks` / the reference's
    `load_vkrs` pick up again. Constraints of the format, checked here: every parameterized mesh becomes a .vks mesh (a mesh
    shared by several parameterized meshes is written once per use), its geometries share one quantisation grid, instance
    transforms are rotation x uniform scale (stored with a 16-bit quaternion: they come back slightly rounded).
    Material parameters a .vks scene cannot express as literals are baked into textures the way the reference expects them:
    base colour -> <name>_BaseColor.vkt (sRGB; BC1 for opaque materials -- the loader only keeps BASE_MATERIAL_NOALPHA for the
    BC1 RGB formats, scene.cpp:857-873 -- RGBA8 for alpha-tested ones), roughness / metallic / specular ->
    <name>_Specular.vkt (BC1: g, b, r), normal map -> <name>_Normal.vkt (BC5); a material without a normal map gets none and
    the reader substitutes the reference's flat default texel (127, 127). Emission and transmission go into the .txt files.
    lod_groups (file version 4): [[(parameterized mesh, detail reduction), ...], ...] -- every list becomes a LoD group (vkr.h:261-270)
    whose first entry is the base level; the reader instances base levels only (scene.cpp:722-736).
    wide_material_ids: {parameterized mesh: uint16 ids} -- that mesh is written with 16-bit per-triangle material ids and a material
    range above 256 (vkr.c:1127-1130: two bytes per id when numMaterialsInRange > 0x100); index_buffers: every mesh also carries the
    (redundant, identity) index buffer of VKR_MESH_FLAGS_INDICES files -- the vertex streams of a .vks file are unrolled either way.
    animation (file version 4): {instance index: [3x4 transform of frame 0, of frame 1, ...]} -- the same number of frames for every
    entry (numFrames). Those instances get animated transform indices (>= numStaticTransforms); the table holds the static transforms,
    then per frame the animated ones (vkr_get_transform_offset, vkr.c:197-208). The scene's own transform of such an instance is not written.
    Returns the material names."""
    animation = {int(k): list(fr) for k, fr in (animation or {}).items()}
    n_frames = 1
    if animation:
        if version < 4:
            raise VksError("animated transforms need file version 4")
        n_frames = len(next(iter(animation.values())))
        if n_frames < 1 or any(len(fr) != n_frames for fr in animation.values()) or any(not 0 <= k < len(scene.instances) for k in animation):
            raise VksError("animation: one transform per frame for every animated instance of the scene")
    wide_material_ids = wide_material_ids or {}
    names = material_names or ["mat%03d" % i for i in range(len(scene.materials))]
    lod_groups = lod_groups or []
    if lod_groups and version < 4:
        raise VksError("LoD groups need file version 4")
    mesh_lod = {}
    for gi, group in enumerate(lod_groups):
        for pmesh, _ in group:
            mesh_lod[int(pmesh)] = gi + 1        # group 0 is the implicit "no levels of detail" group
    n_tris_total = 0
    mesh_blobs, mesh_headers = [], []
    for p, pm in enumerate(scene.pmeshes):
        mesh = scene.meshes[pm.mesh]
        geoms = scene.geometries[mesh.first_geometry:mesh.first_geometry + mesh.num_geometries]
        g0 = geoms[0]
        for g in geoms:
            if not (np.array_equal(np.asarray(g.scaling, f32), np.asarray(g0.scaling, f32)) and np.array_equal(np.asarray(g.offset, f32), np.asarray(g0.offset, f32))):
                raise VksError("parameterized mesh %d: the segments of a .vks mesh share one quantisation grid" % p)
        n = sum(g.num_tris for g in geoms)
        n_tris_total += n
        qpos = np.concatenate([np.asarray(g.qpos, np.uint64) for g in geoms])
        qnu = np.concatenate([_normal_uv_stream(g) for g in geoms])
        if pm.tri_material_ids is not None:
            if len(geoms) != 1:
                raise VksError("parameterized mesh %d: per-triangle materials need a single segment" % p)
            ids = np.asarray(pm.tri_material_ids, np.uint8)
            base, in_range = int(pm.material_offsets[0]), max(2, int(ids.max()) + 1)
            seg_offsets = [0]
        else:
            ids = np.zeros(n, np.uint8)
            base, in_range = 0, len(scene.materials)
            seg_offsets = [int(x) for x in pm.material_offsets]
            if len(geoms) == 1:          # a single segment with one material: numMaterialsInRange = 1 keeps the per-segment path
                base, in_range, seg_offsets = 0, 1, [int(pm.material_offsets[0])]
        if p in wide_material_ids:
            if len(geoms) != 1:
                raise VksError("parameterized mesh %d: per-triangle materials need a single segment" % p)
            ids = np.asarray(wide_material_ids[p], np.uint16)
            if len(ids) != n:
                raise VksError("parameterized mesh %d: one material id per triangle" % p)
            base, in_range, seg_offsets = int(pm.material_offsets[0]), max(0x101, int(ids.max()) + 1), [0]
        elif in_range > 0x100 and len(geoms) == 1:
            raise VksError("more than 256 materials in one segment")
        name = "mesh%04d" % p
        head = struct.pack("<3f3f", *[float(x) for x in g0.scaling], *[float(x) for x in g0.offset])
        tail = struct.pack("<QQiI", len(geoms), n, base, in_range)
        tail += struct.pack("<q4Q", mesh_lod.get(p, 0), 0, 0, 0, 0) if version >= 4 else struct.pack("<5Q", 0, 0, 0, 0, 0)
        tail += b"".join(struct.pack("<Q", g.num_tris) for g in geoms) + b"".join(struct.pack("<i", o) for o in seg_offsets) + _string(name)
        mesh_headers.append((head, tail))
        blob = qpos.tobytes() + qnu.tobytes() + ids.tobytes()
        if index_buffers:
            blob += np.arange(3 * n, dtype=np.uint32).tobytes()
        mesh_blobs.append(blob)
    transforms = [storable_transform(inst.transform) for inst in scene.instances]   # (version 3: one per instance, in the groups)
    static_ids = [k for k in range(len(scene.instances)) if k not in animation]
    animated_ids = sorted(animation)
    transform_index = {k: j for j, k in enumerate(static_ids)}
    transform_index.update({k: len(static_ids) + j for j, k in enumerate(animated_ids)})
    table = [transforms[k] for k in static_ids] + [storable_transform(animation[k][fr]) for fr in range(n_frames) for k in animated_ids]
    # ---- sizes first: every header carries absolute offsets
    scene_header = 8 + 24 + 5 * 8 + (struct.calcsize("<QqQqffQQQq") if version >= 4 else 0)
    at = scene_header
    mesh_header_end = []
    for head, tail in mesh_headers:
        at += len(head) + 24 + len(tail)
        mesh_header_end.append(at)
    group_meta = []
    for k, inst in enumerate(scene.instances):      # one group per instance
        name = _string("inst%05d" % k)
        data_off = at + 8 + 24 + len(name)
        end = data_off + (4 if version >= 4 else 48)
        group_meta.append((name, data_off, end))
        at = end
    lod_offset = at
    if version >= 4:
        at += 8                                      # group 0: zero levels
        for group in lod_groups:
            at += 8 + 12 * len(group)                # count, mesh ids (i64), detail reductions (f32)
    data_offset = at
    at += sum(len(_string(nm)) for nm in names)
    mesh_data_offset = []
    for blob in mesh_blobs:
        mesh_data_offset.append(at)
        at += len(blob)
    animation_offset = at
    with open(path, "wb") as f:
        f.write(struct.pack("<ii3Q", VKR_MAGIC, version, 0, scene_header, data_offset))
        f.write(struct.pack("<5Q", len(scene.pmeshes), len(scene.instances), len(names), n_tris_total, len(scene.instances)))
        if version >= 4:
            f.write(struct.pack("<QqQqffQQQq", 1 + len(lod_groups), lod_offset, 0, 0, float(animation_start) if animation else 0.0,
                                float(animation_step) if animation else 0.0, n_frames, len(static_ids), len(animated_ids), animation_offset))
        for (head, tail), end, off in zip(mesh_headers, mesh_header_end, mesh_data_offset):
            f.write(head + struct.pack("<3Q", MESH_FLAGS_INDICES if index_buffers else 0, end, off) + tail)
        for k, (inst, (name, data_off, end)) in enumerate(zip(scene.instances, group_meta)):
            f.write(struct.pack("<Ii3Q", 0, inst.pmesh, end, data_off, 1) + name)
            f.write(struct.pack("<I", transform_index[k]) if version >= 4 else np.asarray(transforms[k], f32).tobytes())
        if version >= 4:
            f.write(struct.pack("<Q", 0))
            for group in lod_groups:
                f.write(struct.pack("<Q", len(group)) + b"".join(struct.pack("<q", int(m)) for m, _ in group)
                        + b"".join(struct.pack("<f", float(d)) for _, d in group))
        for nm in names:
            f.write(_string(nm))
        for blob in mesh_blobs:
            f.write(blob)
        if version >= 4:
            for t in table:
                f.write(quantize_transform(t))
    # ---- materials
    tdir = texture_dir(path)
    os.makedirs(tdir, exist_ok=True)
    for nm, mat in zip(names, scene.materials):
        def literal_or_texture(value, channel_of=None):
            bits = abi.float_bits(value)
            if bits & 0x80000000:
                t = scene.textures[bits & 0x1FFFFFFF]
                return t.rgba if channel_of is None else t.rgba[..., (bits >> 29) & 3], t.srgb
            return None, False
        base_tex, _ = literal_or_texture(mat.base_color[0])
        emissive = mat.emission_intensity > 0
        if base_tex is None and not emissive:
            rgb = _linear_to_srgb8([mat.base_color[0], mat.base_color[1], mat.base_color[2]])
            base_tex = _solid([rgb[0], rgb[1], rgb[2], 255])
        if base_tex is not None:
            bits = abi.float_bits(mat.base_color[0])
            base_mips = scene.textures[bits & 0x1FFFFFFF].mips if (bits & 0x80000000) else None   # a texture's mip levels go along
            write_vkt(tdir + nm + "_BaseColor.vkt", base_tex, FMT_BC1_RGB_SRGB if (mat.flags & abi.BASE_MATERIAL_NOALPHA) else FMT_RGBA8_UNORM, mips=base_mips)
        chans = []
        for value in (mat.specular, mat.roughness, mat.metallic):
            tex, _ = literal_or_texture(value, channel_of=True)
            chans.append(tex if tex is not None else np.array([[int(np.clip(np.floor(float(value) * 255.0 + 0.5), 0, 255))]], np.uint8))
        h = max(c.shape[0] for c in chans)
        w = max(c.shape[1] for c in chans)
        if any(c.shape not in ((1, 1), (h, w)) for c in chans):
            raise VksError("material %s: specular / roughness / metallic textures of different sizes" % nm)
        spec = np.stack([np.broadcast_to(c, (h, w)) for c in chans] + [np.full((h, w), 255, np.uint8)], axis=2)
        write_vkt(tdir + nm + "_Specular.vkt", spec if (h, w) != (1, 1) else _solid(spec[0, 0]), FMT_BC1_RGB_UNORM)
        if mat.normal_map != -1:
            write_vkt(tdir + nm + "_Normal.vkt", scene.textures[mat.normal_map].rgba, FMT_BC5_UNORM, mips=scene.textures[mat.normal_map].mips)
        if emissive:
            lit = [0.0, 0.0, 0.0] if base_tex is not None else [float(mat.base_color[k]) for k in range(3)]
            with open(tdir + nm + "_EmissionIntensity.txt", "w") as f:
                f.write("".join("%.9g\n" % x for x in [float(mat.emission_intensity)] + lit))
        if mat.specular_transmission != 0.0 or mat.ior != 1.5:
            with open(tdir + nm + "_SpecularTransmission.txt", "w") as f:
                f.write("%.9g\n%.9g\n0\n0\n" % (float(mat.specular_transmission), float(mat.ior)))
    return names


# ------------------------------------------------------------------ command line: .vks -> flat scene dump for the C++ host tools
def main(argv=None):
    """python -m realtimepathtracingresearchframework_amd.vks scene.vks --dump scene.rpsc [--eye x y z --center x y z --up x y z
    --fov f] [--sky KEY]: loads a .vks scene the way the reference does and writes the flat file `bin/rptr_hip` reads
    (host/scene_dump.hpp), i.e. what a reference-side adapter would hand to the backend after its own `Scene` load."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m realtimepathtracingresearchframework_amd.vks", description=main.__doc__)
    ap.add_argument("vks")
    ap.add_argument("--dump", required=True, help="output path of the flat scene file")
    ap.add_argument("--eye", type=float, nargs=3)
    ap.add_argument("--center", type=float, nargs=3)
    ap.add_argument("--up", type=float, nargs=3)
    ap.add_argument("--fov", type=float)
    ap.add_argument("--sky", default="default", choices=sorted(SKY_CONFIGS), help="sky configuration (scenes.SKY_CONFIGS)")
    ap.add_argument("--ignore-textures", action="store_true")
    args = ap.parse_args(argv)
    s = read_vks(args.vks, ignore_textures=args.ignore_textures)
    cam = dict(s.camera)
    for key in ("eye", "center", "up"):
        if getattr(args, key) is not None:
            cam[key] = tuple(getattr(args, key))
    if args.fov is not None:
        cam["fov"] = args.fov
    s.camera = cam
    s.config = SceneConfig(**SKY_CONFIGS[args.sky])
    s.sky_key = args.sky
    s.dump(args.dump)
    print("%s: %d meshes, %d instances, %d triangles, %d materials, %d textures, %d emitters -> %s" % (
        args.vks, len(s.meshes), len(s.instances), s.num_tris(), len(s.materials), len(s.textures), len(s.lights), args.dump))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
