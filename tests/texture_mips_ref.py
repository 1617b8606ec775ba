"""The mip filter of include/rptr_hip.h "dynamic textures" (csrc/texture_mips.h rp_k_mip_level) restated in numpy float32: one level
and a whole chain. The reference renderer generates no mip levels, so the rule in the header is the definition; this file states it tap
by tap, the way the kernel walks it, and takes the sRGB decode table as an argument (backend.srgb_decode_table()).

  sizes:  a source of h x w texels gives max(1, h >> 1) x max(1, w >> 1); level l + 1 is made from the QUANTISED level l
  taps per axis of source size n at destination coordinate x, (source index, integer weight):
      n == 1                   (0, 1)                                          total 1
      n even                   (2x, 1), (2x + 1, 1)                            total 2
      n odd >= 3, m = n >> 1   (2x, m - x), (2x + 1, m), (2x + 2, x + 1)       total n
  per channel, binary32, every operation rounded on its own:
      f(c) = table[c] (colour channels of an sRGB texture) or float(c) (alpha; every channel of a linear texture)
      acc = 0; for ty in row order, tx in column order: acc = acc + float(wx * wy) * f(texel[ty][tx])
      mean = acc / float(totx * toty)
      linear code: min(255, int(mean + 0.5f));  sRGB code: the number of k in 1..255 with mean >= T[k], T[k] = (table[k-1] + table[k]) * 0.5f
"""
import numpy as np

f32 = np.float32


def axis_taps(n):
    """-> (index (m, k) int64, weight (m, k) int64, total): the k taps of each of the m = max(1, n >> 1) destination coordinates"""
    if n == 1:
        return np.zeros((1, 1), np.int64), np.ones((1, 1), np.int64), 1
    m = n >> 1
    x = np.arange(m, dtype=np.int64)
    if n % 2 == 0:
        return np.stack([2 * x, 2 * x + 1], axis=1), np.ones((m, 2), np.int64), 2
    return np.stack([2 * x, 2 * x + 1, 2 * x + 2], axis=1), np.stack([m - x, np.full(m, m, np.int64), x + 1], axis=1), n


def thresholds(table):
    """T[0..255], T[0] = 0 (never compared), T[k] = (table[k - 1] + table[k]) * 0.5f"""
    table = np.asarray(table, f32)
    T = np.zeros(256, f32)
    T[1:] = (table[:-1] + table[1:]) * f32(0.5)
    return T


def encode_srgb(mean, T, chunk=1 << 14):
    """the number of k in 1..255 with mean >= T[k], counted (in chunks: the comparison table is 255 times the input)"""
    flat = np.ascontiguousarray(mean, f32).reshape(-1)
    out = np.empty(len(flat), np.int32)
    for at in range(0, len(flat), chunk):
        out[at:at + chunk] = (flat[at:at + chunk, None] >= T[None, 1:]).sum(axis=1)
    return out.reshape(np.shape(mean))


def level(src, srgb, table):
    """the next level of `src` (h, w, 4) uint8"""
    src = np.ascontiguousarray(src, np.uint8)
    table = np.asarray(table, f32)
    iy, wy, toty = axis_taps(src.shape[0])
    ix, wx, totx = axis_taps(src.shape[1])
    f = src.astype(f32)
    if srgb:
        f[..., :3] = table[src[..., :3]]
    acc = np.zeros((iy.shape[0], ix.shape[0], 4), f32)
    for r in range(iy.shape[1]):
        for c in range(ix.shape[1]):
            w = (wy[:, r][:, None] * wx[:, c][None, :]).astype(f32)   # the integer product, converted once
            texel = f[iy[:, r][:, None], ix[:, c][None, :]]
            acc = acc + w[..., None] * texel
    mean = acc / f32(totx * toty)
    code = np.minimum((mean + f32(0.5)).astype(np.int32), 255)
    if srgb:
        code[..., :3] = encode_srgb(mean[..., :3], thresholds(table))
    return code.astype(np.uint8)


def chain(rgba, srgb, table):
    """[level 1, ..., the 1 x 1 level] of a level 0 (h, w, 4) uint8 (empty for a 1 x 1 texture)"""
    out, cur = [], np.ascontiguousarray(rgba, np.uint8)
    while cur.shape[0] > 1 or cur.shape[1] > 1:
        cur = level(cur, srgb, table)
        out.append(cur)
    return out


def full_levels(h, w):
    n = 1
    while h > 1 or w > 1:
        h, w, n = max(1, h >> 1), max(1, w >> 1), n + 1
    return n


def srgb_decode64(c):
    """IEC 61966-2-1 decode of the 8-bit codes c in float64"""
    v = np.asarray(c, np.float64) / 255.0
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
