"""Inputs of the shading-function tests -- fixed-seed random sets plus the edges where binary32 code goes wrong. One set feeds the
oracle (tests/test_shade_ref64.py, on the CPU first) and the device probes (tests/test_gpu_shade_functions.py)."""
import numpy as np

from realtimepathtracingresearchframework_amd import abi, scenes

F32 = np.float32
ULP_UP = lambda x: np.nextafter(F32(x), F32(np.inf))  # noqa: E731
ULP_DN = lambda x: np.nextafter(F32(x), F32(-np.inf))  # noqa: E731


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def materials(transmission=False):
    """(name, abi.BaseMaterial): roughness at 0, at the 0.002 alpha clamp +- 1 ulp, 0.1, 1; metallic 0 / 1; specular 0; black base;
    ior 1 (Schlick F0 = 0), 1 + 2^-23, 1.5, 3"""
    r_clamp = F32(np.sqrt(F32(0.002)))
    out = []
    for rough in (F32(0.0), ULP_DN(r_clamp), r_clamp, ULP_UP(r_clamp), F32(0.1), F32(0.45), F32(1.0)):
        out.append(("rough=%r" % float(rough), abi.make_material((0.6, 0.5, 0.4), roughness=float(rough), metallic=0.0, ior=1.5)))
    for ior in (F32(1.0), ULP_UP(1.0), F32(3.0)):
        out.append(("ior=%r" % float(ior), abi.make_material((0.6, 0.5, 0.4), roughness=0.3, metallic=0.0, ior=float(ior))))
    out.append(("metal", abi.make_material((0.9, 0.6, 0.3), roughness=0.2, metallic=1.0, ior=1.5)))
    out.append(("black_spec0", abi.make_material((0.0, 0.0, 0.0), roughness=0.5, specular=0.0, metallic=0.0, ior=1.5)))
    # F0 = 0 and no diffuse lobe: F = the Schlick weight itself, so its clamp of 1 - |o.h| at |o.h| = 1 + 1 ulp decides the sign of f
    out.append(("black_metal", abi.make_material((0.0, 0.0, 0.0), roughness=0.3, metallic=1.0, ior=1.5)))
    if transmission:
        for name, m in list(out):
            g = abi.make_material((0.9, 0.95, 1.0), roughness=float(m.roughness), metallic=0.0, ior=float(m.ior),
                                  flags=abi.BASE_MATERIAL_NOALPHA | abi.BASE_MATERIAL_ONESIDED)
            g.specular_transmission = 0.9
            g.clearcoat_gloss = 0.04
            out.append((name + "+glass", g))
    return out


def bsdf_directions(n_random=65536, seed=1):
    """(n, wo, wi, u4): random frames (both sides) followed by the edges: n along +-x, +-y, +-z (the basis branches) and off unit
    length by an ulp; n . w_o in {1, 1e-7, 0, -1e-7}; w_i the exact mirror of w_o (half vector = n), w_i = w_o, w_i below the horizon;
    the samples 0 and 1 - 2^-24"""
    rng = np.random.default_rng(seed)
    n = _unit(rng.normal(size=(n_random, 3)))
    wo = _unit(rng.normal(size=(n_random, 3)))
    wi = _unit(rng.normal(size=(n_random, 3)))
    u = rng.random((n_random, 4)).astype(F32)
    en, ewo, ewi = [], [], []
    axes = [np.eye(3, dtype=F32)[k] * s for k in range(3) for s in (1, -1)]
    tilted = [_unit([0.3, 0.8, 0.52]), _unit([-0.61, 0.2, -0.77])]
    off = [a * ULP_UP(1.0) for a in axes[:2]] + [tilted[0] * ULP_DN(1.0)]
    for nn in axes + tilted + off:
        t = _unit(np.cross(nn, [0.37, 0.41, 0.83]))
        for c in (1.0, 1e-7, 0.0, -1e-7, 0.5, -0.5):
            s = np.sqrt(max(0.0, 1.0 - c * c))
            w_o = _unit(np.asarray(nn, np.float64) * c + t * s) if c not in (1e-7, -1e-7) else (t * F32(s) + nn * F32(c)).astype(F32)
            mirror = (2.0 * np.dot(nn, w_o) * np.asarray(nn, np.float64) - w_o).astype(F32)
            below = _unit(-np.asarray(nn, np.float64) * 0.4 + t * 0.9)
            for w_i in (mirror, w_o, below, _unit(nn), _unit(np.asarray(nn) * 0.2 - t)):
                en.append(nn), ewo.append(w_o), ewi.append(w_i)
    m = len(en)
    eu = np.tile(np.array([[0, 0, 0, 0], [1 - 2 ** -24] * 4, [0.5, 0.25, 0.999, 0.0], [0.0, 1 - 2 ** -24, 0.5, 1 - 2 ** -24]], F32), (m // 4 + 1, 1))[:m]
    return (np.concatenate([n, np.array(en, F32)]), np.concatenate([wo, np.array(ewo, F32)]), np.concatenate([wi, np.array(ewi, F32)]),
            np.concatenate([u, eu]), n_random)


def triangles(n_random=65536, seed=2):
    """(v9 relative to the shading point, u2, the number of random triangles in front): random triangles at distance 0.5 .. 20, then the edges --
    1e-12 sr triangles at 1e4 .. 1e6, the shading point in the triangle's plane, collinear and zero-area triangles, v0.x = +-0 (the
    Householder sign), a near-hemisphere triangle, the samples 0 and 1 - 2^-24"""
    rng = np.random.default_rng(seed)
    c = _unit(rng.normal(size=(n_random, 3))) * rng.uniform(0.5, 20.0, (n_random, 1)).astype(F32)
    v = (c[:, None, :] + rng.normal(size=(n_random, 3, 3)) * rng.uniform(0.05, 2.0, (n_random, 1, 1))).astype(F32)
    u = rng.random((n_random, 2)).astype(F32)
    e = []
    for d in (1e4, 1e5, 1e6):
        s = d * 1e-6 * 1.4
        e.append([[d, 0, 0], [d, s, 0], [d, 0, s]])
        e.append([[0.3 * d, d, 0.2 * d], [0.3 * d + s, d, 0.2 * d], [0.3 * d, d, 0.2 * d + s]])
    e += [[[1, 0, 0], [0, 1, 0], [-1, 1, 0]],                    # in the plane z = 0
          [[1, 1, 1], [2, 2, 2], [3, 3, 3]],                      # collinear with the point
          [[1, 0, 1], [2, 0, 1], [3, 0, 1]],                      # collinear vertices
          [[1, 1, 1], [1, 1, 1], [1, 1, 1]],                      # zero area
          [[0.0, 1, 0], [0.5, 1, 0], [0, 1, 0.5]],                # v0.x = +0
          [[-0.0, 1, 0], [0.5, 1, 0], [0, 1, 0.5]],               # v0.x = -0
          [[1, -1e-3, -1e-3], [-0.5, 0.866, -1e-3], [-0.5, -0.866, 1e-3]],  # almost a hemisphere: 1 + d01 + d02 + d12 -> 0
          [[1, 0, 0], [-0.5, 0.866, 0], [-0.5, -0.866, 1e-7]]]
    e = np.array(e, F32)
    eu = np.tile(np.array([[0, 0], [1 - 2 ** -24, 1 - 2 ** -24], [0.5, 0.0], [0.0, 1 - 2 ** -24]], F32), (len(e), 1))
    ev = np.repeat(e, 4, axis=0)
    v9 = np.concatenate([v.reshape(-1, 9), ev.reshape(-1, 9)])
    return v9, np.concatenate([u, eu]), n_random


def srgb_inputs(n_random=65536, seed=3):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.random(n_random).astype(F32), (rng.random(4096) * 8).astype(F32)])
    k = F32(0.0031308)
    e = np.array([0.0, -0.0, 1e-45, 1e-40, ULP_DN(k), k, ULP_UP(k), 1.0, ULP_DN(1.0), 1.5, 1e6, -0.5, -1e-3, np.nan, np.inf, -np.inf], F32)
    return np.concatenate([x, e])


def half_inputs(seed=4):
    """floats for the RGBA16F conversion: ties between halves, values above 65504, half denormals, random values"""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 0x7C00, 20000).astype(np.uint16).view(np.float16).astype(np.float32)
    ties = (h.astype(np.float64) + np.abs(np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float64) - h) / 2).astype(F32)
    e = np.array([65504.0, 65519.0, 65520.0, 65536.0, 1e9, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14, ULP_DN(2.0 ** -14), 1e-10, -0.0,
                  np.nan, np.inf, -np.inf, -65520.0], F32)
    x = np.concatenate([h, -ties, ties, rng.normal(size=20000).astype(F32) * 100, e])
    pad = (-len(x)) % 4
    return np.concatenate([x, np.zeros(pad, F32)]).reshape(-1, 4)


def texture_set(seed=5):
    """(name, level list, srgb): 1 x 1, 1 x N, N x 1, 3 x 5, 16 x 16 with a full chain and with one level; sRGB and linear"""
    rng = np.random.default_rng(seed)

    def chain(base):
        out, cur = [base], base.astype(np.float64)
        while cur.shape[0] > 1 or cur.shape[1] > 1:
            h, w = max(1, cur.shape[0] // 2), max(1, cur.shape[1] // 2)
            cur = cur[:2 * h if cur.shape[0] > 1 else 1, :2 * w if cur.shape[1] > 1 else 1]
            cur = cur.reshape(h, cur.shape[0] // h, w, cur.shape[1] // w, 4).mean(axis=(1, 3))
            out.append(np.clip(np.round(cur), 0, 255).astype(np.uint8))
        return out

    t = lambda h, w: rng.integers(0, 256, (h, w, 4)).astype(np.uint8)  # noqa: E731
    b16, b35 = t(16, 16), t(3, 5)
    return [("1x1", [t(1, 1)], False), ("1x7", chain(t(1, 7)), True), ("8x1", chain(t(8, 1)), False), ("3x5", chain(b35), True),
            ("3x5_single", [b35], False), ("16x16", chain(b16), False), ("16x16_srgb", chain(b16), True), ("16x16_single", [b16], False)]


def texture_queries(w, h, levels, n_random=8192, seed=6):
    """(uv (N, 2), lod (N,), ddx (N, 2), ddy (N, 2)): random queries, then uv edges (0, -0, 1, texel centres and edges +- 1 ulp,
    -1e-8, -3.75, 1e6, 3e9, 1e10 (beyond the int range in texels), +-inf, NaN), lod edges (NaN, -1, 0, integers, levels - 1, 40) and
    derivative edges (zero, one of them zero, equal, 1e-30, 1e30, anisotropy exactly 12 and just above)"""
    rng = np.random.default_rng(seed)
    uv = (rng.random((n_random, 2)) * 3 - 1).astype(F32)
    lod = (rng.random(n_random) * (levels + 1) - 0.5).astype(F32)
    ddx = (rng.normal(size=(n_random, 2)) * rng.choice([0.01, 0.1, 0.5], (n_random, 1))).astype(F32)
    ddy = (rng.normal(size=(n_random, 2)) * rng.choice([0.01, 0.1, 0.5], (n_random, 1))).astype(F32)
    cs = []
    for size in (w, h):
        c = [0.0, -0.0, 1.0, -1e-8, -3.75, 1e6, 3e9, 1e10, -1e10, np.inf, -np.inf, np.nan]
        for i in range(min(size, 4)):
            for p in ((i + 0.5) / size, i / size):
                p = F32(p)
                c += [p, ULP_UP(p), ULP_DN(p)]
        cs.append(np.array(c, F32))
    eu = np.array(np.meshgrid(cs[0], cs[1])).reshape(2, -1).T.astype(F32)
    el = np.array([np.nan, -1.0, 0.0, 1.0, 2.0, 3.0, levels - 1, ULP_DN(levels - 1), 40.0, 0.5, np.inf, -np.inf], F32)
    k = len(eu)
    lod = np.concatenate([lod, el[np.arange(k) % len(el)]])
    uv = np.concatenate([uv, eu])
    dx = [[0, 0], [0, 0], [0.25, 0], [0.25, 0], [1e-30, 0], [1e30, 0], [12 * 2.0 / w, 0], [12 * 2.0 / w * (1 + 2 ** -20), 0], [3.0 / w, 1.0 / h],
          [np.nan, 0], [np.inf, 0]]
    dy = [[0, 0], [0, 0.25], [0, 0.25], [0, 0], [0, 1e-30], [0, 1e30], [0, 2.0 / h], [0, 2.0 / h], [3.0 / w, 1.0 / h], [0, 0.1], [0, np.inf]]
    ex = np.array(dx, F32)[np.arange(k) % len(dx)]
    ey = np.array(dy, F32)[np.arange(k) % len(dy)]
    return uv, lod, np.concatenate([ddx, ex]), np.concatenate([ddy, ey])


def texture_scene(levels, srgb):
    """a scene whose texture 0 is the level list (the oracle samples its scene's textures)"""
    s = scenes.textured_test()
    s.textures = [scenes.Texture(rgba=levels[0], srgb=srgb, mips=levels[1:] or None)]
    return s


def oct_words(seed=7, n_random=4096):
    """octahedral normal words: the poles, the fold (|x| + |y| = 1), the corners, random"""
    rng = np.random.default_rng(seed)
    e = []
    for x in (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x4000, 0xC000, 0xBFFF):
        for y in (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x4000, 0xC000, 0xBFFF):
            e.append(x | (y << 16))
    for k in range(0, 0x7FFF, 997):  # on the fold: |x| + |y| = 0x7FFF
        e += [(0x8000 + k) | ((0x8000 + 0x7FFF - k) << 16), (0x8000 - k) | ((0x8000 + (0x7FFF - k)) << 16)]
    r = rng.integers(0, 2 ** 32, n_random, dtype=np.uint64)
    return np.concatenate([np.array(e, np.uint64), r])
