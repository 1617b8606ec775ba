"""The oracle's shading functions against the float64 restatement (tests/shade_ref64.py), on the CPU: the independent side of the
device tests (tests/test_gpu_shade_functions.py) is validated here before any GPU run, and every edge input those tests hand to the
device goes through the oracle first -- an input that indexed outside its arrays would show up on the host.

Bounds (excess: how far the binary32 result lies outside the float64 band over one-ulp input neighbourhoods, shade_ref64.band), with
the values measured on the oracle:
  glTF f / wpdf            relative excess <= 2e-3 on random directions, <= 2e-5 for 99.9 % of them (measured 1.2e-3 / 1.1e-5, the
                           largest at roughness <= 0.1: the cancellation in 1 + (a^2 - 1) cos^2 that a band over INPUT ulps does not
                           see); finite wherever the band is (the grazing edges reach 0.54 relative and are only held to finiteness)
                           black metal (F0 = 0, no diffuse): 2e-2 / 5e-5 (measured 1.6e-2 / 3.5e-5, see GLTF_REL_F0_ZERO)
  Lambert f / pdf          relative excess <= 1e-6
  sun pdf, MIS weight      4 ulps of the result
  sRGB encode (powf)       4 ulps (measured 2.3)
  textures                 16 ulps of 1 (measured 12.7)
  triangle solid angle     |omega - exact| <= 2 * 1.16e-5 + 2e-6 on well-conditioned triangles (measured 2.46e-5)
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import shade_cases as S
import shade_ref64 as R
from common import rel_excess
from oracle_lib import _p

K_IEEE = 4.0


def oracle_gltf_eval(m, n, wo, wi, transmission=False):
    N = len(n)
    f, wpdf = np.zeros((N, 3), np.float32), np.zeros(N, np.float32)
    fn = O.lib().orc_gltf_t_eval if transmission else O.lib().orc_gltf_eval
    fn(C.byref(m), _p(n), _p(wo), _p(wi), N, _p(f), _p(wpdf))
    return f, wpdf


def _report(name, e):
    e = e[np.isfinite(e)] if np.any(np.isfinite(e)) else np.zeros(1)
    print("%-34s max band excess %.2f ulp" % (name, float(np.max(e))))


LAMBERT_REL_MAX = 1e-6
GLTF_REL_MAX = 2e-3     # largest relative excess over the band, random directions (measured on the oracle: see the module docstring)
GLTF_REL_TAIL = 2e-5    # ... exceeded by at most 0.1 % of them
# F0 = 0 with no diffuse lobe (black metal): f = D G (1 - |o.h|)^5, and the rounding of |o.h| near 1 -- inside normalize(w_i + w_o), not
# an input ulp -- moves (1 - |o.h|)^5 by 5 ulp(1) / (1 - |o.h|) relative: measured 1.6e-2 / 3.5e-5
GLTF_REL_F0_ZERO = (2e-2, 5e-5)


def gltf_rel_bounds(name):
    return GLTF_REL_F0_ZERO if name.startswith("black_metal") else (GLTF_REL_MAX, GLTF_REL_TAIL)


def gltf_band_check(name, n, wo, wi, nr, f, wpdf, M):
    flo, fhi = R.band(lambda a, b, c: R.gltf_eval(M, a, b, c)[0], (n, wo, wi))
    plo, phi = R.band(lambda a, b, c: R.gltf_eval(M, a, b, c)[1], (n, wo, wi))
    ef = rel_excess(f, flo, fhi).max(axis=1)
    ep = rel_excess(wpdf, plo, phi)
    e = np.maximum(ef, ep)
    # w_i = -w_o: no half vector (normalize(0)); the binary32 code gives NaN there, float64 an arbitrary band
    defined = np.any(wi + wo != 0, axis=1)
    finite = np.isfinite(flo).all(axis=1) & np.isfinite(fhi).all(axis=1) & np.isfinite(plo) & np.isfinite(phi) & defined
    rnd = np.arange(len(n)) < nr
    print("%-28s rel excess: max %.2e, 99.9 %% %.2e (random) / max %.2e (edges), non-finite %d" % (
        name, e[rnd].max(), np.quantile(e[rnd], 0.999), e[~rnd & finite].max(), int((~np.isfinite(f).all(axis=1) | ~np.isfinite(wpdf))[finite].sum())))
    emax, etail = gltf_rel_bounds(name)
    assert e[rnd & finite].max() <= emax and np.quantile(e[rnd & finite], 0.999) <= etail
    assert np.isfinite(f[finite]).all() and np.isfinite(wpdf[finite]).all()
    return e


@pytest.mark.parametrize("name,m", S.materials(), ids=[n for n, _ in S.materials()])
def test_oracle_gltf_against_float64(name, m):
    n, wo, wi, u, nr = S.bsdf_directions()
    f, wpdf = oracle_gltf_eval(m, n, wo, wi)
    gltf_band_check(name, n, wo, wi, nr, f, wpdf, R.material(m))


def test_oracle_lambert_against_float64():
    n, wo, wi, u, nr = S.bsdf_directions(n_random=4096)
    base = np.array([0.7, 0.3, 0.05], np.float32)
    f, pdf = np.zeros((len(n), 3), np.float32), np.zeros(len(n), np.float32)
    wi_s, w_s = np.zeros(3, np.float32), np.zeros(3, np.float32)
    p, mp, q = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
    for i in range(len(n)):
        O.lib().orc_simple_probe(_p(base), _p(n[i]), _p(wo[i]), _p(u[i, :2].copy()), _p(wi[i]), _p(wi_s), _p(w_s), _p(p), _p(mp), _p(f[i]), _p(q))
        pdf[i] = q[0]
    lo, hi = R.band(lambda a, b, c: R.simple_eval(base, a, b, c)[0], (n, wo, wi))
    plo, phi = R.band(lambda a, b, c: R.simple_eval(base, a, b, c)[1], (n, wo, wi))
    e = np.maximum(rel_excess(f, lo, hi).max(axis=1), rel_excess(pdf, plo, phi))
    rnd = np.arange(len(n)) < nr
    print("lambert rel excess max %.2e (random)" % e[rnd].max())
    assert e[rnd].max() <= LAMBERT_REL_MAX and np.isfinite(f).all() and np.isfinite(pdf).all()


def oracle_tri_light(v9, u2):
    out = np.zeros((len(v9), 9), np.float32)
    O.lib().orc_tri_light_probe(_p(np.ascontiguousarray(v9, np.float32)), _p(np.ascontiguousarray(u2, np.float32)), len(v9), _p(out))
    return out


def well_conditioned(v9):
    """triangles of 1e-4 .. 2 sr whose vertices are no closer than 1 % of their distance to one another in direction"""
    exact = R.tri_solid_angle(v9)
    d = np.asarray(v9, np.float64).reshape(-1, 3, 3)
    d = d / np.linalg.norm(d, axis=2, keepdims=True)
    sep = np.min([np.linalg.norm(d[:, i] - d[:, j], axis=1) for i, j in ((0, 1), (1, 2), (0, 2))], axis=0)
    return (exact > 1e-4) & (exact < 2.0) & (sep > 1e-2)


SOLID_ANGLE_ROUNDING = 2e-6   # binary32 rounding of the determinant and the tangent (measured excess over 2 * 1.16e-5: 1.4e-6)


def test_oracle_triangle_solid_angle_against_van_oosterom_strackee():
    """tri.glsl's Householder determinant + fast_positive_atan against the exact solid angle: within twice the approximation's stated
    1.16e-5 absolute error (tri.glsl:54-57) plus binary32 rounding on well-conditioned triangles; edge triangles stay finite and
    non-negative (the zero-area ones give 0)"""
    v9, u2, nr = S.triangles()
    out = oracle_tri_light(v9, u2)
    exact = R.tri_solid_angle(v9)
    ok = well_conditioned(v9)
    assert ok[:nr].mean() > 0.9
    err = np.abs(out[:, 0].astype(np.float64) - exact)
    bound = 2 * R.FAST_ATAN_MAX_ABS_ERROR + SOLID_ANGLE_ROUNDING
    print("solid angle: max |omega - exact| %.3e (bound %.3e), %d triangles" % (err[ok].max(), 2 * R.FAST_ATAN_MAX_ABS_ERROR, ok.sum()))
    assert (err[ok] <= bound).all()
    assert np.isfinite(out[nr:, 0]).all() and (out[nr:, 0] >= 0).all()
    # the sampled directions are unit vectors inside the cone of the triangle's vertices (well-conditioned ones)
    d = out[ok, 5:8].astype(np.float64)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-5)


def test_oracle_sun_pdf_and_mis_against_float64():
    cosr = np.array([np.cos(np.radians(0.53) / 2), 1 - 2 ** -24, 1 - 2 ** -23, 0.5, 0.0, -1.0, 0.9999], np.float32)
    out = np.zeros_like(cosr)
    O.lib().orc_sun_pdf(_p(cosr), len(cosr), _p(out))
    lo, hi = R.band(R.sun_dir_pdf, (cosr,))
    assert np.max(R.band_excess(out, lo, hi)) <= K_IEEE
    rng = np.random.default_rng(11)
    f = np.concatenate([rng.random(4096) * 10, [3e38, 2e38, 1e-40, 1e-45, 0.0, 1.0, 2.0 ** 127]]).astype(np.float32)
    g = np.concatenate([rng.random(4096) * 10, [3e38, 1e38, 1e-40, 1e-45, 1e-45, 0.0, 2.0 ** 127]]).astype(np.float32)
    w = np.zeros_like(f)
    O.lib().orc_nee_mis(_p(f), _p(g), len(f), _p(w))
    lo, hi = R.band(R.nee_mis, (f, g))
    # (f + g overflows to inf above 2^127 each: the binary32 weight is 0 where float64 says 0.5 -- reported, not bounded here)
    fin = np.isfinite(f.astype(np.float32) + g)
    assert np.max(R.band_excess(w[fin], lo[fin], hi[fin])) <= K_IEEE


def test_oracle_srgb_against_float64():
    x = S.srgb_inputs()
    out = np.zeros_like(x)
    O.lib().orc_linear_to_srgb(_p(x), len(x), _p(out))
    lo, hi = R.band(R.linear_to_srgb, (x,))
    e = R.band_excess(out, lo, hi)
    _report("linear_to_srgb", e)
    assert np.max(e) <= 4.0
    # NaN: positive_pow's fmax(|x|, FLT_EPSILON) (util.glsl:19-28) returns the epsilon, the upper branch at 2^-23 comes out
    nan_out = out[np.isnan(x)].astype(np.float64)
    assert (np.abs(nan_out - (1.055 * (2.0 ** -23) ** (1 / 2.4) - 0.055)) <= 4 * R.ulp32(nan_out)).all()


def test_oracle_dequantize_against_float64():
    rng = np.random.default_rng(12)
    q = rng.integers(0, 2 ** 63, 4096, dtype=np.uint64)
    q = np.concatenate([q, np.array([0, 2 ** 63 - 1, 0x1FFFFF | (0x1FFFFF << 21) | (0x1FFFFF << 42)], np.uint64)])
    sc, of = np.array([1e-3, 2e-6, 7.5e-4], np.float32), np.array([-1.0, 3.5, -1000.0], np.float32)
    xyz = np.zeros((len(q), 3), np.float32)
    O.lib().orc_dequantize_positions(_p(q), len(q), _p(sc), _p(of), _p(xyz))
    ref = R.dequantize_position(q, sc, of)
    # q * scaling + offset: two roundings
    assert (np.abs(xyz - ref) <= 2 * R.ulp32(np.maximum(np.abs(ref), np.abs(of))) + 1e-30).all()
    w = S.oct_words()
    words = (w | (w << np.uint64(32))).astype(np.uint64)
    nrm, uv = np.zeros((len(w), 3), np.float32), np.zeros((len(w), 2), np.float32)
    O.lib().orc_dequantize_normal_uv(_p(words), len(w), _p(nrm), _p(uv))
    rn, ru = R.dequantize_normal(w), R.dequantize_uv(w)
    assert np.abs(nrm - rn).max() <= 4 * 2 ** -24 * 4
    assert (np.abs(uv - ru) <= 4 * R.ulp32(np.maximum(np.abs(ru), 1.0))).all()


TEXTURE_ULPS = 16   # of 1 (2^-24): float weights times texels summed in four steps; measured 12.7


@pytest.mark.parametrize("tex", S.texture_set(), ids=[t[0] for t in S.texture_set()])
def test_oracle_texture_sampler_against_float64(tex):
    name, levels, srgb = tex
    h, w = levels[0].shape[:2]
    uv, lod, ddx, ddy = S.texture_queries(w, h, len(levels))
    osc = O.OracleScene(S.texture_scene(levels, srgb))
    got0 = osc.texture_probe(0, uv)
    gotl = osc.texture_lod(0, uv, lod)
    gotg = osc.texture_grad(0, uv, ddx, ddy)
    fin = np.isfinite(uv).all(axis=1) & (np.abs(uv).max(axis=1) < 1e5)   # beyond: one ulp of uv spans texels (checked by the band anyway)
    # NaN / inf coordinates: NaN weights (no texel index outside the level: the probe ran)
    assert np.isnan(got0[~np.isfinite(uv).all(axis=1)]).all()
    for label, got, fn, args in (("lod0", got0, lambda a: R.bilinear(levels[0], srgb, a), (uv,)),
                                 ("lod", gotl, lambda a, l: R.texture_lod(levels, srgb, a, l), (uv, lod)),
                                 ("grad", gotg, lambda a, x, y: R.texture_grad(levels, srgb, a, x, y), (uv, ddx, ddy))):
        sel = fin & (np.isfinite(ddx).all(axis=1) & np.isfinite(ddy).all(axis=1) & (np.abs(ddx).max(axis=1) < 1e20) if label == "grad" else True)
        a = [np.ascontiguousarray(x[sel]) for x in args]
        lo, hi = R.band(fn, a)
        e = R.band_excess(got[sel], lo, hi, floor=2.0 ** -24)
        _report("texture %s %s" % (label, name), e)
        assert np.max(e) <= TEXTURE_ULPS, (label, np.argmax(e))
