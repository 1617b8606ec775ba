"""The binned light selection on the CPU, before any GPU run: the case generators of tests/shade_cases.py reach the edges the device test
(tests/test_gpu_light_selection.py) relies on, and the oracle's sample_tri_lights (orc_tri_light_bins) agrees with the float64 restatement
(tests/shade_ref64.py light_bin / light_contributions / light_select / light_dist_wpdf).

Bounds, with the values measured on the oracle:
  bin [begin, end)           equal to the integer rule on every query
  contributions              |c - float64| <= luminance * (2 * 1.16e-5 + 2e-6) + 4 ulps on lights whose facing tests have a margin and whose
                             triangle is well conditioned (measured 2.27e-5 of the luminance)
  chosen light               the selection rule in binary32 on the oracle's contributions names the oracle's light on EVERY query; the rule
                             in float64 names it on every query whose sel.y is not one of the chosen edge values
  pdf                        relative 4e-3 of 1 / (bins * omega) * p on well-conditioned chosen lights of omega >= 0.01 sr (measured 1.4e-4; the bound:
                             twice the arctangent's 1.16e-5 over 0.01 sr)
  light_dist, mis_wpdf       band excess over the float64 formula at the oracle's own direction, in rounding units (a worst-case envelope
                             of the formula's own roundings, tens of ulps of the result on a typical query:
                             shade_ref64.light_dist_wpdf_excess) <= shade_ref64.ORACLE_DIST_EXCESS / ORACLE_WPDF_EXCESS (measured 0.179 /
                             0.157 units; in plain ulps of the result 158.1 / 228.1, both on single grazing queries); the device test
                             derives its bounds from these two
"""
import numpy as np
import pytest

import shade_cases as S
import shade_ref64 as R

CASES = [(n, b) for n in S.LIGHT_TABLE_SIZES for b in S.LIGHT_BIN_SIZES]
CONTRIB_REL = 2 * R.FAST_ATAN_MAX_ABS_ERROR + 2e-6   # tests/test_shade_ref64.py: the solid angle's bound
PDF_REL = 4e-3


def chosen_light(case, out):
    return out["bins"][:, 2].astype(np.int64)


def fall_through_kinds(case):
    """per query: 0 none, 1 through a full bin of BIN_MAX lights (the walk ends ON the last light), 2 through the table's last, partial
    bin (ends on the zeroed record behind the table), 3 through a shorter bin in the middle (ends on the next bin's first light)"""
    ref, u4 = case["ref"], case["u4"]
    begin, end, light = (ref["bins"][:, k].astype(np.int64) for k in range(3))
    count = end - begin
    _, _, sums = R.light_select(ref["contrib"], count, u4[:, 3], np.float32)
    last = sums[np.arange(len(sums)), count - 1]
    through = ~np.isnan(last) & ~(u4[:, 3] < last)   # (NaN: the walk ended before the bin's last light)
    kind = np.zeros(len(u4), np.int64)
    kind[through & (count == R.BIN_MAX)] = 1
    kind[through & (count < R.BIN_MAX) & (end == len(case["table"]))] = 2
    kind[through & (count < R.BIN_MAX) & (end < len(case["table"]))] = 3
    assert (light[kind == 1] == end[kind == 1] - 1).all() and (light[kind >= 2] == end[kind >= 2]).all()
    return kind


def test_generators_reach_the_edges():
    kinds_seen, dark_seen, nan_seen = set(), 0, 0
    for (n, b) in CASES:
        case = S.light_case(n, b)
        ref, u4 = case["ref"], case["u4"]
        bins = (n + b - 1) // b
        assert 4000 <= len(u4) <= 8192 and ((u4[:, 3] >= 1 - 2.0 ** -24).sum() <= 4 <= 1e-3 * len(u4))
        # every light of the table has its own radiance
        assert len(np.unique(case["table"][:, 3], axis=0)) == n
        # every bin is chosen, by the edge values and by random ones
        assert set(np.unique(ref["bins"][:, 0] // b)) == set(range(bins)), (n, b)
        assert set(np.unique(ref["bins"][case["boundary"], 0] // b)) == set(range(bins)), (n, b)
        kinds_seen |= set(np.unique(fall_through_kinds(case)))
        # every light back-facing or below the horizon: all contributions of the bin are MIN_IRRADIANCE
        dark = case["kinds"] == "dark"
        count = (ref["bins"][:, 1] - ref["bins"][:, 0])[dark]
        c = ref["contrib"][dark]
        inside = np.arange(16)[None, :] < count[:, None]
        assert dark.any() and (c[inside] == np.float32(6.2e-4) * np.float32(0.001)).all() and (c[~inside] == 0).all()
        dark_seen += int(dark.sum())
        for k in ("plane", "vertex", "far", "near"):
            assert (case["kinds"] == k).any(), (n, b, k)
        # a receiver on a vertex of the chosen light gives a direction of NaN (normalize(0)): the device test compares NaN == NaN
        nan_seen += int(np.isnan(ref["dir"][case["kinds"] == "vertex"]).any(axis=1).sum())
    assert kinds_seen == {0, 1, 2, 3}, kinds_seen
    assert dark_seen > 0 and nan_seen > 0


ULP_LIBM, EXCEPTIONS = 64, 1e-3   # tests/shade_probes.py (which loads the device probes: not imported here)


@pytest.mark.parametrize("n,b", CASES)
def test_direction_samples_are_well_conditioned_on_all_but_a_few_queries(n, b):
    """The device test holds light_dir within ULP_LIBM ulps of the oracle's on all but EXCEPTIONS of the queries. Whether a query can
    keep such a bound is a property of the query: where one ulp of the direction sample moves the ORACLE's own direction by more than the
    bound (lights of 1e-4 sr: the far and the dark receivers), one ulp of the device's cosf / sinf does as well. The cases hold such
    queries below 10 * EXCEPTIONS (measured: 0.14 % .. 0.64 %); a device differs there through the last bit of two library calls, less
    often than a whole ulp of both samples in both directions moves the direction, so the device test's rule is decided by the code,
    not by the cases."""
    case = S.light_case(n, b)
    u, ref = case["u4"], case["ref"]
    moved = np.zeros(len(u))
    for toward in (2.0, -2.0):
        v = np.array(u)
        v[:, :2] = np.clip(np.nextafter(u[:, :2], np.float32(toward)), 0.0, 1.0)
        out = S.oracle_tri_light_bins(case["table"], b, case["p"], case["n"], np.ascontiguousarray(v, np.float32))
        a, r = out["dir"].astype(np.float64), ref["dir"].astype(np.float64)
        with np.errstate(invalid="ignore"):
            moved = np.fmax(moved, np.nan_to_num(np.abs(a - r).max(axis=1)) / 2.0 ** -24)
    share = (moved > ULP_LIBM).mean()
    print("lights %2d bins of %2d: %.3f %% of %d queries move by more than %d ulps under one ulp of the direction sample" % (n, b, 100 * share, len(u), ULP_LIBM))
    assert share <= 10 * EXCEPTIONS


@pytest.mark.parametrize("n,b", CASES)
def test_oracle_light_selection_against_float64(n, b):
    case = S.light_case(n, b)
    ref, u4, table, p, nn = case["ref"], case["u4"], case["table"], case["p"], case["n"]
    # the bin: the integer rule
    begin, end, bins = R.light_bin(n, b, u4[:, 2])
    assert np.array_equal(begin, ref["bins"][:, 0]) and np.array_equal(end, ref["bins"][:, 1])
    count = end - begin
    # the contributions
    c64, decided = R.light_contributions(table, begin, end, p, nn)
    lights = R.pad_lights(table)
    idx = np.minimum(begin[:, None] + np.arange(16)[None, :], len(lights) - 1)
    v9 = (lights[idx][:, :, :3, :] - p.astype(np.float64)[:, None, None, :]).reshape(-1, 9)
    exact = R.tri_solid_angle(v9)
    d = v9.reshape(-1, 3, 3) / np.maximum(np.linalg.norm(v9.reshape(-1, 3, 3), axis=2, keepdims=True), 1e-300)
    sep = np.min([np.linalg.norm(d[:, i] - d[:, j], axis=1) for i, j in ((0, 1), (1, 2), (0, 2))], axis=0)
    well = ((exact > 1e-4) & (exact < 2.0) & (sep > 1e-2)).reshape(idx.shape) & decided
    lum = R._lum(lights[idx][:, :, 3])
    err = np.abs(ref["contrib"].astype(np.float64) - c64)
    bound = lum * CONTRIB_REL + 4 * R.ulp32(c64)
    lit = well & (lum > 0)
    print("lights %2d bins of %2d: %6d contributions held, max error / luminance %.2e" % (n, b, well.sum(), (err[lit] / lum[lit]).max() if lit.any() else 0))
    assert (err[well] <= bound[well]).all()
    assert (ref["contrib"][np.arange(16)[None, :] >= count[:, None]] == 0).all()
    # the selection: in binary32 on the oracle's own contributions exactly; in float64 wherever sel.y is no chosen edge value
    light = chosen_light(case, ref)
    pick32, p32, sums32 = R.light_select(ref["contrib"], count, u4[:, 3], np.float32)
    assert np.array_equal(begin + pick32, light)
    pick64, p64, sums64 = R.light_select(ref["contrib"], count, u4[:, 3], np.float64)
    differ = (begin + pick64) != light
    assert not (differ & ~case["boundary"]).any(), np.where(differ & ~case["boundary"])[0][:8]
    # ... and no other query sits within 4 ulps of a running sum (what the fast_math rule of the device test excuses)
    with np.errstate(invalid="ignore"):
        close = (np.abs(sums32 - u4[:, 3:4].astype(np.float64)) <= 4 * 2.0 ** -24).any(axis=1)
    assert not (close & ~case["boundary"]).any()
    # pdf = 1 / omega * p / bins on well-conditioned chosen lights
    at = (np.arange(len(u4)), np.minimum(pick32, 15))
    sel = well[at] & (pick32 < count) & (exact.reshape(idx.shape)[at] >= 1e-2)
    want = p64 / (bins * exact.reshape(idx.shape)[at])
    rel = np.abs(ref["pdf"].astype(np.float64) - want)[sel] / want[sel]
    print("    pdf: %d held, max relative error %.2e" % (sel.sum(), rel.max() if sel.any() else 0))
    assert (rel <= PDF_REL).all()
    # radiance_over_pdf * pdf names the light
    fin = np.isfinite(ref["L"]).all(axis=1) & np.isfinite(ref["pdf"]) & (ref["pdf"] > 0)
    named = R.name_light(table, ref["L"], ref["pdf"])
    rad = lights[:, 3]
    assert fin.sum() > 0.5 * len(u4) and (np.abs(rad[named[fin]] - rad[light[fin]]).max(axis=1) == 0).all()
    # light_dist / mis_wpdf against the float64 formula at the oracle's own direction
    ed, ew, pd, pw = R.light_dist_wpdf_excess(table, bins, p, light, ref["dir"], ref["dist"], ref["mis"])
    print("    light_dist excess %.3f units (%.1f ulps of the result), mis_wpdf excess %.3f units (%.1f ulps)" % (ed.max(), pd.max(), ew.max(), pw.max()))
    assert ed.max() <= R.ORACLE_DIST_EXCESS and ew.max() <= R.ORACLE_WPDF_EXCESS


def test_oracle_scene_without_lights_ignores_the_sun_weight():
    """the oracle's frame setup sends every NEE sample of a light-less scene to the sun (as the library's does: tests/test_gpu_parity.py
    test_scene_without_lights_ignores_the_sun_weight): sun_radiance[3] = 0.5 gives the bits of 1.0, and finite ones"""
    import oracle_lib as O
    from realtimepathtracingresearchframework_amd import abi, scenes
    s = scenes.cornell32()
    s.lights = np.zeros((0, 4, 3), np.float32)
    out = []
    for w in (1.0, 0.5):
        sp = s.scene_params()
        sp.sun_radiance[3] = w
        out.append(O.OracleScene(s).render(48, 32, 2, variant=abi.VARIANT_GLTF, scene_params=sp)[0])
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)) and np.isfinite(out[1]).all()


def test_oracle_light_probe_refuses_an_empty_table():
    import ctypes as C
    import oracle_lib as O
    from realtimepathtracingresearchframework_amd import abi, scenes
    s = scenes.cornell32()
    s.lights = np.zeros((0, 4, 3), np.float32)
    osc = O.OracleScene(s)
    fn = O.lib().orc_tri_light_bins
    fn.argtypes, fn.restype = None, C.c_int
    z = np.zeros(16, np.float32)
    cfg = abi.LightSamplingConfig(0.0, 16, 15.0, 0.0)
    assert fn(C.c_void_p(osc.h), C.byref(cfg), O._p(z), O._p(z), O._p(z), 1, O._p(z), O._p(z), O._p(z), O._p(z), O._p(z), O._p(z.view(np.int32)), O._p(z)) == -1
    osc.close()
