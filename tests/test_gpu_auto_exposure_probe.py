"""The meter kernels of csrc/auto_exposure.h on an array no rendered frame supplies (tests/device_probes/exposure_probe.hip runs
rp_k_meter and rp_k_meter_reduce on it): NaN, infinities, negatives, negative alpha, denormals, every power of two from 2^-17 to 2^17 with
both float neighbours, a run of 1024 equal values; 4099 texels, no multiple of 256 or of 4. Histogram, counts and state must equal the
numpy restatement (tests/auto_exposure_ref.py) exactly."""
import numpy as np
import pytest

import auto_exposure_ref as A
from device_probes import exposure as probe

pytestmark = pytest.mark.gpu
F = np.float32
N = 4099


def _texels():
    rng = np.random.default_rng(5)
    t = np.zeros((N, 4), F)
    t[:, 3] = 1
    lum = np.exp2(rng.uniform(-20, 18, N)).astype(F)                 # below bin 1 and above bin 255 included
    t[:, 0] = t[:, 1] = t[:, 2] = lum
    k = 0
    for e in range(-17, 18):                                           # green alone: lum = 0.7152 g; and grey, lum ~ g
        p = F(2.0) ** F(e)
        for v in (np.nextafter(p, F(0)), p, np.nextafter(p, F(np.inf))):
            t[k, :3] = (0, v, 0)
            t[k + 1, :3] = (v, v, v)
            k += 2
    assert k == 210
    special = [(np.nan, 0, 0, 1), (0, np.nan, 0, 1), (np.inf, 0, 0, 1), (-np.inf, 0, 0, 1), (np.inf, -np.inf, 0, 1), (-1, -1, -1, 1), (-1e-30, 0, 0, 1),
               (0.5, 0.5, 0.5, -1), (0.5, 0.5, 0.5, -0.0), (0.5, 0.5, 0.5, np.nan), (0.5, 0.5, 0.5, -np.inf), (0, 0, 0, 1), (-0.0, -0.0, -0.0, 1),
               (1e-40, 1e-40, 1e-40, 1), (1e-45, 0, 0, 1), (3e38, 3e38, 3e38, 1), (3.4e38, 3.4e38, 3.4e38, 1), (1, -0.29720357, 0, 1), (0.18, 0.18, 0.18, 1)]
    for row in special:
        t[k] = row
        k += 1
    t[1500:1500 + 1024, :3] = (0.25, 0.5, 0.125)                       # sixteen waves of one value: 64 same-address LDS atomics each
    t[N - 3:, :3] = (7.0, 7.0, 7.0)                                     # the tail: the last block's three lanes
    return t


TEXELS = _texels()


def _compare(got, after, want, what):
    g = A.state_of(got)
    bad = A.same_state(g, want)
    print("%s: counted %d black %d ignored %d ev %.6f mean %.6f scale %.6f %s" % (what, g["counted"], g["black"], g["ignored"], g["ev"], g["mean_log2"], g["scale"], bad))
    assert not bad, (what, bad)
    assert not after.any(), what                                        # the reduce kernel cleared the working histogram


@pytest.mark.parametrize("blocks", [1, 3, 17, 64], ids=lambda b: "blocks%d" % b)
def test_the_meter_on_chosen_texels_equals_the_restatement(blocks):
    """1 block: seventeen rounds of the grid-stride loop, the last with three lanes; 17 blocks: one round, the last block three lanes;
    64 blocks: most have nothing to do and add nothing"""
    hist, counted, black, ignored = A.meter(TEXELS)
    assert counted + black + ignored == N and ignored == 9 and black >= 5 and hist[255] > 0 and hist[1] > 0
    assert np.count_nonzero(hist) > 200                                 # nearly every bin is hit
    for fields in (dict(), dict(low_percentile=0.0, high_percentile=1.0), dict(low_percentile=0.1, high_percentile=0.100001), dict(key=1.0, min_ev=-0.5, max_ev=0.5)):
        p = probe.params(**fields)
        want = A.step(TEXELS, fields, None, exposure=0.25)
        for combine in (False, True):                                   # the library's instantiation, and the one with the wave-combine step
            got, after = probe.meter(TEXELS, p, exposure=0.25, blocks=blocks, combine=combine)
            _compare(got, after, want, "blocks %d combine %d %s" % (blocks, combine, fields))


def test_the_combining_meter_counts_what_the_plain_one_counts():
    """rp_k_meter<true> (lanes of a wave with the same bin share one LDS atomic; kept for the timing comparison) gives the same histogram"""
    p = probe.params()
    a, _ = probe.meter(TEXELS, p, blocks=5, combine=True)
    b, _ = probe.meter(TEXELS, p, blocks=5, combine=False)
    assert not A.same_state(A.state_of(a), A.state_of(b))


def test_a_state_carried_in_adapts_and_an_all_black_array_keeps_it():
    fields = dict(dt=0.25, speed_up=0.5, speed_down=4.0)
    first, _ = probe.meter(TEXELS, probe.params(**fields), blocks=4)
    want0 = A.step(TEXELS, fields, None)
    _compare(first, np.zeros(1, np.uint32), want0, "first")
    with np.errstate(all="ignore"):
        dark, bright = TEXELS * F(1 / 64), TEXELS * F(16)
    for name, src in (("darker", dark), ("brighter", bright)):
        src[:, 3] = TEXELS[:, 3]
        got, after = probe.meter(src, probe.params(**fields), blocks=4, state_in=first)
        want = A.step(src, fields, want0)
        _compare(got, after, want, name)
        assert want["calls"] == 2 and want["ev"] != want["target_ev"]
    got, after = probe.meter(src, probe.params(reset_history=1, **fields), blocks=4, state_in=first)
    _compare(got, after, A.step(src, dict(fields, reset_history=1), want0), "reset")
    black = np.zeros((N, 4), F)
    black[:, 3] = 1
    got, after = probe.meter(black, probe.params(**fields), blocks=4, state_in=first)
    want = A.step(black, fields, want0)
    _compare(got, after, want, "black")
    assert want["ev"] == want0["ev"] and want["counted"] == 0 and want["black"] == N
    got, after = probe.meter(black, probe.params(**fields), blocks=4)
    _compare(got, after, A.step(black, fields, None), "black, no state")
