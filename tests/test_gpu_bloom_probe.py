"""The bloom kernels of csrc/bloom.h on arrays no rendered frame supplies (tests/device_probes/bloom_probe.hip runs the library's launch
sequence on them): sizes around every edge the kernels have -- one texel, one row, one column, the LDS tile's edge, the tail's capacity --
impulses, values over twenty octaves, and texels with NaN, infinities, negative colour and alpha outside [0, 1]. Both forms of level 1
(one thread per texel; the LDS tile) and both forms of the chain (one launch per level; the one-workgroup tail) must equal the numpy
restatement (tests/bloom_ref.py) and each other bit for bit, also when a block cap of 1 or 2 makes every grid-stride loop take many trips."""
import numpy as np
import pytest

import bloom_ref as R
from device_probes import bloom as probe

pytestmark = pytest.mark.gpu
F = np.float32
FORMS = [(False, False), (True, False), (False, True), (True, True)]      # (tile, tail)


def _constants():
    return probe.constants()


def _image(W, H, seed):
    """log-uniform values from 2^-8 to 2^12, an impulse in each corner and the centre, and the texels a prefilter must drop or clamp"""
    rng = np.random.default_rng(seed)
    src = np.exp2(rng.uniform(-8, 12, (H, W, 4))).astype(F)
    src[..., 3] = 1
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        src[y, x, :3] = (3000.0, 1500.0, 750.0)
    special = [(np.nan, 1, 1, 1), (1, np.nan, 1, 1), (np.inf, 1, 1, 1), (1, 1, -np.inf, 1), (-4, 8, -0.0, 1), (-1, -2, -3, 1), (8, 8, 8, -1.0), (8, 8, 8, -np.inf),
               (8, 8, 8, np.nan), (8, 8, 8, 7.5), (8, 8, 8, -0.0), (3e38, 3e38, 1, 1), (1e-40, 0, 0, 1), (0, 0, 0, 1), (1e6, 2e5, 1e5, 1)]
    n = W * H
    if n >= 4 * len(special):
        flat = src.reshape(-1, 4)
        at = rng.choice(np.arange(1, n - 1), len(special), replace=False)
        for k, row in zip(at, special):
            flat[k] = row
    fb = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    return src, fb


def _compare(src, fb, fields, scale, what, forms=FORMS, caps=(2048,), from_state=False):
    d, u, img = R.bloom(src, fb, scale, **fields)
    p = probe.params(**fields)
    starts = set()
    for tile, tail in forms:
        for cap in caps:
            gd, gu, gimg, t0 = probe.run(src, fb, p, scale=scale, from_state=from_state, tile=tile, tail=tail, max_blocks=cap)
            tag = "%s tile %d tail %d cap %d" % (what, tile, tail, cap)
            assert sorted(gd) == sorted(d), tag
            for l in d:
                assert R.same_bits(gd[l], d[l]), (tag, "d(%d)" % l, int(np.count_nonzero(gd[l].view(np.uint32) != d[l].view(np.uint32))))
                assert R.same_bits(gu[l], u[l]), (tag, "u(%d)" % l, int(np.count_nonzero(gu[l].view(np.uint32) != u[l].view(np.uint32))))
            assert np.array_equal(gimg, img), (tag, int(np.count_nonzero(gimg != img)))
            if tail:
                starts.add(t0)
    return d, (starts.pop() if len(starts) == 1 else None)


SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 4), (64, 1), (65, 33), (127, 129)]


@pytest.mark.parametrize("W,H", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_small_and_odd_sizes(W, H):
    src, fb = _image(W, H, 10 + W + H)
    l_max = len(R.sizes(W, H)) - 1
    for fields in (dict(), dict(levels=12, scatter=1.0, threshold=0.0, knee=0.0, tone_mapping_mode=1), dict(levels=1, intensity=1.0, clamp=4.0)):
        d, t0 = _compare(src, fb, fields, 0.5, "%dx%d %s" % (W, H, fields))
        whole = ((W + 1) // 2) * ((H + 1) // 2) <= _constants()["tail_texels"]
        assert t0 == (1 if whole else 2), (W, H, t0)                    # all but 127 x 129: the whole pyramid lies in the tail
        assert len(d) == R.level_count(W, H, fields.get("levels", 0)) <= l_max


def test_sizes_around_the_tile_edge():
    """level 1 one texel below, at and above one tile and two tiles per axis: source sizes 2 t - 1 .. 2 t + 1 give level-1 sizes t and t + 1,
    2 t - 3, 2 t - 2 give t - 1"""
    c = _constants()
    t = c["tile"]
    assert c["tile_src"] == 2 * t + 2
    seen = set()
    for W, H in ((2 * t - 2, 2 * t + 1), (2 * t, 2 * t - 3), (2 * t + 1, 2 * t), (4 * t - 2, 3), (4 * t, 2 * t + 2), (4 * t + 1, 4 * t + 2)):
        src, fb = _image(W, H, W * 131 + H)
        d, _ = _compare(src, fb, dict(threshold=0.5, tone_mapping_mode=2), 2.0, "%dx%d" % (W, H), caps=(2048, 1))
        seen.add(d[1].shape[1])
        seen.add(d[1].shape[0])
    assert {t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1} <= seen, seen


def test_sizes_around_the_tail_capacity():
    """level 1 with one texel fewer than, exactly, and one more than RP_BLOOM_TAIL_TEXELS (as a row, and as a rectangle): the tail starts at
    level 1, 1 and 2; a size whose tail starts at level 3"""
    c = _constants()
    cap = c["tail_texels"]
    rows = 32
    assert cap % rows == 0
    wide = cap // rows
    cases = [((2 * (cap - 1), 1), 1), ((2 * cap, 1), 1), ((2 * cap + 1, 1), 2), ((2 * wide, 2 * rows), 1), ((2 * wide + 1, 2 * rows), 2), ((2 * wide, 2 * rows - 3), 1),
             ((8 * wide - 3, 8 * rows + 5), 4), ((4 * wide + 2, 4 * rows), 3)]
    for (W, H), want_start in cases:
        src, fb = _image(W, H, W + 7 * H)
        sizes = R.sizes(W, H)
        first_fit = next(l for l in range(1, len(sizes)) if sizes[l][0] * sizes[l][1] <= cap)
        assert first_fit == want_start, ((W, H), first_fit)
        d, t0 = _compare(src, fb, dict(levels=12, threshold=0.25, scatter=0.9), 1.0, "%dx%d" % (W, H))
        assert t0 == want_start, ((W, H), t0)
        assert len(d) >= want_start + 2


def test_block_caps_of_one_and_two_make_the_loops_take_many_trips():
    """127 x 129: level 1 is 64 x 65 = 4160 texels, 17 blocks' worth, and 4 x 5 = 20 tiles; the composite has 16383 pixels, 64 blocks' worth"""
    src, fb = _image(127, 129, 3)
    _compare(src, fb, dict(levels=12, white_balance=(1.2, 1.0, 0.8)), 1.0, "127x129 capped", caps=(1, 2))
    src, fb = _image(300, 70, 4)                                         # level 1 is 150 x 35, more than the tail takes: a capped level 1 and a capped up step
    d, t0 = _compare(src, fb, dict(), 1.0, "300x70 capped", caps=(1, 2, 3))
    assert t0 == 2


def test_impulses_and_the_scale_read_from_a_device_state():
    W, H = 65, 33
    src = np.zeros((H, W, 4), F)
    src[..., 3] = 1
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        src[y, x, :3] = (40.0, 20.0, 10.0)
    fb = np.zeros((H, W, 4), np.uint8)
    fields = dict(levels=12, threshold=0.0, knee=0.0, clamp=64.0, scatter=1.0, intensity=1.0)
    d, _ = _compare(src, fb, fields, 0.75, "impulses")
    assert (d[7][0, 0, :3] > 0).all() and d[7].shape == (1, 1, 4)
    _compare(src, fb, fields, 0.75, "impulses, scale from the state", from_state=True)
    srcr, fbr = _image(W, H, 9)
    _compare(srcr, fbr, dict(tone_mapping_mode=1), F(2.0) ** F(-3.5), "random, scale from the state", from_state=True)
