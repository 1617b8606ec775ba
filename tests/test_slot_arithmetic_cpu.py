"""The integer restatement of the slot and index arithmetic (tests/slot_ref.py) and its cases, on the CPU: the magic-number division rule
is exact for every case with n < 2^31 on Python integers, the restated tile mapping is a bijection between a frame's pixels and its
non-padding slots, the ranks' rows partition the frame, and the cases reach the edges tests/test_gpu_slot_arithmetic.py relies on."""
import numpy as np
import pytest

import slot_ref as SR


def test_division_rule_is_exact_below_2_31():
    n, d = SR.div_cases()
    assert len(n) <= 2 ** 17 and int(n.max()) == 2 ** 31 - 1 and int(d.max()) == 2 ** 30 + 1
    ds = set(int(x) for x in d)
    assert set(range(1, 1026)) <= ds and {1920 * 1, 3840, 7680, 2 ** 11 - 1, 2 ** 30} <= ds and set(SR.frame_divisors()) <= ds
    for nn, dd in zip(n.tolist(), d.tolist()):
        assert SR.div_by_rule(nn, dd) == nn // dd, (nn, dd)
    # every divisor meets a multiple of itself, the numbers around it and the largest numerator
    for dd in (1, 2, 3, 1025, 2 ** 30 + 1, 7680):
        mine = set(n[d == dd].tolist())
        assert {0, dd, 2 ** 31 - 1} <= mine and ((2 ** 31 - 1) // dd) * dd in mine
    # the comment's claim has an edge: beyond 2^31 the rule may be wrong, which is why every caller stays below
    assert any(SR.div_by_rule(nn, dd) != nn // dd for dd in (3, 5, 7, 641) for nn in range(2 ** 32 - 4 * dd, 2 ** 32))


@pytest.mark.parametrize("frame", SR.SMALL_FRAMES, ids=["%dx%d" % f for f in SR.SMALL_FRAMES])
def test_restated_tile_mapping_is_a_bijection(frame):
    w, h = frame
    for world in SR.WORLDS:
        for sr in SR.STRIPE_ROWS:
            seen_rows = []
            for rank in range(world):
                rows, tx, ty, npix = SR.geometry(w, h, rank, world, sr)
                slots, pix = SR.slot_cases(w, h, rank, world, sr)
                assert len(slots) == npix and len(pix) == w * rows and npix % 256 == 0
                lx, ly, ok = SR.slot_to_local(w, rows, tx, slots)
                assert ok.sum() == w * rows
                assert len(np.unique(ly[ok] * w + lx[ok])) == w * rows                       # every pixel once
                assert np.array_equal(SR.local_to_slot(tx, lx[ok], ly[ok]), slots[ok])       # round trip
                assert np.array_equal(np.sort(SR.local_to_slot(tx, pix[:, 0], pix[:, 1])), slots[ok].astype(np.int64))
                seen_rows.append(SR.local_row_to_global(rank, world, sr, np.arange(rows)))
            assert np.array_equal(np.sort(np.concatenate(seen_rows)), np.arange(h)), (world, sr)


def test_cases_reach_the_edges():
    # a frame smaller than a tile, sizes that are no multiple of 8 or 16, ranks without rows, more than 2^24 slots
    assert SR.geometry(1, 1) == (1, 2, 2, 256)
    assert SR.geometry(17, 33, 7, 8, 8)[0] == 0 and SR.geometry(17, 33, 7, 8, 8)[3] == 4 * 2 * 64
    assert SR.geometry(7680, 4320)[3] == 7680 * 4320 > 2 ** 24
    slots, pix = SR.slot_cases(3840, 2160, 0, 1, 32)
    assert len(slots) >= 4 * (3840 // 16) * (2160 // 16) and int(slots.max()) == SR.geometry(3840, 2160)[3] - 1
    # reset and continued batches, more than one frame, wrapping frame constants
    kinds = {(c[0] > 1, bool(c[2])) for c in SR.SLOT_FRAME_CASES}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    assert any(c[3] + c[4] + c[0] * c[1] >= 2 ** 32 for c in SR.SLOT_FRAME_CASES)
    out = SR.slot_frame(3, 5, 1, 77, 10, 10, np.arange(15))
    assert out[4].tolist() == [0, 14, 77, 10] and out[5].tolist() == [1, 0, 92, 0] and out[14].tolist() == [2, 4, 97, 0]
    out = SR.slot_frame(3, 5, 0, 77, 10, 10, np.arange(15))
    assert out[5].tolist() == [1, 15, 77, 15] and out[14].tolist() == [2, 24, 77, 20]
