"""The device's slot and index arithmetic (csrc/dshade.h rp_div with rp_make_div, rp_slot_to_local, rp_local_to_slot,
rp_local_row_to_global, rp_slot_frame through the sp_div, sp_slots and sp_slot_frame probes) against the integer restatement of
tests/slot_ref.py, in both builds (integer code: the builds must not differ).

rp_div == n // d on every case with n < 2^31 (the exactness the comment of RpDivU32 claims); over frames from 1 x 1 to 8K, worlds of 1,
2, 3 and 8 ranks (every rank) and stripes of 1, 5, 8 and 32 rows: the slot of a pixel and the pixel of a slot invert each other, every
local pixel is hit exactly once, padding slots report false, a local row's frame row equals the formula, the ranks' rows partition
[0, height); rp_slot_frame equals the restatement for reset and continued batches. Small frames exhaustively, 1080p / 4K / 8K on the four
corners of every block of tiles, random slots and the first pixel of every row. No array handed to a probe exceeds 2^17 elements."""
import ctypes as C

import numpy as np
import pytest

import slot_ref as SR
from oracle_lib import _p
from shade_probes import call

pytestmark = pytest.mark.gpu


class Geometry(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "rank", "world", "stripe_rows")]


def test_division_by_frame_constants():
    n, d = SR.div_cases()
    assert len(n) <= SR.MAX_ARRAY and int(n.max()) < 2 ** 31
    want = (n.astype(np.int64) // d.astype(np.int64)).astype(np.uint32)
    for fast in (0, 1):
        q = np.zeros(len(n), np.uint32)
        call(fast, "sp_div", _p(n), _p(d), len(n), _p(q))
        bad = q != want
        print("rp_div %-5s %d cases over %d divisors, largest divisor %d: %d wrong" % (("ieee", "fast")[fast], len(n), len(np.unique(d)), d.max(), bad.sum()))
        assert not bad.any(), (n[bad][:8], d[bad][:8], q[bad][:8])


def device_slots(fast, g, slots, pix):
    """rp_slot_to_local of the slots, rp_local_to_slot / rp_local_row_to_global of the pixels, in calls of at most MAX_ARRAY elements"""
    local = np.zeros((len(slots), 3), np.int32)
    slot_of, grow = np.zeros(len(pix), np.uint32), np.zeros(len(pix), np.int32)
    step = SR.MAX_ARRAY // 3
    for a in range(0, max(len(slots), len(pix)), step):
        s, p = np.ascontiguousarray(slots[a:a + step]), np.ascontiguousarray(pix[a:a + step])
        l3, so, gr = np.zeros((len(s), 3), np.int32), np.zeros(len(p), np.uint32), np.zeros(len(p), np.int32)
        call(fast, "sp_slots", C.byref(g), _p(s), len(s), _p(l3), _p(p), len(p), _p(so), _p(gr))
        local[a:a + step], slot_of[a:a + step], grow[a:a + step] = l3, so, gr
    return local, slot_of, grow


@pytest.mark.parametrize("frame", SR.FRAMES, ids=["%dx%d" % f for f in SR.FRAMES])
def test_slots_and_pixels(frame):
    w, h = frame
    small = frame in SR.SMALL_FRAMES
    checked = 0
    for world in SR.WORLDS:
        for sr in SR.STRIPE_ROWS:
            rows_of_ranks = {0: [], 1: []}
            for rank in range(world):
                g = Geometry(w, h, rank, world, sr)
                rows, tx, ty, npix = SR.geometry(w, h, rank, world, sr)
                slots, pix = SR.slot_cases(w, h, rank, world, sr)
                lx, ly, ok = SR.slot_to_local(w, rows, tx, slots)
                for fast in (0, 1):
                    geo = np.zeros(4, np.int32)
                    call(fast, "sp_slot_geometry", C.byref(g), _p(geo))
                    assert geo.tolist() == [rows, tx, ty, npix]
                    local, slot_of, grow = device_slots(fast, g, slots, pix)
                    # slot -> pixel: the restatement's pixel; padding slots report false
                    assert np.array_equal(local[:, 2] != 0, ok), (world, sr, rank)
                    assert np.array_equal(local[:, 0], lx) and np.array_equal(local[:, 1], ly), (world, sr, rank)
                    # pixel -> slot: the restatement's slot, and back to the pixel on the device itself
                    assert np.array_equal(slot_of.astype(np.int64), SR.local_to_slot(tx, pix[:, 0], pix[:, 1])), (world, sr, rank)
                    back, _, _ = device_slots(fast, g, slot_of, pix[:0])
                    assert (back[:, 2] == 1).all() and np.array_equal(back[:, :2], pix), (world, sr, rank)
                    # slot -> pixel -> slot wherever the pixel exists
                    _, again, _ = device_slots(fast, g, slots[:0], np.ascontiguousarray(local[ok, :2]))
                    assert np.array_equal(again, slots[ok]), (world, sr, rank)
                    if small:   # every local pixel is hit exactly once
                        assert len(slots) == npix and ok.sum() == w * rows and len(np.unique(local[ok, 1].astype(np.int64) * w + local[ok, 0])) == w * rows
                    # local row -> frame row
                    assert np.array_equal(grow.astype(np.int64), SR.local_row_to_global(rank, world, sr, pix[:, 1])), (world, sr, rank)
                    first = np.unique(pix[:, 1][pix[:, 0] == 0], return_index=True)[1]
                    rows_of_ranks[fast].append(grow[pix[:, 0] == 0][first])
                    checked += len(slots) + len(pix)
            # over the ranks of the world the rows partition [0, height)
            for fast, got in rows_of_ranks.items():
                if got:
                    assert np.array_equal(np.sort(np.concatenate(got)), np.arange(h)), (world, sr, fast)
    print("slots %dx%d: %d slots and pixels over %d worlds x %d stripe heights, every rank" % (w, h, checked, len(SR.WORLDS), len(SR.STRIPE_ROWS)))


def test_slot_frame():
    for case in SR.SLOT_FRAME_CASES:
        frames, spp, reset, fo, sb, fi = case
        sslots = np.arange(frames * spp, dtype=np.uint32)
        want = SR.slot_frame(frames, spp, reset, fo, sb, fi, sslots)
        for fast in (0, 1):
            out = np.zeros((len(sslots), 4), np.uint32)
            call(fast, "sp_slot_frame", frames, spp, reset, fo, sb, fi, _p(sslots), len(sslots), _p(out))
            assert np.array_equal(out, want), (case, out[:4], want[:4])
    print("rp_slot_frame: %d batches, reset and continued" % len(SR.SLOT_FRAME_CASES))
