"""An integer restatement of the slot and index arithmetic of csrc/dshade.h (rp_div / rp_make_div, rp_slot_frame, rp_slot_to_local,
rp_local_to_slot, rp_local_row_to_global) and of the frame geometry rptr_hip_initialize derives -- TEST INFRASTRUCTURE.

Written from what the functions are FOR, on Python / int64 integers with // and %: tiles of 8 x 8 pixels, numbered row-major inside
blocks of TILE_BLOCK x TILE_BLOCK tiles, the blocks row-major over the local image; stripe s of `stripe_rows` rows belongs to rank
s % world. tests/test_slot_arithmetic_cpu.py checks the restatement against itself (round trips, partitions) and the magic-number rule
on Python integers; tests/test_gpu_slot_arithmetic.py holds the device functions to it. The cases live here too."""
import numpy as np

TILE_BLOCK = 2   # RP_TILE_BLOCK


# ---------------------------------------------------------------- the restatement
def make_div(d):
    """the (mul, shift) rule the comment of RpDivU32 states: shift = ceil(log2 d) - 1, mul = ceil(2^(32 + shift) / d); (0, 0) for d = 1"""
    if d <= 1:
        return 0, 0
    shift = (d - 1).bit_length() - 1
    return -((-(1 << (32 + shift))) // d), shift


def div_by_rule(n, d):
    mul, shift = make_div(d)
    return ((n * mul) >> 32) >> shift if mul else n


def local_rows(height, stripe_rows, rank, world):
    stripes = (height + stripe_rows - 1) // stripe_rows
    return sum(min(stripe_rows, height - s * stripe_rows) for s in range(rank, stripes, world))


def geometry(width, height, rank=0, world=1, stripe_rows=32):
    """(local_rows, tiles_x, tiles_y, npix_padded): whole blocks of tiles over width x max(local_rows, 1)"""
    rows = local_rows(height, stripe_rows, rank, world)
    block = 8 * TILE_BLOCK
    tiles_x = (width + block - 1) // block * TILE_BLOCK
    tiles_y = (max(rows, 1) + block - 1) // block * TILE_BLOCK
    return rows, tiles_x, tiles_y, tiles_x * tiles_y * 64


def slot_to_local(width, rows, tiles_x, slot):
    """-> (lx, ly, the pixel exists)"""
    slot = np.asarray(slot, np.int64)
    tile, inside = slot // 64, slot % 64
    blk, t_in = tile // (TILE_BLOCK * TILE_BLOCK), tile % (TILE_BLOCK * TILE_BLOCK)
    blocks_x = tiles_x // TILE_BLOCK
    tx = (blk % blocks_x) * TILE_BLOCK + t_in % TILE_BLOCK
    ty = (blk // blocks_x) * TILE_BLOCK + t_in // TILE_BLOCK
    lx, ly = tx * 8 + inside % 8, ty * 8 + inside // 8
    return lx, ly, (lx < width) & (ly < rows)


def local_to_slot(tiles_x, lx, ly):
    lx, ly = np.asarray(lx, np.int64), np.asarray(ly, np.int64)
    tx, ty = lx // 8, ly // 8
    blk = (ty // TILE_BLOCK) * (tiles_x // TILE_BLOCK) + tx // TILE_BLOCK
    tile = blk * TILE_BLOCK * TILE_BLOCK + (ty % TILE_BLOCK) * TILE_BLOCK + tx % TILE_BLOCK
    return tile * 64 + (ly % 8) * 8 + lx % 8


def local_row_to_global(rank, world, stripe_rows, ly):
    ly = np.asarray(ly, np.int64)
    return ((ly // stripe_rows) * world + rank) * stripe_rows + ly % stripe_rows


def slot_frame(batch_frames, frame_spp, batch_reset, frame_offset, sample_base, frame_id, sslot):
    """-> (N, 4) uint32: frame, sample_index, frame_offset, frame_id of sample slot sslot (begin_frame's rule for the frames behind the
    first: a reset moves frame_offset on by what was accumulated and starts again at sample 0, otherwise frame_id counts on)"""
    s = np.asarray(sslot, np.int64)
    frame = s // frame_spp if batch_frames > 1 else np.zeros_like(s)
    first = frame == 0
    if batch_reset:
        si = np.where(first, sample_base + s, s - frame * frame_spp)
        fo = np.where(first, frame_offset, frame_offset + sample_base + frame * frame_spp)
        fi = np.where(first, frame_id, 0)
    else:
        si, fo, fi = sample_base + s, np.full_like(s, frame_offset), frame_id + frame * frame_spp
    return (np.stack([frame, si, fo, fi], axis=1) % 2 ** 32).astype(np.uint32)


# ---------------------------------------------------------------- cases
FRAMES = ((1, 1), (8, 8), (9, 7), (17, 33), (250, 130), (1920, 1080), (3840, 2160), (7680, 4320))
SMALL_FRAMES, LARGE_FRAMES = FRAMES[:5], FRAMES[5:]
WORLDS = (1, 2, 3, 8)
STRIPE_ROWS = (1, 5, 8, 32)
MAX_ARRAY = 2 ** 17


def frame_divisors():
    """tiles per block row, stripe rows, width and padded pixels of 1080p, 4K and 8K"""
    d = set(STRIPE_ROWS)
    for (w, h) in LARGE_FRAMES:
        for world in WORLDS:
            for sr in STRIPE_ROWS:
                _, tx, _, npix = geometry(w, h, world - 1, world, sr)
                d |= {w, tx // TILE_BLOCK, npix}
    return sorted(d)


def div_cases(seed=30):
    """(n, d) uint32 pairs, n < 2^31: d = 1 .. 1025, 2^k - 1 / 2^k / 2^k + 1 (k = 11 .. 30), the frame constants; per d the numerators 0, 1,
    d - 1, d, d + 1, k d - 1 / k d / k d + 1 for k = 2, 3, 1000, floor((2^31 - 1) / d) and half of it, 2^31 - 1 and 2^31 - 2, eight random"""
    rng = np.random.default_rng(seed)
    ds = set(range(1, 1026)) | set(frame_divisors())
    for k in range(11, 31):
        ds |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    top = 2 ** 31 - 1
    n, d = [], []
    for x in sorted(ds):
        ns = {0, 1, x - 1, x, x + 1, top, top - 1}
        for k in (2, 3, 1000, top // x, top // x // 2):
            ns |= {k * x - 1, k * x, k * x + 1}
        ns |= set(int(v) for v in rng.integers(0, 2 ** 31, 8))
        ns = [v for v in ns if 0 <= v <= top]
        n += ns
        d += [x] * len(ns)
    return np.array(n, np.uint32), np.array(d, np.uint32)


def block_corner_slots(npix_padded):
    """the slots of the four corner pixels of every block of TILE_BLOCK x TILE_BLOCK tiles (the 16 x 16 pixel square's corners)"""
    per_block = 64 * TILE_BLOCK * TILE_BLOCK
    b = np.arange(npix_padded // per_block, dtype=np.int64)[:, None] * per_block
    last = TILE_BLOCK - 1
    corners = np.array([0, last * 64 + 7, last * TILE_BLOCK * 64 + 56, (TILE_BLOCK * TILE_BLOCK - 1) * 64 + 63], np.int64)
    return (b + corners[None, :]).reshape(-1)


def slot_cases(width, height, rank, world, stripe_rows, seed=31):
    """(slots, pixels (N, 2)) of one geometry: every slot and every local pixel of a small frame; of a large one the corners of every block,
    4096 random slots, the pixels those slots name and the first pixel of every local row"""
    rows, tiles_x, tiles_y, npix = geometry(width, height, rank, world, stripe_rows)
    if (width, height) in SMALL_FRAMES:
        slots = np.arange(npix, dtype=np.int64)
        ly, lx = np.divmod(np.arange(width * rows, dtype=np.int64), width)
    else:
        rng = np.random.default_rng(seed + rank)
        slots = np.unique(np.concatenate([block_corner_slots(npix), rng.integers(0, npix, 4096)]))
        sx, sy, ok = slot_to_local(width, rows, tiles_x, slots)
        lx = np.concatenate([sx[ok], np.zeros(rows, np.int64)])
        ly = np.concatenate([sy[ok], np.arange(rows, dtype=np.int64)])
    return slots.astype(np.uint32), np.ascontiguousarray(np.stack([lx, ly], axis=1).astype(np.int32))


SLOT_FRAME_CASES = (
    # batch_frames, frame_spp, batch_reset, frame_offset, sample_base, frame_id
    (1, 1, 0, 0, 0, 0), (1, 16, 1, 5, 3, 3), (4, 1, 1, 0, 0, 0), (4, 1, 0, 9, 2, 2), (3, 5, 1, 77, 10, 10), (3, 5, 0, 77, 10, 10),
    (8, 2, 1, 0xFFFFFFF0, 14, 14), (8, 2, 0, 0xFFFFFFF0, 0xFFFFFFF8, 0xFFFFFFF8), (2, 7, 1, 0, 0xFFFFFFFE, 1), (16, 1, 0, 1, 0, 0),
)
