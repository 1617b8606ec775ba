"""The irradiance-probe rule of include/rptr_hip.h (csrc/probes.h) restated in numpy float32, operation for operation: every product and
sum is one float32 operation on float32 operands, in the header's association. The direction table comes from the library
(probes.directions: the table the device is given), never from this file's own libm."""
import numpy as np

F = np.float32
SH_C = [F(0.282095), F(0.488603), F(0.488603), F(0.488603), F(1.092548), F(1.092548), F(0.315392), F(1.092548), F(0.546274)]
SKIP_BITS = np.uint32(0xFFFFFFFF)  # mode_or_data = -1


def directions_f64(K):
    """the spherical Fibonacci set in double (numpy's libm): what rptr_hip_probe_directions rounds to float"""
    k = np.arange(K, dtype=np.float64)
    g = (np.sqrt(5.0) - 1.0) / 2.0
    z = 1.0 - (2.0 * k + 1.0) / K
    kg = k * g
    phi = 2.0 * np.pi * (kg - np.floor(kg))
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def rotate(table, rotation):
    """(K, 3) float32: dir[r] = (R[r][0] x + R[r][1] y) + R[r][2] z"""
    R = np.asarray(rotation, F).reshape(3, 3)
    t = np.asarray(table, F)
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    return np.stack([(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z for r in range(3)], axis=1).astype(F)


def usable(positions):
    return np.isfinite(np.asarray(positions, F)).all(axis=1)


def rays(positions, table, rotation, t_max):
    """(n K, 8) float32 records (compare as bits: mode_or_data = -1 is a NaN pattern)"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    d = rotate(table, rotation)
    n, K = len(pos), len(d)
    q = np.zeros((n, K, 8), F)
    q[:, :, 0:3] = pos[:, None, :]
    q[:, :, 4:7] = d[None, :, :]
    q[:, :, 7] = F(t_max)
    bits = q.view(np.uint32)
    bits[:, :, 3] = np.where(usable(pos), np.uint32(0), SKIP_BITS)[:, None]
    return q.reshape(n * K, 8)


def basis(d):
    """(K, 9) float32 from float32 directions"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    one, three = F(1.0), F(3.0)
    Y = [np.full(len(d), SH_C[0], F), SH_C[1] * y, SH_C[2] * z, SH_C[3] * x, SH_C[4] * (x * y), SH_C[5] * (y * z), SH_C[6] * (three * (z * z) - one),
         SH_C[7] * (x * z), SH_C[8] * (x * x - y * y)]
    out = np.stack(Y, axis=1)
    assert out.dtype == F
    return out


def sanitise(values, clamp):
    """(..., 4) float32: rays with a non-finite component -> 0; rgb scaled by clamp / max(r, g, b) where that exceeds clamp > 0"""
    v = np.array(values, F, copy=True)
    v[~np.isfinite(v).all(axis=-1)] = F(0.0)
    clamp = F(clamp)
    if clamp > 0:
        m = np.maximum(np.maximum(v[..., 0], v[..., 1]), v[..., 2])
        over = m > clamp
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # (the lanes `over` does not select)
            s = (clamp / m).astype(F)
            for ch in range(3):
                v[..., ch] = np.where(over, v[..., ch] * s, v[..., ch])
    return v


def project(values, table, rotation, clamp=0.0, blend=1.0, old=None, positions=None):
    """values (n, K, 4) -> coefficients (n, 9, 4) float32 with the device's sum order: lane l takes k = l, l + 64, ... ascending from +0,
    then the xor butterfly over 32, 16, 8, 4, 2, 1, then the weight float(4 pi / K) and the blend. `old`: what the buffer held (kept by
    skipped probes; blended into for blend != 1)."""
    table = np.asarray(table, F)
    K = len(table)
    v = sanitise(np.asarray(values, F).reshape(-1, K, 4), clamp)
    n = len(v)
    Y = basis(rotate(table, rotation))  # (K, 9)
    trips = (K + 63) // 64
    terms = np.zeros((n, trips * 64, 9, 4), F)
    terms[:, :K] = v[:, :, None, :] * Y[None, :, :, None]
    have = np.zeros(trips * 64, bool)
    have[:K] = True
    acc = np.zeros((n, 64, 9, 4), F)
    for t in range(trips):
        sl = slice(64 * t, 64 * t + 64)
        acc = np.where(have[sl][None, :, None, None], acc + terms[:, sl], acc)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    assert acc.dtype == F
    assert (acc.view(np.uint32) == acc[:, :1].view(np.uint32)).all()  # IEEE addition commutes: every lane ends with the same bits
    w = F(4.0 * np.pi / K)
    new = acc[:, 0] * w
    blend = F(blend)
    if old is not None:
        old = np.asarray(old, F).reshape(n, 9, 4)
    if blend != F(1.0):
        with np.errstate(invalid="ignore", over="ignore"):
            new = old + (new - old) * blend
    if positions is not None:
        keep = ~usable(np.asarray(positions, F).reshape(-1, 3))
        if keep.any():
            new = new.copy()
            new.view(np.uint32)[keep] = old.view(np.uint32)[keep]
    return new.astype(F)


def project_f64(values, table, rotation, clamp=0.0):
    """the same sums in float64: the same float32 basis values and sanitised ray values, the products, the sums and the weight in double;
    with the sum of |terms| beside them: (n, 9, 4), (n, 9, 4)"""
    table = np.asarray(table, F)
    K = len(table)
    v = sanitise(np.asarray(values, F).reshape(-1, K, 4), clamp).astype(np.float64)
    Y = basis(rotate(table, rotation)).astype(np.float64)
    terms = v[:, :, None, :] * Y[None, :, :, None]
    w = 4.0 * np.pi / K
    return terms.sum(axis=1) * w, np.abs(terms).sum(axis=1) * w
