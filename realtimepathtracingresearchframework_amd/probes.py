"""Irradiance probes on the host side (include/rptr_hip.h "irradiance probes"; RenderHip.trace_probes): the direction set, a rotation per
call for per-frame rotated ray sets, the SH basis the device projects onto, the cosine-lobe convolution that turns radiance coefficients
into irradiance, and a regular grid of positions.

The per-frame loop of a probe grid that refines over time:

    pos = probes.grid(lo, hi, counts)
    coeffs = np.zeros((len(pos), 9, 4), np.float32)
    for i in range(frames):
        r.trace_probes(pos, camera, coeffs=coeffs, rotation=probes.rotation(i), sample_index=i, blend=1.0 if i == 0 else 0.1)
    E = probes.sh_irradiance(coeffs[k], normals)
"""
import ctypes as C
import math

import numpy as np

from . import abi

SH_C = np.float32([0.282095, 0.488603, 0.488603, 0.488603, 1.092548, 1.092548, 0.315392, 1.092548, 0.546274])
# the zonal coefficients of the clamped cosine lobe, per band (Ramamoorthi & Hanrahan 2001): pi, 2 pi / 3, pi / 4
SH_COSINE = np.array([math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5)


def directions(K) -> np.ndarray:
    """(K, 3) float32: the spherical Fibonacci set of rptr_hip_probe_directions -- the table the device uses, from the library"""
    from . import backend
    L = backend.load_library()
    out = np.zeros((int(K), 3), np.float32)
    rc = L.rptr_hip_probe_directions(int(K), out.ctypes.data_as(C.c_void_p))
    if rc != abi.RPTR_OK:
        raise backend.BackendError(rc, (L.rptr_hip_last_error(None) or b"").decode())
    return out


def rotation(index) -> np.ndarray:
    """(3, 3) float32, row-major: a rotation per call index, well spread over SO(3) -- Shoemake's uniform quaternion from the (2, 3, 5)
    Halton point of index + 1 -- computed in double and rounded once. index 0, 1, 2, ... give different ray sets per frame."""
    def halton(i, base):
        f, r = 1.0, 0.0
        while i > 0:
            f /= base
            r += f * (i % base)
            i //= base
        return r

    i = int(index) + 1
    u1, u2, u3 = halton(i, 2), halton(i, 3), halton(i, 5)
    a, b = math.sqrt(1.0 - u1), math.sqrt(u1)
    x, y, z, w = a * math.sin(2 * math.pi * u2), a * math.cos(2 * math.pi * u2), b * math.sin(2 * math.pi * u3), b * math.cos(2 * math.pi * u3)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)
    return R.astype(np.float32)


def sh_basis(d) -> np.ndarray:
    """(..., 9): the real L2 basis at directions d (..., 3), in the order and with the constants of the device's projection; the result
    has d's floating-point type (float32 in: the device's products and sums, operation for operation)"""
    d = np.asarray(d)
    t = d.dtype.type if d.dtype in (np.float32, np.float64) else np.float64
    x, y, z = (d[..., k].astype(t) for k in range(3))
    c = SH_C.astype(t)
    one, three = t(1.0), t(3.0)
    Y = [np.full(x.shape, c[0], t), c[1] * y, c[2] * z, c[3] * x, c[4] * (x * y), c[5] * (y * z), c[6] * (three * (z * z) - one), c[7] * (x * z),
         c[8] * (x * x - y * y)]
    return np.stack(Y, axis=-1)


def sh_irradiance(coeffs, normals) -> np.ndarray:
    """irradiance E(n) = sum_i A_i c_i Y_i(n): coeffs (..., 9, C) radiance coefficients as trace_probes returns them, normals (m, 3) unit
    vectors; returns (..., m, C) float64. A = pi, 2 pi / 3 (band 1), pi / 4 (band 2)."""
    c = np.asarray(coeffs, np.float64)
    Y = sh_basis(np.asarray(normals, np.float64).reshape(-1, 3))  # (m, 9)
    return np.einsum("mi,...ic->...mc", Y * SH_COSINE, c)


def grid(lo, hi, counts) -> np.ndarray:
    """(nx ny nz, 3) float32: a regular grid of probe positions over the box [lo, hi], cell-centred (probe (i, j, k) at lo + (index +
    0.5) * (hi - lo) / counts), x fastest; computed in double, rounded once"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    n = [int(c) for c in counts]
    axes = [lo[a] + (np.arange(n[a]) + 0.5) * (hi[a] - lo[a]) / n[a] for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
