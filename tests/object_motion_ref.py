"""Object motion vectors in float64: the yardstick of tests/test_object_motion_cpu.py and tests/test_gpu_object_motion.py.

The rule is the one include/rptr_hip.h states at rptr_hip_object_motion:

    ray      the representative ray of pixel (x, y): through ((x + .5) / W, (y + .5) / H) [+ 0.5 * screen_jitter], pinhole, from the camera
             (tests/dof_ref.py lens_ray without draws: float32, the operations of csrc/kernels.h rp_primary_ray_ex)
    hit      closest hit of the oracle's brute-force trace (opaque geometry, interval (0, inf)) on the CURRENT scene
    x_cur    origin + t * direction
    x_prev   O2W_prev(i) * (O2W_cur(i)^-1 * x_cur) for a rigid instance; for a geometry whose positions changed the (u, v) interpolation of
             the triangle's PREVIOUS positions, through O2W_prev(i)
    value    project(view_ref, x_prev) / max(w, 0) - project(view, x_cur) / max(w, 0), the arithmetic of csrc/dshade.h rp_store_geometry_aovs
    mask     hits on an instance whose transform differs bitwise from the previous one, or on a geometry whose positions changed

Everything after the float32 ray and the oracle's (t, u, v) is float64."""
import numpy as np

import dof_ref as D
import oracle_lib as O


def view_projection(cam, W, H):
    """the x / y / w rows of VP as csrc/host_frame.inl compute_view_projection makes them, in float64: (view (3, 4), proj (2,))"""
    pos, d, up, fovy = D._cam_fields(cam)
    pos, d, up = np.asarray(pos, np.float64), np.asarray(d, np.float64), np.asarray(up, np.float64)
    cx, cz = np.cross(d, up), -d
    r = np.stack([np.cross(up, cz), np.cross(cz, cx), np.cross(cx, up)]) / np.dot(cx, np.cross(up, cz))
    view = np.concatenate([r, -(r @ pos)[:, None]], axis=1)
    tan = np.tan(np.radians(float(fovy)) / 2.0)
    return view, np.array([1.0 / (tan * (float(W) / float(H))), 1.0 / tan])


def project(view, proj, p):
    v = p @ view[:, :3].T + view[:, 3]
    return proj[0] * v[:, 0], -(proj[1] * v[:, 1]), -v[:, 2]


def motion(view_ref, proj_ref, view, proj, x_prev, x_cur):
    """(n, 2): the .xy of the motion + jitter texel for world points x_cur seen at x_prev by the reference view"""
    rx, ry, rw = project(view_ref, proj_ref, x_prev)
    cx, cy, cw = project(view, proj, x_cur)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd, cd = np.maximum(rw, 0.0), np.maximum(cw, 0.0)
        return np.stack([rx / rd - cx / cd, ry / rd - cy / cd], axis=-1)


def affine(m, p):
    m = np.asarray(m, np.float64).reshape(3, 4)
    return p @ m[:, :3].T + m[:, 3]


def affine_inverse(m):
    m = np.asarray(m, np.float64).reshape(3, 4)
    inv = np.linalg.inv(m[:, :3])
    return np.concatenate([inv, -(inv @ m[:, 3])[:, None]], axis=1)


def hits(scene, W, H, cam, jitter=None, dyn_cur=None):
    """the representative rays of every pixel against `scene` (its float positions of dynamic geometries: dyn_cur {geometry: (n, 3)}):
    (x_cur (W H, 3) float64, hit (W H,) bool, instance, global geometry, primitive, u, v), pixels row by row"""
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = D.lens_ray(cam, W, H, xs.reshape(-1), ys.reshape(-1), None, None, 0.0, 0.0, jitter=jitter)
    osc = O.OracleScene(scene)
    for g, P in (dyn_cur or {}).items():
        osc.set_dynamic_vertices(g, P)
    tuv, ids = osc.trace_ex(o, d, 0.0, np.inf, bvh_mode=O.BVH_BRUTE)
    osc.close()
    hit = tuv[:, 0] >= 0
    inst = np.where(hit, ids[:, 0], 0)
    first = np.array([scene.meshes[scene.pmeshes[i.pmesh].mesh].first_geometry for i in scene.instances], np.int64)
    geom = first[inst] + np.where(hit, ids[:, 1], 0)
    x_cur = o.astype(np.float64) + tuv[:, 0:1].astype(np.float64) * d.astype(np.float64)
    return x_cur, hit, inst, geom, np.where(hit, ids[:, 2], 0), tuv[:, 1].astype(np.float64), tuv[:, 2].astype(np.float64)


def reference(scene, W, H, cam, cam_ref, xf_prev, xf_cur, dyn_prev=None, dyn_cur=None, jitter=None, every_hit=False):
    """scene: the CURRENT scene (instances at xf_cur); xf_prev / xf_cur: (n, 3, 4) object-to-world of every instance in the previous /
    this frame (float32 arrays are compared bitwise for "moved"); dyn_prev / dyn_cur: {global geometry: (3 tris, 3) positions} of the
    geometries whose positions changed; cam_ref: the previous frame's camera. every_hit: the value of every pixel that hits, moved or not.
    -> (xy (H, W, 2) float64, NaN where nothing is written; mask (H, W) bool)"""
    x_cur, hit, inst, geom, prim, u, v = hits(scene, W, H, cam, jitter, dyn_cur)
    xf_prev, xf_cur = np.asarray(xf_prev), np.asarray(xf_cur)
    n = len(scene.instances)
    moved_inst = np.array([xf_prev[i].astype(np.float32).tobytes() != xf_cur[i].astype(np.float32).tobytes() if xf_prev.dtype == np.float32 and xf_cur.dtype == np.float32
                           else not np.array_equal(xf_prev[i], xf_cur[i]) for i in range(n)])
    deformed = np.isin(geom, list((dyn_prev or {}).keys())) & hit
    mask = hit & (moved_inst[inst] | deformed)
    todo = hit if every_hit else mask
    x_prev = x_cur.copy()
    for i in range(n):
        sel = todo & (inst == i) & ~deformed
        if sel.any():
            x_prev[sel] = affine(xf_prev[i], affine(affine_inverse(xf_cur[i]), x_cur[sel]))
    for g, P in (dyn_prev or {}).items():
        P = np.asarray(P, np.float64).reshape(-1, 3, 3)
        for i in range(n):
            sel = todo & deformed & (geom == g) & (inst == i)
            if sel.any():
                t = P[prim[sel]]
                p_obj = (1.0 - u[sel] - v[sel])[:, None] * t[:, 0] + u[sel][:, None] * t[:, 1] + v[sel][:, None] * t[:, 2]
                x_prev[sel] = affine(xf_prev[i], p_obj)
    view, proj = view_projection(cam, W, H)
    view_ref, proj_ref = view_projection(cam_ref, W, H)
    xy = np.full((W * H, 2), np.nan)
    xy[todo] = motion(view_ref, proj_ref, view, proj, x_prev[todo], x_cur[todo])
    return xy.reshape(H, W, 2), mask.reshape(H, W)
