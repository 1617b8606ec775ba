"""The three kinds of ray query in mixed sequences on one handle, with more queries than the static pools of the persistent traversal
hold: the queries behind the pools are dealt out through a cursor the runs borrow from frame context 0 (csrc/host_queries.inl
borrowed_cursor; csrc/dtraverse.h: "the shared cursor starts behind every static pool"), which a rendered frame and every run leave
advanced. A run that started from a stale cursor would leave result slots untouched."""
import numpy as np
import pytest

from common import random_queries, renderer
from realtimepathtracingresearchframework_amd import abi, backend, scenes

pytestmark = pytest.mark.gpu

FILL = np.float32(7.0)
WAVES_PER_BLOCK = 4  # csrc/dtraverse.h RP_TRAVERSE_BLOCK = 256 threads
FETCH = 64           # the smallest pool a traversal wave takes (option "traverse_fetch")


def _renderer(s, frames_in_flight):
    return renderer(s, 64, 64, frames_in_flight=frames_in_flight, options={"traverse_fetch": FETCH})


def _untouched(rows):
    """rows of a results array whose every word still is the fill value"""
    return (np.ascontiguousarray(rows).view(np.float32).reshape(len(rows), -1) == FILL).all(axis=1)


@pytest.mark.parametrize("scene_name", ["two_level_test", "cornell32"])  # (cornell32: the single-instance instantiations)
def test_every_kind_of_run_starts_from_a_fresh_cursor(scene_name):
    import torch
    s = getattr(scenes, scene_name)()
    r = _renderer(s, 1)
    grid = r.get_option("traversal_grid_shared")
    if grid * WAVES_PER_BLOCK * FETCH + 10000 > 2_000_000:  # a smaller shared grid: three blocks per CU
        r.close()
        r = _renderer(s, 4)
        grid = r.get_option("traversal_grid_shared")
    n = grid * WAVES_PER_BLOCK * FETCH + 10000
    fetch = r.get_option("traverse_fetch")
    print("%s: traversal_grid_shared %d, traverse_fetch %d, %d queries" % (scene_name, grid, fetch, n))
    # the premise: the static pools (one of `fetch` queries per wave of the grid) do not hold all the queries
    assert grid > 0 and fetch == FETCH and grid * WAVES_PER_BLOCK * fetch < n <= 2_000_000

    q = random_queries(np.random.default_rng(11), n, -6, 6)
    q[::7, 3] = np.int32(-1).view(np.float32)  # mode_or_data < 0: the result slot is left alone
    skipped = np.zeros(n, bool)
    skipped[::7] = True
    cam = s.camera_params()

    def closest():
        return r.render_ray_queries(q, np.full((n, 4), FILL, np.float32))

    def surface():
        res = np.zeros(n, abi.SURFACE_HIT_DTYPE)
        res.view(np.float32)[:] = FILL
        return r.render_surface_queries(q, cam, results=res)

    A = closest()                                                                              # 1
    B = surface()                                                                              # 2
    n_rad = 4096
    rad = r.render_radiance_queries(q[:n_rad], cam, spp=1, results=np.full((n_rad, 4), FILL, np.float32))  # 3
    _, visits = r.trace_counted(q, tmin=np.zeros(n, np.float32), any_hit=True)          # 4
    r.render(backend.RenderConfiguration(cam, abi.VARIANT_GLTF, reset_accumulation=True), spp=1)  # 5
    A2 = closest()                                                                             # 6
    B2 = surface()                                                                             # 7

    assert np.array_equal(A2.view(np.uint32), A.view(np.uint32))
    assert np.array_equal(B2.view(np.uint8), B.view(np.uint8))
    for what, res in (("closest", A), ("surface", B), ("radiance", rad)):
        skip = skipped[:len(res)]
        untouched = _untouched(res)
        print("%s: %d of %d slots untouched, %d queries skipped" % (what, int(untouched.sum()), len(res), int(skip.sum())))
        assert not untouched[~skip].any(), what
        assert untouched[skip].all(), what
    hit = ~skipped & (A.view(np.int32)[:, 2] >= 0)
    miss = ~skipped & ~hit
    print("closest: %d hits, %d misses" % (int(hit.sum()), int(miss.sum())))
    assert hit.sum() >= 1000 and miss.sum() >= 1000
    assert (visits[hit] > 0).all()  # nodes and triangles

    # the same queries from device buffers on a caller's stream
    tq = torch.from_numpy(q).cuda()
    tr = torch.full((n, 4), float(FILL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        r.trace_device(tq.data_ptr(), n, tr.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(tr.cpu().numpy().view(np.uint32), A.view(np.uint32))
    r.close()
