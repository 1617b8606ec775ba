"""The premise of tests/test_gpu_surface_queries.py, checked without a GPU: on its cases the oracle's ray log holds exactly one primary
ray per pixel, and the frame the oracle renders together with its AOV images is the frame of the logged render -- the AOV images belong
to the logged rays."""
import numpy as np
import pytest

import oracle_lib as O
from surface_query_cases import CASES, primary_rays, scene


@pytest.mark.parametrize("name,variant,W,H", CASES)
def test_the_logged_primaries_are_the_rays_behind_the_aov_images(name, variant, W, H):
    s = scene(name)
    osc = O.OracleScene(s)
    q, logged = primary_rays(osc, s, W, H, variant)
    assert q.shape == (W * H, 8) and np.isfinite(q[:, 0:7]).all()
    frame, _, aovs = osc.render(W, H, 1, variant=variant, aovs=True)
    assert np.array_equal(frame.view(np.uint32), logged.view(np.uint32))
    assert [a.shape for a in aovs] == [(H, W, 4)] * 3
