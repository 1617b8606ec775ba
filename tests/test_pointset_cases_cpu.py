"""The point-set cases of tests/shade_cases.py on the CPU: they reach the edges tests/test_gpu_pointset_functions.py relies on, evaluated on
the oracle (orc_pointset_probe, orc_rng_probe), and the integer restatement of the uniform generator equals the oracle's."""
import numpy as np

import oracle_lib as O
import shade_cases as S
from realtimepathtracingresearchframework_amd import abi, pointsets, scenes


def test_generator_restatement_and_the_state_that_gives_one():
    states = S.randf_states()
    nxt, f = S.randf_ref(states)
    assert f.dtype == np.float32 and (f <= 1.0).all() and (f >= 0.0).all()
    # rp_randf == 1.0 occurs: a state steps onto 0xFFFFFF80 (the smallest that rounds up to 2^32) and onto 0xFFFFFFFF; 0xFFFFFF7F stays below
    assert (f == 1.0).sum() >= 2 and 0xFFFFFF80 in nxt and 0xFFFFFFFF in nxt
    assert f[nxt == 0xFFFFFF7F][0] == np.float32(1.0 - 2.0 ** -24) and f[nxt == 0][0] == 0.0
    # the restatement walks the oracle's generator: seed state and eight draws
    for (index, frame, px, py, w) in ((3, 7, 10, 20, 256), (0, 0, 0, 0, 200), (2 ** 24, 0xFFFFFFF0, 7679, 4319, 7680)):
        state, draws = O.rng_probe(index, frame, px, py, w, n=8)
        s = np.array([state], np.uint32)
        for k in range(8):
            s, v = S.randf_ref(s)
            assert v[0] == draws[k]


def test_pointset_cases_reach_the_edges():
    q, dims = S.pointset_queries(), S.pointset_dims()
    assert len(q) * len(dims) <= 2 ** 17
    width, si, fo, fi, px, py = (q[:, k].astype(np.int64) for k in range(6))
    assert (px >= 256).any() and (py >= 256).any() and (width < 256).any() and ((px >> 8) + (py >> 8) * (width >> 8) > 0).any()
    assert (65536 * si >= 2 ** 32).any() and (fo * 13 + fi >= 2 ** 32).any() and (px + py * width >= 2 ** 24).any()
    assert {1023, 1024, 1025, 2047, 8191} <= set(dims.tolist()) and (dims // 8 // 128 >= 1).any()
    bn_dim = dims.astype(np.int64) % 8 + dims.astype(np.int64) // 1024 * 8        # (bn_rng.glsl: before the mask of BNData_Dimensions - 1)
    assert ((bn_dim >= 128) & (bn_dim < 256)).any() and (bn_dim >= 256).any()
    assert set(range(6 + 8 * abi.MAX_PATH_DEPTH, 6 + 8 * abi.MAX_PATH_DEPTH + 8)) <= set(dims.tolist())
    # the wrapped Z-Sobol' index: 65536 * 65536 = 2^32 shifts by nothing, so sample 65536 names the points of sample 0
    osc = O.OracleScene(scenes.cornell32())
    osc.set_rng_variant(abi.RNG_VARIANT_Z_SBL, pointsets.default_table(abi.RNG_VARIANT_Z_SBL))
    a = osc.pointset_probe(65536, 0, 0, 300, 200, 1920, 0, dims)
    b = osc.pointset_probe(0, 0, 0, 300, 200, 1920, 0, dims)
    c = osc.pointset_probe(1, 0, 0, 300, 200, 1920, 0, dims)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and c[1] != b[1] and c[1] >= 65536
    # beyond the Sobol' dimensions the mask wraps: d and d - 1024 draw from the same matrix (the scramble differs: compare single draws)
    osc.set_rng_variant(abi.RNG_VARIANT_SOBOL, pointsets.default_table(abi.RNG_VARIANT_SOBOL))
    assert osc.pointset_probe(5, 3, 0, 9, 9, 256, 0, [1025])[0][0] == osc.pointset_probe(5, 3, 0, 9, 9, 256, 0, [1])[0][0]
    osc.close()
