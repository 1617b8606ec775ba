"""The closest-hit query entry points without a GPU: a NULL handle and bad arguments are refused before the device is touched
(tests/test_radiance_queries_abi.py and tests/test_surface_queries_abi.py do the same for their kinds; tests/test_gpu_query_entries.py
runs all three)."""
import ctypes as C

import numpy as np

from realtimepathtracingresearchframework_amd import abi, backend


def _refused(L, rc):
    assert rc == abi.RPTR_E_INVALID, rc
    assert "bad argument" in L.rptr_hip_last_error(None).decode(), L.rptr_hip_last_error(None)


def test_host_array_entries_refuse_a_null_handle_a_negative_count_and_null_buffers():
    L = backend.load_library()
    q = np.zeros((2, 8), np.float32)
    out = np.full((2, 4), 7.0, np.float32)
    qp, op = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for n, queries, results in ((2, qp, op), (-1, qp, op), (2, None, op), (2, qp, None), (2, None, None)):
        _refused(L, L.rptr_hip_trace(None, queries, n, results))
        _refused(L, L.rptr_hip_trace_counted(None, queries, n, results, None, None, 0))
        _refused(L, L.rptr_hip_trace_counted(None, queries, n, results, None, None, 1))
    assert (out == 7.0).all()


def test_device_entries_refuse_a_null_handle_a_negative_count_and_null_buffers():
    """(the addresses are never dereferenced: the handle is refused first)"""
    L = backend.load_library()
    for n, queries, results in ((2, 4096, 8192), (-1, 4096, 8192), (2, None, 8192), (2, 4096, None)):
        _refused(L, L.rptr_hip_trace_device(None, C.c_void_p(queries), n, C.c_void_p(results), None))
    _refused(L, L.rptr_hip_render_ray_queries(None, 2))
    _refused(L, L.rptr_hip_render_ray_queries(None, -1))
