"""tests/host_tools.py: a host program is compiled once per process."""
import os

from host_tools import build_host_tool


def test_a_host_tool_is_built_once_per_process():
    """rptr_compare needs neither the library nor a GPU: the second call returns the first call's executable, untouched"""
    first = build_host_tool("rptr_compare", link_library=False, extra=("-lz",))
    stamp = os.stat(first).st_mtime_ns
    assert os.access(first, os.X_OK)
    assert build_host_tool("rptr_compare", link_library=False, extra=("-lz",)) == first
    assert os.stat(first).st_mtime_ns == stamp
