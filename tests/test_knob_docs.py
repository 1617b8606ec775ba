"""The compile-time knobs the documents list are switches the sources have (CPU, text only)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtimepathtracingresearchframework_amd", "csrc")


def _documented_knobs(path):
    """RP_* tokens of the paragraphs (blocks between blank lines; a table is one block) that are about build variants: they name tools/mkvariant.sh"""
    text = open(os.path.join(ROOT, path)).read()
    blocks = [b for b in re.split(r"\n\s*\n", text) if "mkvariant.sh" in b]
    return sorted(set(re.findall(r"\bRP_[A-Z0-9_]+\b", "\n".join(blocks))))


def test_every_documented_compile_time_knob_exists():
    """README.md and tools/README.md once listed switches that had long lost their other side. Every RP_* name of their knob paragraphs
    is a switch of the sources: a default under `#ifndef NAME` that -DNAME=... overrides, or (RP_PROF, which has no value) code under
    `#ifdef NAME` that -DNAME turns on."""
    sources = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(f))
    switches = set(re.findall(r"^[ \t]*#[ \t]*ifn?def[ \t]+(RP_[A-Z0-9_]+)\b", sources, re.M))
    for doc in ("README.md", "tools/README.md"):
        knobs = _documented_knobs(doc)
        assert knobs, doc  # the paragraph is still where this test looks for it
        missing = [k for k in knobs if k not in switches]
        assert not missing, (doc, missing)
    assert "RP_NODE_MIN" in _documented_knobs("README.md") and "RP_PROF" in _documented_knobs("tools/README.md")
