"""tests/bvh_check.py on everything the host can build (rptr_hip_build_bvh_host needs no GPU):

  * the checker catches what it claims to: one small mutation of a correct tree per rule, each refused under its own rule's name;
  * every host-built form passes it with zero tolerance: scenes x RPTR_FLATTEN / RPTR_REBRAID / RPTR_COLLAPSE / the host statement of PLOC;
  * the encoder itself (csrc/bvh4.h) under a stand-alone fuzz, plain and with -fsanitize=address,undefined (tests/host_probes/)."""
import copy
import functools
import os
import subprocess

import numpy as np
import pytest

import bvh_check as B
from realtimepathtracingresearchframework_amd import backend, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _forest():
    return scenes.forest(n_meshes=3, tris_per_tree=300, n_instances=25, name="f")


@functools.lru_cache(maxsize=None)
def _base():
    """the small forest, two-level and re-braided (101 records over 13 sub-roots), as the host builds it; never written to"""
    s = _forest()
    nodes, tris, insts, need = backend.build_bvh_host(s)
    rep = B.check_bvh(nodes, tris, insts, s, stack_bound=need)
    for a in (nodes, tris, insts):
        a.setflags(write=False)
    return s, nodes, tris, insts, need, rep


def _leaf(first, count):
    return -2 - (first * 8 + count)


def _occupied(nd, rep, tlas):
    """(n, 3, 4) mask: slot in use, node reached, on the wanted level"""
    use = (nd["child"] != B.EMPTY) & (rep["reached"] & (rep["is_tlas"] == tlas))[:, None]
    return np.broadcast_to(use[:, None, :], (len(nd), 3, 4))


def _mutate_qhi(nd, rep):
    plo, phi = B.decode_planes(nd)
    step = B.grid_step(nd["exp"]).astype(np.float64)[:, :, None]
    slack = phi.astype(np.float64) - rep["slot_hi"].astype(np.float64)
    n, a, k = np.argwhere(_occupied(nd, rep, False) & (slack < 0.5 * step) & (nd["qhi"] > nd["qlo"]))[0]
    nd["qhi"][n, a, k] -= 1


def _mutate_qlo(nd, rep):
    plo, phi = B.decode_planes(nd)
    step = B.grid_step(nd["exp"]).astype(np.float64)[:, :, None]
    slack = rep["slot_lo"].astype(np.float64) - plo.astype(np.float64)
    n, a, k = np.argwhere(_occupied(nd, rep, False) & (slack < 0.5 * step) & (nd["qhi"] > nd["qlo"]))[0]
    nd["qlo"][n, a, k] += 1


def _blas_leaves(nd, rep):
    c = nd["child"]
    for n, k in np.argwhere((c < 0) & (c != B.EMPTY) & (rep["reached"] & ~rep["is_tlas"])[:, None]):
        v = -2 - int(c[n, k])
        yield int(n), int(k), v >> 3, v & 7


def _mutate_leaf_count(nd, rep):
    n, k, first, count = next(x for x in _blas_leaves(nd, rep) if x[3] >= 2)
    nd["child"][n, k] = _leaf(first, count - 1)


def _mutate_leaf_first(nd, rep):
    n, k, first, count = next(x for x in _blas_leaves(nd, rep) if x[3] >= 1 and x[2] > 10)
    nd["child"][n, k] = _leaf(first + 1, count)


def _mutate_swap_leaves(nd, rep):
    plo, phi = B.decode_planes(nd)
    by_node = {}
    for n, k, first, count in _blas_leaves(nd, rep):
        by_node.setdefault(n, []).append(k)
    for n, ks in by_node.items():
        for j in ks:
            for k in ks:   # slot j's stored box does not hold what slot k has below it
                if j != k and ((plo[n, :, j] > rep["slot_lo"][n, :, k]) | (phi[n, :, j] < rep["slot_hi"][n, :, k])).any():
                    nd["child"][n, [j, k]] = nd["child"][n, [k, j]]
                    return
    raise AssertionError("no pair of sibling leaves with different boxes")


def _mutate_origin(nd, rep):
    occ = _occupied(nd, rep, False)
    qhi_max = np.where(occ, nd["qhi"], 0).max(axis=2)                       # (n, 3)
    n, a = np.argwhere(occ.any(axis=2) & (qhi_max <= 254) & (nd["exp"] > 1))[0]
    use = occ[n, a]
    nd["origin"][n, a] = np.float32(nd["origin"][n, a] - B.grid_step(nd["exp"])[n, a])
    nd["qlo"][n, a, use] += 1
    nd["qhi"][n, a, use] += 1


def _mutate_exponent(nd, rep):
    occ = _occupied(nd, rep, False)
    n, a = np.argwhere(occ.any(axis=2) & (nd["exp"] < 250))[0]
    use = occ[n, a]
    nd["exp"][n, a] += 1
    nd["qlo"][n, a, use] //= 2
    nd["qhi"][n, a, use] = (nd["qhi"][n, a, use].astype(np.int32) + 1) // 2


def _mutate_empty_slot(nd, rep):
    n, k = np.argwhere((nd["child"] == B.EMPTY) & rep["reached"][:, None])[0]
    nd["qlo"][n, 1, k], nd["qhi"][n, 1, k] = 0, 255


def _tlas_leaves(nd, rep):
    c = nd["child"]
    for n, k in np.argwhere((c < 0) & (c != B.EMPTY) & rep["is_tlas"][:, None]):
        yield int(n), int(k), (-2 - int(c[n, k])) >> 3


def _mutate_tlas_leaf(nd, rep):
    n, k, first = next(x for x in _tlas_leaves(nd, rep) if x[2] >= 1)
    nd["child"][n, k] = _leaf(first - 1, 1)


def _mutate_instance_box(nd, rep):
    """the lower x bound of an instance box that defines its node's origin, moved up by one float spacing: the plane is inside the box"""
    n, k, first = next(x for x in _tlas_leaves(nd, rep) if nd["qlo"][x[0], 0, x[1]] == 0)
    nd["origin"][n, 0] = np.nextafter(nd["origin"][n, 0], np.float32(np.inf))


MUTATIONS = [
    ("qhi_lowered_by_one", _mutate_qhi, "containment", "upper plane"),
    ("qlo_raised_by_one", _mutate_qlo, "containment", "lower plane"),
    ("leaf_count_minus_one", _mutate_leaf_count, "triangle-once", "0 leaves"),
    ("leaf_first_plus_one", _mutate_leaf_first, "triangle-once", "leaves"),
    ("sibling_leaves_swapped_without_their_boxes", _mutate_swap_leaves, "containment", "cuts into the child"),
    ("origin_one_step_down", _mutate_origin, "origin", "origin"),
    ("exponent_plus_one_q_halved", _mutate_exponent, "exponent", "rp_bvh4_exponent"),
    ("empty_slot_with_a_box", _mutate_empty_slot, "empty-slot", "inverted"),
    ("top_level_leaf_names_the_neighbouring_record", _mutate_tlas_leaf, "record-once", "top-level leaves"),
    ("instance_box_one_float_spacing_short", _mutate_instance_box, "origin", "top level node"),
]


@pytest.mark.parametrize("name,mutate,rule,words", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_the_checker_refuses_a_damaged_tree_under_the_rule_that_was_broken(name, mutate, rule, words):
    s, nodes, tris, insts, need, rep = _base()
    damaged = nodes.copy()
    mutate(B.as_nodes(damaged), rep)
    assert not np.array_equal(damaged.view(np.uint32), nodes.view(np.uint32))
    with pytest.raises(B.BvhCheckError) as e:
        B.check_bvh(damaged, tris, insts, s, stack_bound=need)
    print(e.value)
    assert e.value.rule == rule and str(e.value).startswith("rule %s:" % rule) and words in str(e.value), str(e.value)
    assert "node" in str(e.value) or "record" in str(e.value)


def test_contained_mutations_pass_containment_alone():
    """origin one step down and exp + 1 with halved q still CONTAIN everything (which is why containment alone would not do): the planes
    of the damaged nodes, decoded, hold the exact bounds below them"""
    s, nodes, tris, insts, need, rep = _base()
    for mutate in (_mutate_origin, _mutate_exponent):
        damaged = nodes.copy()
        nd = B.as_nodes(damaged)
        mutate(nd, rep)
        plo, phi = B.decode_planes(nd)
        use = _occupied(nd, rep, False)
        assert (plo[use] <= rep["slot_lo"][use]).all() and (phi[use] >= rep["slot_hi"][use]).all()


def test_the_checker_holds_the_stack_against_the_reported_bound_and_refuses_presplit_trees(monkeypatch):
    s, nodes, tris, insts, need, rep = _base()
    assert rep["stack_entries"] <= need
    with pytest.raises(B.BvhCheckError) as e:
        B.check_bvh(nodes, tris, insts, s, stack_bound=rep["stack_entries"] - 1)
    assert e.value.rule == "stack"
    monkeypatch.setenv("RPTR_PRESPLIT", "3000,2.0")
    n2, t2, i2, _ = backend.build_bvh_host(s)
    with pytest.raises(B.BvhCheckError) as e:
        B.check_bvh(n2, t2, i2, s)
    assert e.value.rule == "presplit" and "RPTR_PRESPLIT" in str(e.value)


def test_overrides_of_transforms_and_positions_are_what_the_records_are_held_against():
    """the tree of a scene with other transforms / other vertices passes against the ORIGINAL scene only with the overrides"""
    s = scenes.two_level_test()
    moved = copy.copy(s)
    moved.instances = [copy.copy(i) for i in s.instances]
    xf = {}
    for k in (2, 7):
        M = np.asarray(s.instances[k].transform, np.float32).copy()
        M[:, 3] += np.float32(0.75)
        M[0, 1] += np.float32(0.3)
        moved.instances[k].transform = xf[k] = M
    nodes, tris, insts, need = backend.build_bvh_host(moved)
    B.check_bvh(nodes, tris, insts, s, transforms=xf, stack_bound=need)
    with pytest.raises(B.BvhCheckError) as e:
        B.check_bvh(nodes, tris, insts, s)
    assert e.value.rule == "record"
    # positions: the same tree against a scene whose geometry 1 holds other vertices
    other = copy.copy(s)
    other.geometries = list(s.geometries)
    g = copy.copy(s.geometries[1])
    g.qpos = np.roll(np.asarray(g.qpos), 3)
    other.geometries[1] = g
    with pytest.raises(B.BvhCheckError) as e:
        B.check_bvh(nodes, tris, insts, other, transforms=xf)
    assert e.value.rule == "tri-record"
    g0 = s.geometries[1]
    B.check_bvh(nodes, tris, insts, other, transforms=xf, positions={1: scenes.dequantize_positions(g0.qpos, g0.scaling, g0.offset)})


# ------------------------------------------------------------------ the host builder, every form
SCENES = {
    "cornell32": scenes.cornell32,
    "glass_test": scenes.glass_test,
    "two_level_test": scenes.two_level_test,
    "grid48x24_emitters": lambda: scenes.grid(48, 24, with_emitters=True),
    "forest25": _forest,
    "soup3": lambda: scenes.soup(3),
    "soup5": lambda: scenes.soup(5),
    "soup6": lambda: scenes.soup(6),
    "soup7": lambda: scenes.soup(7),
    "alpha_test": scenes.alpha_test,
    "textured_test": scenes.textured_test,
    "book512": lambda: scenes.book(512),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


def _one_dynamic(name):
    s = copy.copy(_scene(name))
    s.meshes = [copy.copy(m) for m in s.meshes]
    s.meshes[0].dynamic = True
    return s


PLOC = {"RPTR_HOST_PLOC": "25", "RPTR_PLOC_LEAF": "2"}
SWEEP = [(name, {"RPTR_FLATTEN": f}) for name in SCENES for f in ("0", "1")]
SWEEP += [(name, {"RPTR_FLATTEN": "-1", "dynamic": "1"}) for name in ("forest25", "soup3", "two_level_test")]
SWEEP += [(name, {"RPTR_REBRAID": b}) for name in ("forest25", "soup5") for b in ("1", "4", "9")]
SWEEP += [(name, {"RPTR_COLLAPSE": c, "RPTR_FLATTEN": f}) for name in ("forest25", "soup7") for c in ("greedy", "optimal", "even") for f in ("0", "1")]
SWEEP += [(name, {"RPTR_COLLAPSE": "even", "RPTR_REBRAID": "9"}) for name in ("forest25",)]
SWEEP += [(name, dict(PLOC, RPTR_FLATTEN=f)) for name in ("forest25", "soup6", "grid48x24_emitters") for f in ("0", "1")]
SWEEP += [(name, dict(PLOC, RPTR_FLATTEN="-1", dynamic="1", RPTR_PLOC_TOP="16")) for name in ("forest25", "soup3")]


@pytest.mark.parametrize("name,env", SWEEP, ids=["%s-%s" % (n, ",".join("%s=%s" % (k.replace("RPTR_", "").lower(), v) for k, v in sorted(e.items()))) for n, e in SWEEP])
def test_every_host_built_form_passes_the_exact_checker(name, env, monkeypatch):
    env = dict(env)
    s = _one_dynamic(name) if env.pop("dynamic", None) else _scene(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nodes, tris, insts, need = backend.build_bvh_host(s)
    rep = B.check_bvh(nodes, tris, insts, s, stack_bound=need)
    print("%s %s: %d nodes, %d records, worst slack %.6f steps, instance overhang %.3f of its bound, stack %d <= %d" % (
        name, env, rep["nodes_reached"], rep["top_records"], rep["worst_slack_steps"], rep["worst_instance_overhang"], rep["stack_entries"], need))
    assert rep["nodes_reached"] + rep["unreached_nodes"] == rep["nodes"] and rep["worst_slack_steps"] < 2.0
    if env.get("RPTR_FLATTEN") == "1" and len(s.instances) > 1:
        assert rep["top_records"] == 1 and rep["records"] == 1 + len(s.instances) and rep["triangles"] == s.num_instanced_tris()
    if env.get("RPTR_FLATTEN") == "-1":
        n_dyn = sum(1 for i in s.instances if s.pmeshes[i.pmesh].mesh == 0)
        assert rep["top_records"] == 1 + n_dyn
    if env.get("RPTR_REBRAID") in ("4", "9"):
        assert len(s.instances) < rep["top_records"] <= int(env["RPTR_REBRAID"]) * len(s.instances) and rep["sub_roots"]


# ------------------------------------------------------------------ the encoder
def _build_fuzz(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra,
                           "-I" + os.path.join(ROOT, "realtimepathtracingresearchframework_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_probes", "bvh4_encode_fuzz.cpp"), "-o", exe])
    return exe


def test_encoder_fuzz(tmp_path):
    """rp_bvh4_encode on adversarial boxes (large offsets with tiny extents, sub-normal extents, near FLT_MAX, 200-binade mixes, -0.0,
    lo == hi, 1 to 4 children): containment, origin, exponent and tightness, checked by the program itself"""
    p = subprocess.run([_build_fuzz(tmp_path, "fuzz", []), "60000"], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "bvh4 encoder fuzz: 540000 nodes" in p.stdout, p.stderr


def test_encoder_fuzz_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined and run as a plain executable (another seed)"""
    exe = _build_fuzz(tmp_path, "fuzz_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    p = subprocess.run([exe, "20000", "7"], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "bvh4 encoder fuzz: 180000 nodes" in p.stdout and "runtime error" not in p.stderr, p.stderr
