"""The product's host-side BVH build (binned SAH -> 4-wide collapse -> 64-byte nodes with 8-bit child boxes,
rptr_hip_build_bvh_host) needs no GPU: the oracle walks the built tree on the CPU and must find exactly what its own
brute force finds; the encoding must be conservative and structurally sound."""
import numpy as np
import pytest

import bvh_check
import oracle_lib as O
from realtimepathtracingresearchframework_amd import backend, scenes

EMPTY = np.int32(-2147483646)  # RPTR_BVH4_EMPTY


NODE_DT = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("pad0", "u1"), ("qlo", "u1", (3, 4)), ("qhi", "u1", (3, 4)),
                    ("child", "<i4", 4), ("pad1", "<u4", 2)])
TRI_DT = np.dtype([("v0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("prim", "<u4"), ("geom", "<u4"), ("pad", "<u4")])


def _rays(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:40, 0] = 0  # axis-parallel rays (safe reciprocal path)
    d[40:80, 2] = 0
    return o, d


@pytest.mark.parametrize("scene_fn,lo,hi", [(scenes.cornell32, -5, 5), (scenes.two_level_test, -6, 6),
                                            (lambda: scenes.grid(48, 24, with_emitters=True), -30, 30),
                                            (lambda: scenes.forest(n_meshes=3, tris_per_tree=300, n_instances=25, name="f"), -6, 6)])
def test_host_built_tree_walked_by_the_oracle_equals_brute_force(scene_fn, lo, hi):
    s = scene_fn()
    nodes, tris, insts, need = backend.build_bvh_host(s)
    assert 2 <= need <= 24 + 128
    osc = O.OracleScene(s)
    osc.import_bvh(nodes, tris, insts)
    o, d = _rays(6000, 5, lo, hi)
    tuv_b, ids_b = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_BRUTE)
    tuv_t, ids_t, visits = osc.trace_ex_counts(o, d, 1e-4, 1e20, bvh_mode=O.BVH_IMPORTED)
    assert np.array_equal(tuv_b.view(np.uint32), tuv_t.view(np.uint32)) and np.array_equal(ids_b, ids_t)
    assert (ids_b[:, 0] >= 0).sum() > 100 and visits[:, 0].max() < 2000
    # occlusion queries over clipped intervals agree too
    tmax = np.where(tuv_b[:, 0] > 0, tuv_b[:, 0] * np.random.default_rng(1).choice([0.5, 1.5], len(o)), 5.0).astype(np.float32)
    any_b = osc.trace_ex(o, d, 1e-4, tmax, any_hit=True, bvh_mode=O.BVH_BRUTE)[1][:, 0]
    any_t = osc.trace_ex(o, d, 1e-4, tmax, any_hit=True, bvh_mode=O.BVH_IMPORTED)[1][:, 0]
    assert np.array_equal(any_b, any_t)


@pytest.mark.parametrize("scene_fn,lo,hi", [(scenes.cornell32, -5, 5), (lambda: scenes.soup(3, n_meshes=2, tris_per_mesh=150, n_instances=4), -4, 4),
                                            (lambda: scenes.forest(n_meshes=3, tris_per_tree=300, n_instances=25, name="f"), -6, 6)])
@pytest.mark.parametrize("flatten", ["0", "1"])
def test_trees_with_split_references_still_equal_brute_force(scene_fn, lo, hi, flatten, monkeypatch):
    """RPTR_PRESPLIT (csrc/bvh_build.h presplit_triangles): a triangle is referenced by several leaves, each with the box of a part of it.
    The parts cover the triangle (boxes rounded outwards), every reference names the same triangle record, so the closest hit -- smallest t,
    ties by (instance, geometry, primitive) -- and every occlusion answer stay those of brute force, bit for bit; slivers, points,
    duplicates and flat meshes (the soup) included."""
    s = scene_fn()
    monkeypatch.setenv("RPTR_FLATTEN", flatten)
    monkeypatch.setenv("RPTR_PRESPLIT", "0")
    nodes0, tris0, insts0, _ = backend.build_bvh_host(s)
    monkeypatch.setenv("RPTR_PRESPLIT", "3000,2.0")
    nodes, tris, insts, need = backend.build_bvh_host(s)
    assert len(tris) > 1.2 * len(tris0)       # references were added ...
    t0, t1 = tris0.view(TRI_DT), tris.view(TRI_DT)
    rec0 = {bytes(r) for r in t0}
    assert {bytes(r) for r in t1} == rec0     # ... and every reference is one of the scene's triangle records, none is lost
    osc = O.OracleScene(s)
    osc.import_bvh(nodes, tris, insts)
    o, d = _rays(6000, 7, lo, hi)
    if flatten == "1" and len(s.instances) > 1:
        # a flattened scene intersects world-space triangles (t / u / v differ from the object-space brute force by rounding): the
        # yardstick is the flattened tree WITHOUT split references, which holds the very same triangle records
        base = O.OracleScene(s)
        base.import_bvh(nodes0, tris0, insts0)
        truth = lambda *a, **k: base.trace_ex(*a, bvh_mode=O.BVH_IMPORTED, **k)  # noqa: E731
    else:
        truth = lambda *a, **k: osc.trace_ex(*a, bvh_mode=O.BVH_BRUTE, **k)  # noqa: E731
    tuv_b, ids_b = truth(o, d, 1e-4, 1e20)
    tuv_t, ids_t = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_IMPORTED)
    assert (ids_b[:, 0] >= 0).sum() > 100
    assert np.array_equal(tuv_b.view(np.uint32), tuv_t.view(np.uint32)) and np.array_equal(ids_b, ids_t)
    tmax = np.where(tuv_b[:, 0] > 0, tuv_b[:, 0] * np.random.default_rng(2).choice([0.5, 1.5], len(o)), 5.0).astype(np.float32)
    any_b = truth(o, d, 1e-4, tmax, any_hit=True)[1][:, 0]
    any_t = osc.trace_ex(o, d, 1e-4, tmax, any_hit=True, bvh_mode=O.BVH_IMPORTED)[1][:, 0]
    assert np.array_equal(any_b, any_t)


def test_encoded_boxes_contain_their_subtrees_and_the_tree_is_sound():
    """tests/bvh_check.py on the height field: every stored plane holds the exact float bounds of the three vertices of everything below
    it with ZERO tolerance, origin and exponent are the encoder's for those bounds, every plane lies within 2 grid steps (+ one float
    spacing) of what it bounds, every triangle record is in exactly one leaf and is its vertices bit for bit, every node is reached
    exactly once, and the traversal stack the builder reports covers the tree"""
    s = scenes.grid(40, 20)
    nodes_f, tris_f, insts_f, need = backend.build_bvh_host(s)
    rep = bvh_check.check_bvh(nodes_f, tris_f, insts_f, s, stack_bound=need)
    print("worst slack %.6f grid steps, %d nodes, stack %d of %d" % (rep["worst_slack_steps"], rep["nodes_reached"], rep["stack_entries"], need))
    assert rep["worst_slack_steps"] < 2.0                                  # the compression is tight
    assert rep["triangles"] == s.num_tris() == len(tris_f) // 12           # every triangle, in exactly one leaf (rule triangle-once)
    assert rep["nodes_reached"] == rep["nodes"] == len(nodes_f) // 16 and rep["unreached_nodes"] == 0   # every node reached exactly once
    # top level: one node with one leaf that names the one instance
    assert rep["tlas_nodes"] == 1 and rep["top_records"] == 1 and rep["mesh_roots"] == [1]
    top = nodes_f.view(NODE_DT)[0]["child"]
    assert (top != EMPTY).sum() == 1 and (-2 - int(top[top != EMPTY][0])) == (0 << 3 | 1)


def test_host_build_rejects_bad_indices():
    s = scenes.cornell32()
    s.instances[0].pmesh = 99
    with pytest.raises(backend.BackendError):
        backend.build_bvh_host(s)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fuzz_soups_host_tree_equals_brute_force(seed):
    """slivers, zero-area and duplicate triangles, flat meshes, sheared / mirrored / non-uniformly scaled instances"""
    s = scenes.soup(seed)
    nodes, tris, insts, need = backend.build_bvh_host(s)
    osc = O.OracleScene(s)
    osc.import_bvh(nodes, tris, insts)
    o, d = _rays(5000, 100 + seed, -5, 5)
    tuv_b, ids_b = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_BRUTE)
    tuv_t, ids_t = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_IMPORTED)
    assert np.array_equal(tuv_b.view(np.uint32), tuv_t.view(np.uint32)) and np.array_equal(ids_b, ids_t)
    tuv_o, ids_o = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_OWN)   # the oracle's own 2-wide float tree agrees too
    assert np.array_equal(tuv_b.view(np.uint32), tuv_o.view(np.uint32)) and np.array_equal(ids_b, ids_o)
    assert (ids_b[:, 0] >= 0).sum() > 200


@pytest.mark.parametrize("braid", [4, 9])
def test_rebraided_instances_give_the_same_answers(monkeypatch, braid):
    """Partial re-braiding: an instance is represented by several records that start at sub-roots of its bottom-level tree.
    More records than instances, same hits (instance ids in the answers are those of the scene), same occlusion."""
    s = scenes.forest(n_meshes=3, tris_per_tree=300, n_instances=25, name="f")
    monkeypatch.setenv("RPTR_REBRAID", "1")
    _, _, insts1, _ = backend.build_bvh_host(s)
    monkeypatch.setenv("RPTR_REBRAID", str(braid))
    nodes, tris, insts, need = backend.build_bvh_host(s)
    n_records = insts.size // 32
    assert insts1.size // 32 == len(s.instances) and len(s.instances) < n_records <= braid * len(s.instances)
    ids = insts.view(np.int32).reshape(-1, 32)[:, 14]          # RptrBvhInstance.instance_id
    assert set(ids.tolist()) == set(range(len(s.instances)))
    osc = O.OracleScene(s)
    osc.import_bvh(nodes, tris, insts)
    o, d = _rays(6000, 9, -6, 6)
    tuv_b, ids_b = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_BRUTE)
    tuv_t, ids_t = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_IMPORTED)
    assert np.array_equal(tuv_b.view(np.uint32), tuv_t.view(np.uint32)) and np.array_equal(ids_b, ids_t)
    any_b = osc.trace_ex(o, d, 1e-4, 3.0, any_hit=True, bvh_mode=O.BVH_BRUTE)[1][:, 0]
    any_t = osc.trace_ex(o, d, 1e-4, 3.0, any_hit=True, bvh_mode=O.BVH_IMPORTED)[1][:, 0]
    assert np.array_equal(any_b, any_t)


def test_alpha_flags_of_the_host_built_tree():
    """RPTR_BVH_TRI_ALPHA marks exactly the triangles that some parameterized mesh gives an alpha-tested material"""
    s = scenes.alpha_test()
    nodes, tris, insts, _ = backend.build_bvh_host(s)
    t = np.frombuffer(np.ascontiguousarray(tris).tobytes(), dtype=np.uint32).reshape(-1, 12)
    flags = t[:, 11]
    expect = 8 + 2 + int(np.isin(s.pmeshes[2].tri_material_ids, (0, 1)).sum()) + 2        # screens, mixed, literal quad
    assert int(flags.sum()) == expect and set(np.unique(flags)) <= {0, 1}
    # the oracle walking this tree gives the oracle's own image up to noise: a fractional alpha draws from the path's generator per
    # candidate met, and the two trees meet the candidates in different orders (the 4-wide tree's looked-up child order)
    osc = O.OracleScene(s)
    own, _ = osc.render(80, 60, 32)
    osc.import_bvh(nodes, tris, insts)
    imp, _ = osc.render(80, 60, 32, bvh_mode=O.BVH_IMPORTED)
    rmse = float(np.sqrt(np.mean((own[..., :3] - imp[..., :3]).astype(np.float64) ** 2)))
    assert rmse < 0.08 and abs(float(own[..., :3].mean()) - float(imp[..., :3].mean())) < 0.02 * float(own[..., :3].mean())


def test_flattened_tree_on_the_host(monkeypatch):
    """RPTR_FLATTEN=1: one tree over all instanced triangles in world space; every triangle names its instance record, the first
    record is the identity instance the top level refers to, the scene's own records follow"""
    s = scenes.two_level_test()
    monkeypatch.setenv("RPTR_FLATTEN", "1")
    nodes, tris, insts, need = backend.build_bvh_host(s)
    monkeypatch.setenv("RPTR_FLATTEN", "0")
    t = np.frombuffer(np.ascontiguousarray(tris).tobytes(), dtype=np.uint32).reshape(-1, 12)
    recs = np.frombuffer(np.ascontiguousarray(insts).tobytes(), dtype=np.int32).reshape(-1, 32)
    n_inst = len(s.instances)
    instanced = sum(sum(g.num_tris for g in s.geometries[s.meshes[s.pmeshes[i.pmesh].mesh].first_geometry:][:s.meshes[s.pmeshes[i.pmesh].mesh].num_geometries])
                    for i in s.instances)
    assert len(t) == instanced and len(recs) == n_inst + 1
    rec = t[:, 11] >> 8
    assert rec.min() == 1 and rec.max() == n_inst and len(np.unique(rec)) == n_inst
    assert recs[0, 15] & 1 and recs[0, 14] == -1                  # flags: RPTR_BVH_INSTANCE_FLAT; instance_id of the start record
    assert recs[1:, 14].tolist() == list(range(n_inst))           # the scene's records in instance order
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    assert np.array_equal(recs[0, :12].view(np.float32), ident)
    # the oracle walks it: same image as its own two-level tree up to the rounding of the pre-transformed triangles
    osc = O.OracleScene(s)
    own, _ = osc.render(80, 60, 2)
    osc.import_bvh(nodes, tris, insts)
    flat, st = osc.render(80, 60, 2, bvh_mode=O.BVH_IMPORTED, count=True)
    assert float(np.sqrt(np.nanmean((own[..., :3] - flat[..., :3]).astype(np.float64) ** 2))) < 5e-3
    nodes2, tris2, insts2, _ = backend.build_bvh_host(s)
    osc.import_bvh(nodes2, tris2, insts2)
    _, st2 = osc.render(80, 60, 2, bvh_mode=O.BVH_IMPORTED, count=True)
    assert st.nodes_closest < st2.nodes_closest                   # and with fewer node visits


def _surviving_area(nodes_f, first, count):
    """sum of the (dequantised) child boxes' half areas over all inner children of the node range: what the area-optimal collapse minimises
    (every binary node that survives as a wide node is a visit with probability ~ its area), up to the rounding of the 8-bit planes"""
    nd = nodes_f.view(NODE_DT)[first:first + count]
    step = np.ldexp(1.0, nd["exp"].astype(np.int32) - 127)[:, :, None]
    ext = (nd["qhi"].astype(np.float64) - nd["qlo"].astype(np.float64)) * step           # (n, 3, 4)
    area = ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0]          # (n, 4)
    return float(area[nd["child"] >= 0].sum())


@pytest.mark.parametrize("scene_fn,lo,hi", [(lambda: scenes.grid(64, 32), -30, 30), (lambda: scenes.soup(11, n_meshes=1, tris_per_mesh=900, n_instances=1), -4, 4),
                                            (lambda: scenes.forest(n_meshes=1, tris_per_tree=2000, n_instances=1, name="one-tree"), -6, 6)])
def test_collapse_rules_area_optimal_against_greedy(scene_fn, lo, hi, monkeypatch):
    """bvh_build.h collapse_bvh4: the default (COLLAPSE_OPTIMAL, dynamic programming over slot quotas) never keeps more box area in inner nodes than
    the greedy rule, makes fewer nodes, visits fewer on average -- and every rule gives brute force's answers with the same leaves"""
    s = scene_fn()
    o, d = _rays(5000, 9, lo, hi)
    out = {}
    for rule in ("greedy", "optimal", "even"):
        monkeypatch.setenv("RPTR_COLLAPSE", rule)
        nodes, tris, insts, _ = backend.build_bvh_host(s)
        osc = O.OracleScene(s)
        osc.import_bvh(nodes, tris, insts)
        tuv_b, ids_b = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_BRUTE)
        tuv_t, ids_t, visits = osc.trace_ex_counts(o, d, 1e-4, 1e20, bvh_mode=O.BVH_IMPORTED)
        assert np.array_equal(tuv_b.view(np.uint32), tuv_t.view(np.uint32)) and np.array_equal(ids_b, ids_t), rule
        n_nodes = len(nodes) // 16
        out[rule] = (n_nodes, _surviving_area(nodes, 1, n_nodes - 1), float(visits[:, 0].mean()), np.sort(tris.view(np.uint32).reshape(-1, 12), axis=0))
        osc.close()
    monkeypatch.delenv("RPTR_COLLAPSE")
    assert backend.build_bvh_host(s)[0].tobytes() == _rebuild(s, monkeypatch, "optimal")   # the default IS the optimal rule
    (ng, ag, vg, tg), (no, ao, vo, to) = out["greedy"], out["optimal"]
    print("nodes greedy %d optimal %d even %d | inner box area %.4g / %.4g | node visits per ray %.2f / %.2f / %.2f" % (ng, no, out["even"][0], ag, ao, vg, vo, out["even"][2]))
    assert np.array_equal(tg, to)                       # the same triangles (the collapse does not touch the leaves)
    assert no <= ng and ao <= ag * 1.02 and vo <= vg * 1.02   # (1.02: the areas are those of the 8-bit boxes, the rule minimises the float boxes')


def _rebuild(s, monkeypatch, rule):
    monkeypatch.setenv("RPTR_COLLAPSE", rule)
    b = backend.build_bvh_host(s)[0].tobytes()
    monkeypatch.delenv("RPTR_COLLAPSE")
    return b


def test_partially_flattened_scene_on_the_host(monkeypatch):
    """Round 5: a scene with a dynamic mesh keeps that mesh's instances two-level and flattens the instances of its STATIC meshes into one
    world-space tree, held by the top level as one identity instance (option "flatten" = auto; before, one dynamic mesh sent the whole scene
    down the two-level walk). Layout: the top level refers to 1 + (instances of dynamic meshes) records, none of them flagged
    RPTR_BVH_INSTANCE_FLAT; the scene's own records follow, record bias + i for instance i; the flat tree's triangles name them, the
    dynamic mesh's triangles name none. The oracle walks it: the hits of its own two-level walk (ids; t up to the rounding of the
    pre-transformed triangles)."""
    s = scenes.forest(n_meshes=3, tris_per_tree=300, n_instances=25, name="f")
    s.meshes[0].dynamic = True
    n_dyn = sum(1 for i in s.instances if s.pmeshes[i.pmesh].mesh == 0)
    assert 0 < n_dyn < len(s.instances) - 1
    monkeypatch.setenv("RPTR_FLATTEN", "-1")
    nodes, tris, insts, need = backend.build_bvh_host(s)
    monkeypatch.setenv("RPTR_FLATTEN", "0")
    nodes2, tris2, insts2, _ = backend.build_bvh_host(s)
    t = np.frombuffer(np.ascontiguousarray(tris).tobytes(), dtype=np.uint32).reshape(-1, 12)
    recs = np.frombuffer(np.ascontiguousarray(insts).tobytes(), dtype=np.int32).reshape(-1, 32)
    n_inst, bias = len(s.instances), 1 + n_dyn
    assert len(recs) == bias + n_inst and not (recs[:bias, 15] & 1).any()
    assert sorted(recs[:bias, 14].tolist()) == sorted([-1] + [k for k, i in enumerate(s.instances) if s.pmeshes[i.pmesh].mesh == 0])
    assert recs[bias:, 14].tolist() == list(range(n_inst))
    rec = t[:, 11] >> 8
    static = [k for k, i in enumerate(s.instances) if s.pmeshes[i.pmesh].mesh != 0]
    assert set(np.unique(rec[rec > 0]).tolist()) == {bias + k for k in static}
    dyn_tris = sum(g.num_tris for g in s.geometries[s.meshes[0].first_geometry:][:s.meshes[0].num_geometries])
    assert int((rec == 0).sum()) == dyn_tris                      # the dynamic mesh: ONE object-space tree, shared by its instances
    osc = O.OracleScene(s)
    o, d = _rays(6000, 5, -6, 6)
    osc.import_bvh(nodes2, tris2, insts2)
    tuv2, ids2 = osc.trace_ex(o, d, 1e-4, 1e20, bvh_mode=O.BVH_IMPORTED)
    osc.import_bvh(nodes, tris, insts)
    tuv, ids, visits = osc.trace_ex_counts(o, d, 1e-4, 1e20, bvh_mode=O.BVH_IMPORTED)
    same = (ids == ids2).all(axis=1)
    assert same.mean() > 0.999 and (ids2[:, 0] >= 0).sum() > 500
    hit = same & (ids2[:, 0] >= 0)
    assert np.allclose(tuv[hit, 0], tuv2[hit, 0], rtol=2e-5, atol=1e-6)
    dyn_hit = hit & np.isin(ids2[:, 0], [k for k in range(n_inst) if k not in static])
    assert dyn_hit.sum() > 10 and np.array_equal(tuv[dyn_hit].view(np.uint32), tuv2[dyn_hit].view(np.uint32))   # object-space triangles: the same bits
