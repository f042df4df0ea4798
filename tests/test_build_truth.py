"""The device tree build replayed stage by stage against an exact judge (tests/build_truth.py), and the wide tree's bytes -- host build, host refit, device build,
device refit -- predicted from its topology and the mesh.  Everything is compared with np.array_equal: the builders compute with plain IEEE arithmetic.

CPU leg: layer A against the host builder (fpt_debug_build_bvh, fpt_debug_refit_bvh), the stack model on every tree of the leg, the judge's self-checks and the judge's
own trees under test_wide_bvh.check_tree / check_containment.  GPU leg: the probe of the last device build (Renderer.debug_build_arrays) against layers A and B in both
device modes, pass by pass, and the twelve planted mistakes of the judge, each refused by the device's data on a named case (TEETH)."""
import copy
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene

import build_truth as bt
from test_wide_bvh import _soup, _build_raw, check_containment, check_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = bt.Judge()
# The largest mesh that is replayed whole (stages 1..5, both layers): the judge's replay of mode 2 plus the slot check, the stack model and the comparison of the wide
# children take about 1.5 s of numpy per mode at 3000 triangles (measured on one CPU core: replay 0.63 s, slot check 0.72 s, stack model 0.13 s, children 0.05 s)
FULL_REPLAY_CAP = 3000
SOUP_SIZES = (2, 3, 7, 8, 9, 13, 14, 15, 27, 28, 29, 63, 64, 65, 255, 256, 257, 600)
DEGENERATE = ("coincident40", "mixed600", "flat", "lattice", "scaled1e-25", "scaled1e19")


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------
def _mesh(tris):
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3); n = len(tris)
    vtx = np.zeros((3 * n, 4), np.float32); vtx[:, :3] = tris.reshape(-1, 3)
    idx = np.zeros((n, 4), np.int32); idx[:, :3] = np.arange(3 * n).reshape(n, 3)
    return idx, vtx


_MESHES = {}


def case_mesh(name):
    """(idx [n, 4] int32, vtx [m, 4] float32) of a named case; the shadow-mask word of the indices is set so that the records' mask column is exercised"""
    if name in _MESHES:
        return _MESHES[name]
    if name.startswith("soup"):
        n = int(name[4:]); idx, vtx = _soup(n, np.random.default_rng(1000 + n))
    elif name == "coincident40":          # all keys equal, zero centre extent on every axis
        idx, vtx = _mesh(np.tile(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), (40, 1, 1)))
    elif name == "mixed600":          # the soup of test_device_build_on_degenerate_soups, cut to 600: coincident, point-like and collinear triangles
        idx, vtx = _soup(600, np.random.default_rng(9), spread=1.0, size=0.05)
        vtx[:300, :3] = np.tile(np.float32([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [0.5, 0.6, 0.5]]), (100, 1))
        vtx[300:330, :3] = np.float32([0.25, 0.25, 0.25])
        vtx[330:360, :3] = np.tile(np.float32([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9], [0.5, 0.5, 0.5]]), (10, 1))
    elif name == "flat":          # every triangle in the plane z = 0: the box centres' z extent is exactly zero
        idx, vtx = _soup(500, np.random.default_rng(21), spread=1.0, size=0.03); vtx[:, 2] = 0.0
    elif name == "lattice":
        # box centres 1.25 + j / 16, j = 0..8 per axis, triangles symmetric about them by 1 / 64: every coordinate lies in [1, 2), one binade, so the pad rounds the same
        # way on both sides and the centre 0.5f lo + 0.5f hi is exact; (c - 1.25) / 0.5 = j / 8 is exact, the cell j * 2^18 a boundary, and j = 8 meets the clamp to 2097151.
        # The last two triangles are a pair of flat boxes laid out so that a leaf of the two costs exactly what the inner node costs (the cost row's <= decides)
        j = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 3)
        c = 1.25 + j / 16.0; d = 1.0 / 64
        tris = np.stack([c + d * np.array([-1, -1, -1]), c + d * np.array([1, 1, -1]), c + d * np.array([-1, 1, 1])], 1)
        f = np.float32; o = f(1.5 + 1 / 32)          # between the lattice's points; found by a search over the last bits of these six numbers with the judge's own arithmetic
        w, h, dx, dy, w2, h2 = (f(v) for v in (0.00391697883605957, 0.003920555114746094, 0.007943304255604744, 0.0039136409759521484, 0.0039299726486206055, 0.003922939300537109))
        x0, y0 = f(o + dx), f(o + dy)
        pair = [[[o, o, o], [f(o + w), o, o], [o, f(o + h), o]], [[x0, y0, o], [f(x0 + w2), y0, o], [x0, f(y0 + h2), o]]]
        idx, vtx = _mesh(np.concatenate([tris, np.float32(pair)]))
    elif name.startswith("scaled"):
        idx, vtx = _soup(600, np.random.default_rng(33), spread=1.0, size=0.01)
        if name == "scaled1e-25":
            vtx[:60, :3] = vtx[:60, :3] * np.float32(1e-3) + np.float32(0.5)          # a tight cluster: nodes small enough for the exponent clamp
        vtx[:, :3] = (vtx[:, :3].astype(np.float64) * float(name[6:])).astype(np.float32)
    elif name == "chain":          # the deep-chain mesh of test_builder_bounds_the_traversal_stack_on_a_deep_chain
        n = 1500
        k = np.arange(n, dtype=np.float64); sz = 1.03 ** k; ang = k * 0.7
        P = [np.stack([np.cos(ang + d), np.sin(ang + d), k * 1e-3], 1) * np.stack([sz, sz, np.ones(n)], 1) for d in (0.0, 2.1, 4.2)]
        vtx = np.zeros((3 * n, 4), np.float32); vtx[:, :3] = np.concatenate(P)
        idx = np.zeros((n, 4), np.int32); idx[:, 0] = np.arange(n); idx[:, 1] = n + np.arange(n); idx[:, 2] = 2 * n + np.arange(n)
    elif name == "cornell_glossy":
        s = scene.cornell_box("CornellBox-Glossy"); idx, vtx = s.vertex_indices.copy(), s.vertex_data.copy()
    elif name == "standin_sub":          # a sub-mesh of standin_small (bathroom_standin(0.08)): its first triangles up to the cap -- the room and the first objects -- over all of its vertices
        s = scene.bathroom_standin(0.08)
        idx, vtx = s.vertex_indices[:FULL_REPLAY_CAP].copy(), s.vertex_data.copy()
    elif name == "soup70000":
        idx, vtx = _soup(70000, np.random.default_rng(70))
    else:
        raise KeyError(name)
    idx = np.ascontiguousarray(idx, np.int32); vtx = np.ascontiguousarray(vtx, np.float32)
    if not name.startswith(("cornell", "standin")):
        idx[:, 3] = (np.arange(len(idx)) % 3).astype(np.int32)
    _MESHES[name] = (idx, vtx)
    return idx, vtx


def moved(vtx, seed=4, amount=0.02):
    rng = np.random.default_rng(seed)
    ext = float(np.max(vtx[:, :3].max(0) - vtx[:, :3].min(0)))
    out = vtx.copy(); out[:, :3] += (rng.standard_normal((len(vtx), 3)) * amount * ext).astype(np.float32)
    return out


def _scene_of(idx, vtx):
    s = copy.copy(scene.cornell_box("CornellBox-JP"))
    s.vertex_indices = idx; s.vertex_data = vtx; s.num_triangles = len(idx); s.num_vertices = len(vtx)
    s.material_indices = (np.arange(len(idx)) % len(s.materials)).astype(np.int32); s.texture_indices_comp = None
    s.bbox = (vtx[:, :3].min(0), vtx[:, :3].max(0))
    return s


# ---- what a wide tree is held to (layer A), whoever built it ------------------------------------------------------------------------------------------------------
def judge_wide_tree(label, idx, vtx, nodes, recs, stack_need, watertight=False, judge=J, slot_sample=None, rays=300):
    """bytes from topology, numbering, the stack rule and the stack model, the slot check; -> (prediction, slot checks decided uniquely)"""
    pred = judge.predict_from(idx, vtx, nodes, recs, watertight)
    T = pred["topology"]
    assert judge.check_numbering(T) == len(recs) == len(idx)
    assert np.array_equal(np.sort(recs[:, 9].view(np.int32)), np.arange(len(idx))), label
    assert np.array_equal(pred["records"].view(np.uint32), np.asarray(recs, np.float32).view(np.uint32)), label + ": records"
    bad = np.argwhere(pred["nodes"] != nodes)
    assert not len(bad), "%s: %d node words differ from the bytes the topology and the mesh give, first (node, word) %s: %08x, judge %08x" % (
        label, len(bad), bad[0], nodes[tuple(bad[0])], pred["nodes"][tuple(bad[0])])
    need = judge.stack_need_rule(T)
    assert int(need[0]) == stack_need, "%s: stack_need %d, the builders' rule gives %d" % (label, stack_need, need[0])
    model = judge.stack_model_max(T, bt.decode_boxes(nodes), rays)
    print("%s: stack model %d, stack_need %d, gap %d" % (label, model, stack_need, stack_need - model))
    assert model <= stack_need, "%s: a ray can need %d stack entries, the builder's bound is %d" % (label, model, stack_need)
    unique = judge.slot_check_nodes(pred, slot_sample)
    return pred, unique


# ---- CPU leg ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_judge_self_checks():
    """the judge against plainer forms of itself: the subset table of the treelet kernel, the exponent's definition by search, the radix tree by recursion on the
    minimum, the exact placement search against every placement one by one, ordered ints"""
    src = open(os.path.join(ROOT, "fermat_amd", "csrc", "fpt_build_lbvh.hip")).read()
    table = [int(x) for x in re.search(r"c_trbvh_subsets\[120\]\s*=\s*\{([^}]*)\}", src).group(1).replace("\n", " ").split(",")]
    assert table == [s for subs in bt.Judge.SUBSETS for s in subs] and len(table) == 120
    for S, P in bt.Judge.PARTS.items():
        assert len(P) == 2 ** (bin(S).count("1") - 1) - 1 and all(p & (S & -S) and p & ~S == 0 and p != S for p in P) and list(P) == sorted(P)
    rng = np.random.default_rng(2)
    ext = np.concatenate([np.ldexp(rng.random(400) + 0.5, rng.integers(-140, 130, 400)), np.ldexp(255.0, np.arange(-110, 125)), [0.0, -1.0, 255.0, np.nextafter(255.0, 300)]])
    for x, e in zip(ext, J.grid_exponent(ext)):
        want = next((k for k in range(-100, 121) if x / np.ldexp(1.0, k) <= 255.0), 120) if x > 0 else -100
        assert e == want, (x, e, want)
    f = np.float32([0.0, -0.0, 1.0, -1.0, 3e38, -3e38, 1e-40, -1e-40])
    o = bt.ordered(f); assert np.array_equal(bt.unordered(o).view(np.uint32), f.view(np.uint32)) and (np.diff(o[np.argsort(f[2:])+ 2]) > 0).all() and o[1] < o[0]
    for n in (2, 3, 5, 17, 64):          # radix tree: split = the unique minimum of delta over the range, found by plain recursion; duplicates included
        keys = np.sort(rng.integers(0, 6, n).astype(np.uint64) << np.uint64(rng.integers(0, 50)))
        left, right = J.radix_tree(keys)

        def delta(i):
            a, b = int(keys[i]), int(keys[i + 1])
            return 64 - (a ^ b).bit_length() if a != b else 64 + 32 - (i ^ (i + 1)).bit_length()

        def rec(l, r, node):
            s = min(range(l, r), key=delta)
            assert sum(delta(i) == delta(s) for i in range(l, r)) == 1
            assert left[node] == (~s if s == l else s) and right[node] == (~(s + 1) if s + 1 == r else s + 1)
            assert node in (l, r)
            if s > l:
                rec(l, s, s)
            if s + 1 < r:
                rec(s + 1, r, s + 1)
        rec(0, n - 1, 0)
    for n in (1, 2, 4, 5):
        sc = rng.normal(size=(n, 8)); sc[0, 1] = sc[0, 2]; sc[n - 1, 5] = sc[0, 5]
        b = J.best_placement(sc); br = J.slot_check_brute(sc)
        from fractions import Fraction
        assert Fraction(b[0], b[5]) == br[0] and (None if b[1] is None else Fraction(b[1], b[5])) == br[1] and b[2] == br[2]
        assert sum(Fraction(float(sc[c][s])) for c, s in enumerate(b[3])) == br[0]
    # a unique best placement is demanded, a worse one refused
    box = np.float32([[0, 0, 0, 1, 1, 1], [2, 2, 2, 3, 3, 3]]); nb = np.float32([0, 0, 0, 3, 3, 3])
    assert J.slot_check(box, nb, [0, 7]) == "unique"
    with pytest.raises(AssertionError):
        J.slot_check(box, nb, [7, 0])


CPU_CASES = ("soup2", "soup9", "soup65", "soup600", "coincident40", "mixed600", "flat", "lattice", "scaled1e-25", "scaled1e19", "chain", "cornell_glossy", "standin_sub")


def _host(idx, vtx, vtx1=None):
    L = fa.lib()
    nn, nr, dp, nw = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    st = fa.api.BvhStats()
    a = (C.c_uint32(len(idx)), C.c_void_p(idx.ctypes.data), C.c_uint32(len(vtx)), C.c_void_p(vtx.ctypes.data))
    if vtx1 is None:
        rc, nn_, nr_, st, nodes, recs = _build_raw(idx, vtx, want_arrays=True)
        assert rc == 0
        return nodes, recs, st
    vtx1 = np.ascontiguousarray(vtx1, np.float32)
    a = a + (C.c_void_p(vtx1.ctypes.data),)
    assert L.fpt_debug_refit_bvh(*a, C.byref(nn), C.byref(nr), C.byref(dp), None, None, C.byref(st)) == 0, L.fpt_last_error(None)
    nodes = np.zeros((nn.value, 20), np.uint32); recs = np.zeros((nr.value, 12), np.float32)
    assert L.fpt_debug_refit_bvh(*a, C.byref(nn), C.byref(nr), C.byref(dp), C.c_void_p(nodes.ctypes.data), C.c_void_p(recs.ctypes.data), None) == 0
    return nodes, recs, st.as_dict()


@pytest.mark.parametrize("name", CPU_CASES)
def test_layer_a_against_the_host_builder(name):
    """build_wide8 and refit_wide8 are documented as the device kernels' arithmetic: the host tree's bytes, and those of its refit to moved vertices and to the same
    vertices, are the ones layer A predicts from the topology -- boxes bottom-up, exponents by their definition, qlo / qhi the tightest grid values --, the records
    follow the mesh, stack_need is the rule's, no hit set of the stack model needs more than it, and every node's slots hold the best placement.

    Stack gap (stack_need - the model's largest stack pointer, printed per tree), largest observed: 5, on `chain` (46 against 41); 0 on most soups, 1 on the smallest
    soups, coincident40, cornell_glossy and standin_sub; the device trees of the GPU leg: 0..2.  The rule charges every leaf-bearing node of a path one parked triangle
    group.  The kernel parks the group in hand only when a node step brings triangles while some are still pending, and it tests one triangle in the iteration that
    brings a group: a group of one triangle is never parked (the chain mesh's SAH tree peels one triangle per level), the root has nothing in hand to park, and the
    triangles of a path's last leaf-bearing node are parked only when a sibling taken from the stack brings triangles of its own."""
    idx, vtx = case_mesh(name)
    nodes, recs, st = _host(idx, vtx)
    pred, unique = judge_wide_tree("host/" + name, idx, vtx, nodes, recs, st["stack_need"])
    hist = np.bincount(pred["used"].sum(1), minlength=9)
    assert st["slot_hist"] == hist.tolist() and st["depth"] == len(pred["topology"]["levels"]) - 1
    assert st["inner_children"] == int(pred["topology"]["inner"].sum()) and st["leaf_children"] == int((pred["topology"]["tris"] > 0).sum())
    if name in ("soup65", "soup600", "mixed600", "scaled1e-25", "scaled1e19", "cornell_glossy", "standin_sub"):          # (flat, chain, coincident: every placement has its mirror image)
        assert unique >= 1, "no slot check of this tree was decided uniquely"
    for label, v1 in (("moved", moved(vtx)), ("same", vtx)):
        n1, r1, st1 = _host(idx, vtx, v1)
        assert np.array_equal(n1[:, 4:8], nodes[:, 4:8]) and np.array_equal(r1[:, 9].view(np.int32), recs[:, 9].view(np.int32))
        p1 = J.predict_from(idx, v1, n1, r1)
        assert np.array_equal(p1["nodes"], n1) and np.array_equal(p1["records"].view(np.uint32), r1.view(np.uint32)), "host refit (%s) of %s" % (label, name)
        if label == "same":
            assert np.array_equal(n1, nodes) and np.array_equal(r1.view(np.uint32), recs.view(np.uint32)), "a refit to the same vertices changes the tree"
    assert check_containment(nodes, recs) >= len(nodes)


def test_host_watertight_records_and_identical_nodes():
    """a watertight tree's records hold the vertices; its nodes are byte-identical (layer A with the intersector as input)"""
    idx, vtx = case_mesh("cornell_glossy")
    nodes, recs, st = _host(idx, vtx)
    p = J.predict_from(idx, vtx, nodes, recs, watertight=True)
    assert np.array_equal(p["nodes"], nodes)
    tri = idx[recs[:, 9].view(np.int32)][:, :3]
    assert np.array_equal(p["records"][:, 3:6], vtx[tri[:, 1], :3]) and np.array_equal(p["records"][:, 6:9], vtx[tri[:, 2], :3])


GPU_FULL = tuple("soup%d" % n for n in SOUP_SIZES) + DEGENERATE + ("cornell_glossy", "standin_sub")


@pytest.mark.parametrize("name", GPU_FULL)
def test_the_judges_own_tree_is_a_valid_tree(name, table):
    """layer B completed by an optimal slot assignment, in both device modes: a tree over every triangle whose boxes contain what is below them
    (check_containment), holding the children stage 5 gathers; for the real scenes also test_wide_bvh.check_tree against the oracle's closest hits (the soups do not
    meet check_tree's own demand that most of its random rays hit something)"""
    idx, vtx = case_mesh(name)
    assert len(idx) <= FULL_REPLAY_CAP
    for mode in (1, 2):
        t0 = time.time()
        S = J.replay(idx, vtx, mode)
        nodes, recs, need, depth, pred = J.wide_tree(S, idx, vtx)
        took = time.time() - t0
        assert J.check_numbering(pred["topology"]) == len(idx) and np.array_equal(np.sort(recs[:, 9].view(np.int32)), np.arange(len(idx)))
        assert check_containment(nodes, recs) >= len(nodes) and J.same_children(S, pred) == len(nodes)
        assert J.stack_model_max(pred["topology"]) <= need
        if name in ("cornell_glossy", "standin_sub"):
            check_tree(_scene_of(idx, vtx), nodes, recs, min(need, 48), table, 150, 3)
        assert took < 5.0, "the judge's replay of %s took %.1f s" % (name, took)
        if mode == 2 and len(idx) >= 7:
            assert sum(p["rewritten"] + p["kept"] for p in S["passes"]) >= 1


def test_the_stack_model_can_catch_a_short_bound():
    """the planted mistake `need_no_leaf` (the rule without its leaf term): the model must exceed the mutated bound on some tree -- the only evidence that the model
    could ever catch a bound that is one short.  CPU half of TEETH['need_no_leaf']"""
    idx, vtx = case_mesh("soup600")
    nodes, recs, st = _host(idx, vtx)
    T = J.predict_from(idx, vtx, nodes, recs)["topology"]
    short = int(bt.Judge({"need_no_leaf"}).stack_need_rule(T)[0])
    assert short < st["stack_need"] and J.stack_model_max(T) > short


# ---- GPU leg ---------------------------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("FPT_BVH_BUILD", raising=False); monkeypatch.delenv("FPT_INTERSECTOR", raising=False)


class Device:
    """one context for every device build of this module: meshes go to the device as they come, fpt_rt_create_geometry / fpt_rt_refit_geometry are called on them"""
    def __init__(self, table):
        self.r = fa.Renderer(scene.cornell_box("CornellBox-JP"), 16, 16, fa.default_options(2), table=table)
        self.cache = {}

    def build(self, idx, vtx, mode, watertight=False, passes=None):
        r = self.r; t = r.torch
        self.d_idx = t.from_numpy(idx).to(r.dev); self.d_vtx = t.from_numpy(vtx).to(r.dev); t.cuda.synchronize(r.dev)
        r.set_build_mode(mode); r.set_intersector(1 if watertight else 0)
        if passes is not None:
            r.debug_set_treelet_passes(passes)
        r._check(r.L.fpt_rt_create_geometry(r.ctx, C.c_uint32(len(idx)), C.c_void_p(self.d_idx.data_ptr()), C.c_uint32(len(vtx)), C.c_void_p(self.d_vtx.data_ptr())))
        nodes, recs = r.download_bvh()
        return dict(nodes=nodes, recs=recs, stats=r.bvh_stats(), arrays=r.debug_build_arrays(), mode=mode)

    def refit(self, idx, vtx1):
        r = self.r; t = r.torch
        self.d_vtx = t.from_numpy(np.ascontiguousarray(vtx1, np.float32)).to(r.dev); t.cuda.synchronize(r.dev)
        r._check(r.L.fpt_rt_refit_geometry(r.ctx, C.c_uint32(len(idx)), C.c_void_p(self.d_idx.data_ptr()), C.c_uint32(len(vtx1)), C.c_void_p(self.d_vtx.data_ptr())))
        return r.download_bvh()

    def case(self, name, mode):
        if (name, mode) not in self.cache:
            self.cache[name, mode] = self.build(*case_mesh(name), mode)
        return self.cache[name, mode]


@pytest.fixture(scope="module")
def device(table):
    d = Device(table)
    yield d
    d.r.close()


def replay_differences(judge, idx, vtx, B, passes=3, upto=5):
    """layer B against the probe's arrays: the names of the stages whose arrays differ from the judge's (empty: the device build is the judge's, bit for bit)"""
    A = B["arrays"]; mode = B["mode"]; diff = []
    S = judge.replay(idx, vtx, mode, passes, upto)
    eq = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if not eq(S["refs"], A["refs"]): diff.append("refs")
    if not eq(S["bounds"], A["bounds"]): diff.append("bounds")
    if not eq(S["keys"], A["keys"]): diff.append("keys")
    if not eq(S["vals"], A["vals"]): diff.append("vals")
    if upto < 3:
        return diff, S
    if upto < 4:
        if not (eq(S["left"], A["left"]) and eq(S["right"], A["right"])): diff.append("tree")
        return diff, S
    if not (eq(S["left"], A["left"]) and eq(S["right"], A["right"])): diff.append("tree")
    if not eq(S["node_box"], A["node_box"]): diff.append("node_box")
    for f in ("c", "k", "k8", "leaf", "count"):
        if not eq(np.ascontiguousarray(S["cells"][f]), np.ascontiguousarray(A["cells"][f])): diff.append("cells." + f)
    if mode == 2:
        if not np.array_equal(S["tcount_final"], A["tcount"]): diff.append("tcount")
        if not eq(S["tcost_final"], A["tcost"]): diff.append("tcost")
    if S["depth_binary"] != A["depth_binary"]: diff.append("depth_binary")
    return diff, S


def full_replay(label, idx, vtx, B, watertight=False, passes=3, slot_sample=None):
    """everything the probe returns and every node and record byte; -> (stage-5 state, prediction, unique slot checks)"""
    A = B["arrays"]; st = B["stats"]
    assert A["n"] == len(idx) and A["mode"] == B["mode"] and A["nodes"] == len(B["nodes"]) and A["passes"] == (passes if B["mode"] == 2 else 0)
    diff, S = replay_differences(J, idx, vtx, B, passes)
    assert not diff, "%s: the device build differs from the judge's replay in %s" % (label, diff)
    pred, unique = judge_wide_tree(label, idx, vtx, B["nodes"], B["recs"], st["stack_need"], watertight, slot_sample=slot_sample)
    assert np.array_equal(J.stack_need_rule(pred["topology"]), A["need"].astype(np.int64)), label + ": need"
    assert J.same_children(S, pred) == len(B["nodes"])
    # statistics
    T = pred["topology"]
    assert st["nodes"] == T["N"] and st["records"] == len(idx) and st["depth"] == len(T["levels"]) - 1, (label, st)
    assert st["slot_hist"] == np.bincount(pred["used"].sum(1), minlength=9).tolist(), (label, st)
    assert st["inner_children"] == int(T["inner"].sum()) == T["N"] - 1 and st["leaf_children"] == int((T["tris"] > 0).sum()), (label, st)
    if B["mode"] == 2:
        assert st["depth_binary"] == S["depth_binary"] and st["optimise_iterations"] == passes, (label, st)
    return S, pred, unique


def refit_check(device, label, idx, vtx, B, watertight=False):
    v1 = moved(vtx)
    n1, r1 = device.refit(idx, v1)
    assert np.array_equal(n1[:, 4:8], B["nodes"][:, 4:8])
    p = J.predict_from(idx, v1, n1, r1, watertight)
    assert np.array_equal(p["nodes"], n1) and np.array_equal(p["records"].view(np.uint32), r1.view(np.uint32)), label + ": the device refit's bytes"


@gpu
@pytest.mark.parametrize("name", tuple("soup%d" % n for n in SOUP_SIZES))
def test_device_build_full_replay(name, device):
    """a lone root (2..8), the first treelet at gamma = 7, the gamma thresholds 14 and 28, the wave boundary (64) and the block boundary (256) of the references kernel"""
    idx, vtx = case_mesh(name)
    for mode in (1, 2):
        full_replay("%s/mode%d" % (name, mode), idx, vtx, device.case(name, mode))


@gpu
@pytest.mark.parametrize("name", DEGENERATE)
def test_device_build_ties_and_degeneracies(name, device):
    idx, vtx = case_mesh(name)
    for mode in (1, 2):
        B = device.case(name, mode)
        S, pred, unique = full_replay("%s/mode%d" % (name, mode), idx, vtx, B)
        keys = B["arrays"]["keys"]
        if name == "coincident40":
            assert (keys == keys[0]).all() and (B["arrays"]["bounds"][6:9] == B["arrays"]["bounds"][9:12]).all()
        if name == "mixed600":
            assert (np.diff(keys) == 0).sum() >= 99
        if name == "flat":
            assert B["arrays"]["bounds"][8] == B["arrays"]["bounds"][11] and B["arrays"]["bounds"][6] != B["arrays"]["bounds"][9]
        if name == "lattice":
            q = S["cells_q"][:729]
            assert (q % (1 << 18) == 0).sum() + (q == 2097151).sum() == q.size and (q == 2097151).any() and (q == 0).any(), "the lattice's centres are not on cell boundaries"
        if name == "scaled1e-25":
            assert (pred["exponents"] == -100).any(), "no exponent at the clamp"


@gpu
@pytest.mark.parametrize("name", ("cornell_glossy", "standin_sub"))
def test_device_build_real_scenes_and_refit(name, device):
    idx, vtx = case_mesh(name)
    assert len(idx) <= FULL_REPLAY_CAP
    for mode in (1, 2):
        B = device.build(idx, vtx, mode)
        full_replay("%s/mode%d" % (name, mode), idx, vtx, B)
        refit_check(device, "%s/mode%d+refit" % (name, mode), idx, vtx, B)
        if name == "cornell_glossy":          # both intersectors: a watertight tree's records hold the vertices, its nodes are byte-identical
            W = device.build(idx, vtx, mode, watertight=True)
            assert np.array_equal(W["nodes"], B["nodes"]) and not np.array_equal(W["recs"], B["recs"])
            full_replay("%s/mode%d/watertight" % (name, mode), idx, vtx, W, watertight=True)
            refit_check(device, "%s/mode%d/watertight+refit" % (name, mode), idx, vtx, W, watertight=True)


@gpu
def test_device_build_large(device):
    """70 000 triangles: the bounds fold over more than 256 partials, keys, sort, the radix tree against the Cartesian-tree judge (stages 1..3), and layer A on the whole
    tree -- boxes from topology, the stack condition -- with the slot check on a sample of 2 000 nodes"""
    idx, vtx = case_mesh("soup70000")
    assert (len(idx) + 255) // 256 > 256
    B = device.build(idx, vtx, 1)
    diff, S = replay_differences(J, idx, vtx, B, upto=3)
    assert not diff, diff
    sample = np.random.default_rng(5).choice(len(B["nodes"]), 2000, replace=False)
    pred, unique = judge_wide_tree("soup70000/mode1", idx, vtx, B["nodes"], B["recs"], B["stats"]["stack_need"], slot_sample=sample, rays=40)
    assert np.array_equal(J.stack_need_rule(pred["topology"]), B["arrays"]["need"].astype(np.int64)) and unique >= 1000
    B2 = device.build(idx, vtx, 2)          # mode 2: the radix tree has been restructured in the scratch; stages 1..2 and layer A remain
    diff, _ = replay_differences(J, idx, vtx, B2, upto=2)
    assert not diff, diff
    sample = np.random.default_rng(6).choice(len(B2["nodes"]), 200, replace=False)
    judge_wide_tree("soup70000/mode2", idx, vtx, B2["nodes"], B2["recs"], B2["stats"]["stack_need"], slot_sample=sample, rays=0)


@gpu
def test_device_build_pass_by_pass(device):
    """mode 2 with 0, 1, 2, 3 treelet passes on the 600-soup: 0 passes give mode 1's tree, every step is the judge's; the override lasts one build"""
    idx, vtx = case_mesh("soup600")
    one = device.case("soup600", 1)
    trees = []
    for p in (0, 1, 2, 3):
        B = device.build(idx, vtx, 2, passes=p)
        full_replay("soup600/mode2/%d passes" % p, idx, vtx, B, passes=p)
        trees.append(B)
    A0 = trees[0]["arrays"]
    assert np.array_equal(A0["left"], one["arrays"]["left"]) and np.array_equal(A0["right"], one["arrays"]["right"]) and np.array_equal(trees[0]["nodes"], one["nodes"])
    assert not np.array_equal(trees[1]["arrays"]["left"], A0["left"]) and not np.array_equal(trees[2]["arrays"]["left"], trees[1]["arrays"]["left"])
    again = device.build(idx, vtx, 2)
    assert again["arrays"]["passes"] == 3 and np.array_equal(again["nodes"], trees[3]["nodes"])


@gpu
def test_device_build_statistics_and_non_vacuity(device):
    """bvh_stats of a device build equals the judge's counts (full_replay asserts it per case); and the cases really exercise what they are there for"""
    idx, vtx = case_mesh("soup600")
    B = device.case("soup600", 2)
    S, pred, unique = full_replay("soup600/mode2", idx, vtx, B)
    st = B["stats"]
    assert st["stack_need"] == int(J.stack_need_rule(pred["topology"])[0]) and st["depth_binary"] == S["depth_binary"] == B["arrays"]["depth_binary"]
    assert sum(p["rewritten"] for p in S["passes"]) >= 1 and sum(p["kept"] for p in S["passes"]) >= 1          # a treelet rewritten, one left alone
    T = pred["topology"]
    assert (T["tris"] == 2).any(), "no two-triangle leaf"
    used = pred["used"].sum(1)
    assert (used < 8).any() and (used == 8).any()
    assert unique >= 1, "no slot check decided uniquely"
    for name in ("coincident40", "mixed600"):          # equal keys
        assert (np.diff(device.case(name, 1)["arrays"]["keys"]) == 0).any()
    i2, v2 = case_mesh("scaled1e-25")
    assert (J.predict_from(i2, v2, device.case("scaled1e-25", 1)["nodes"], device.case("scaled1e-25", 1)["recs"])["exponents"] == -100).any()


@gpu
def test_the_probe_never_returns_stale_memory(device, table):
    r = fa.Renderer(scene.cornell_box("CornellBox-JP"), 16, 16, fa.default_options(2), table=table)
    with pytest.raises(fa.FptError, match="no device build"):          # a host build leaves nothing to probe
        r.debug_build_arrays()
    r.set_build_mode(1); r.rebuild_geometry()
    A = r.debug_build_arrays()
    assert A["n"] == r.scene.num_triangles and "tcount" not in A
    buf = np.zeros(4, np.uint8)
    assert r.L.fpt_debug_device_build(r.ctx, C.c_uint32(1), C.c_void_p(buf.ctypes.data), C.c_uint64(4)) != 0 and b"size" in r.L.fpt_last_error(r.ctx)
    assert r.L.fpt_debug_device_build(r.ctx, C.c_uint32(10), C.c_void_p(buf.ctypes.data), C.c_uint64(4)) != 0          # tcount: mode 2 only
    assert r.L.fpt_debug_device_build(r.ctx, C.c_uint32(12), C.c_void_p(buf.ctypes.data), C.c_uint64(4)) != 0
    assert r.L.fpt_debug_device_build(r.ctx, C.c_uint32(104), None, C.c_uint64(0)) != 0
    r.set_build_mode(0)          # releases the scratch
    with pytest.raises(fa.FptError, match="no device build"):
        r.debug_build_arrays()
    r.close()


# the planted mistakes: mutation -> (case, mode, the stage of the replay or the check that must refuse it)
TEETH = {
    "swap_xz": ("soup600", 1, "keys"), "round_cell": ("soup600", 1, "keys"), "no_tiebreak": ("coincident40", 1, "tree"),
    "dp_tie_larger": ("lattice", 2, "tree"), "treelet_leaf_limit": ("soup600", 2, "tcost"), "c_prim_half": ("soup600", 1, "cells.c"),
    "leaf_strict": ("lattice", 1, "cells.leaf"), "k8_from_k6": ("soup600", 1, "cells.k8"), "exp_plus_one": ("soup600", 1, "nodes"),
    "qlo_nearest": ("soup600", 1, "nodes"), "pad_no_scene": ("soup600", 1, "refs"), "need_no_leaf": ("soup600", 1, "stack")}


@gpu
@pytest.mark.parametrize("mutation", bt.MUTATIONS)
def test_the_judge_has_teeth(mutation, device):
    """the device code cannot be mutated inside a test, so the judge is: each planted mistake must be refused by the device's data on its named case"""
    name, mode, where = TEETH[mutation]
    idx, vtx = case_mesh(name)
    B = device.case(name, mode)
    assert not replay_differences(J, idx, vtx, B)[0]
    M = bt.Judge({mutation})
    if where == "nodes":
        assert not np.array_equal(M.predict_from(idx, vtx, B["nodes"], B["recs"])["nodes"], B["nodes"])
    elif where == "stack":
        T = J.predict_from(idx, vtx, B["nodes"], B["recs"])["topology"]
        short = M.stack_need_rule(T)
        assert not np.array_equal(short, B["arrays"]["need"].astype(np.int64)) and J.stack_model_max(T) > int(short[0]), "the stack model cannot tell a short bound"
    else:
        assert where in replay_differences(M, idx, vtx, B, upto=4)[0], "%s is not refused by %s in mode %d" % (mutation, name, mode)
