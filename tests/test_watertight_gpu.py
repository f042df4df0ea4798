"""The watertight traversal kernels (fermat_amd/csrc/fpt_trace_wt.hip) on the GPU: an acceleration structure built for fpt-WT (Renderer.set_intersector(1)).

  1. kernel = specification: t, triangle, u, v of closest hits, the occlusion flag of any hits and trace_shadow_bits equal tests/watertight_spec.py's float32
     brute force BIT FOR BIT on the quality, fast and trbvh trees and after a device refit -- so the answers are a function of the ray and the triangles alone.
     The far300 sets, beyond the stated guarantee of tree independence, go through the fp64 judge only.
  2. the guarantee: rays cast from inside the two closed meshes at their shared edges and vertices all report a hit and none slips past its closest crossing,
     on every tree and after the refit.  The default intersector on the same rays is the control (printed, not asserted).
  3. ownership: the intersector is the tree's.  A request alone changes nothing, a rebuild changes tree and description together, a refused build leaves both,
     FPT_INTERSECTOR overrides the request.
  4. the three renderers on a watertight tree: finite frames, passes in flight bit-identical to sequential passes, the frame's mean next to the default's.
  5. the C++ mirror's `-intersector watertight`.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene

import test_trace_truth as ttt
import test_watertight_spec as tws
import trace_truth as tt
import watertight_spec as wt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TREES = ["quality", "fast", "trbvh", "quality+refit"]
EXACT = [n for n in sorted(ttt.CLOSEST) if not n.endswith("/far300")]          # origins within 30 scene magnitudes: answers do not depend on the tree
JUDGED = [n for n in sorted(ttt.CLOSEST) if n.endswith("/far300")]
# Sets aimed from inside at the edges and vertices of the closed meshes AFTER the refit moved them (and the move made them non-convex): seen from inside, some of those
# edges are silhouettes, where fpt-WT promises a hit but not the fp64 answer.  Slips to a farther hit, measured with the specification (which the kernel
# equals bit for bit): 7, 1, 16, 4; bounded at twice that, at least 2, as tests/test_trace_truth.py bounds its own.  Rays without a hit: 0, no allowance.
MOVED_SLIP_BOUND = {"icosphere/edges": 14, "icosphere/vertices": 2, "fan_room/edges": 32, "fan_room/vertices": 8}


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    """the tests choose intersector and build mode themselves"""
    monkeypatch.delenv("FPT_INTERSECTOR", raising=False)
    monkeypatch.delenv("FPT_BVH_BUILD", raising=False)


def _moved_welded(s):
    """test_trace_truth._moved for a CLOSED mesh.  A Scene keeps three vertices of its own per triangle, so moving every vertex on its own tears a closed mesh
    open along every edge (a third of the inside rays then really leave it, in the fp64 truth too): corners that coincide move together, by the displacement of the first"""
    _, first, inverse = np.unique(s.vertex_data[:, :3], axis=0, return_index=True, return_inverse=True)
    return ttt._moved(s)[first[inverse.ravel()]]


def _renderer(s, tree, table, intersector=fa.INTERSECTOR_WATERTIGHT, moved=ttt._moved):
    """an 8 x 8 context whose tree was built for `intersector` by the named builder; "+refit": every vertex moved as test_trace_truth._moved does, device refit.
    Returns the renderer and the scene the tree now stands for."""
    r = fa.Renderer(s, 8, 8, fa.default_options(2), table=table)
    r.set_intersector(intersector)
    r.set_build_mode({"quality": 0, "fast": 1, "trbvh": 2}[tree.split("+")[0]])
    r.rebuild_geometry()
    assert r.intersector() == (intersector, intersector)
    if tree.endswith("+refit"):
        s = ttt._with_vertices(s, moved(s))
        r.refit_geometry(s.vertex_data)
        assert r.intersector() == (intersector, intersector)          # a refit keeps the tree's own
    return r, s


@functools.lru_cache(maxsize=None)
def _moved_scene(key, masked=False):
    """the scene of a case after test_trace_truth._moved (what "+refit" refits to), one object per scene so that the specification below is evaluated once"""
    s = ttt.masked(ttt.get_scene(key)) if masked else ttt.get_scene(key)
    return ttt._with_vertices(s, ttt._moved(s))


@functools.lru_cache(maxsize=None)
def _spec_moved(name):
    """the specification on the moved vertices: a closest-hit case of test_trace_truth by name, an inside set as (key, what), an any-hit case as ("any", key)"""
    if isinstance(name, tuple) and name[0] == "any":
        s = _moved_scene(name[1], True); _, rays, _ = ttt.any_case(name[1])
        return wt.occluded(s.vertex_indices, s.vertex_data, rays)
    if isinstance(name, tuple):
        s = _moved_scene(name[0]); _, rays, _ = tws.inside_case(*name)
    else:
        s = _moved_scene(ttt.CLOSEST[name][0]); _, rays, _ = ttt.closest_case(name)
    return wt.closest(s.vertex_indices, s.vertex_data, rays)


def _same_hits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)) for f in ("t", "triId", "u", "v"))


def _first_difference(a, b):
    bad = np.zeros(len(a), bool)
    for f in ("t", "triId", "u", "v"):
        bad |= np.ascontiguousarray(a[f]).view(np.uint32) != np.ascontiguousarray(b[f]).view(np.uint32)
    i = int(np.flatnonzero(bad)[0])
    return "%d of %d rays differ, e.g. ray %d: kernel %s, specification %s" % (bad.sum(), len(a), i, a[i], b[i])


@pytest.mark.parametrize("tree", TREES)
def test_kernel_equals_the_specification_bit_for_bit(tree, table):
    """every case on every tree; after the refit the same cases, with the specification evaluated again on the moved vertices (and the truth for the far300 sets)"""
    refit = tree.endswith("+refit")
    by_scene = {}
    for name in EXACT + JUDGED:
        by_scene.setdefault(ttt.CLOSEST[name][0], []).append(name)
    for key, what in tws.INSIDE:
        by_scene.setdefault(key, []).append((key, what))
    slips = {}
    for key, names in sorted(by_scene.items()):
        r, s = _renderer(ttt.get_scene(key), tree, table)
        for name in names:
            if isinstance(name, tuple):
                _, rays, T = tws.inside_case(*name); want = tws.spec_inside(*name); label = "%s/inside-%s" % name
            else:
                _, rays, T = ttt.closest_case(name); want = None if name in JUDGED else tws.spec_closest(name); label = name
            got = r.trace(rays)
            if refit:
                assert np.array_equal(s.vertex_data, _moved_scene(key).vertex_data)
                want = None if name in JUDGED else _spec_moved(name)
                T = tt.truth(s.vertex_indices, s.vertex_data, rays) if name in JUDGED else None
            if want is not None:
                assert _same_hits(got, want), "%s [%s]: %s" % (label, tree, _first_difference(got, want))
            else:
                slips[label] = ttt.judge_closest(s, rays, T, got, "%s [%s]" % (label, tree))
        r.close()
    for key in sorted(ttt.ANY):
        r, s = _renderer(ttt.masked(ttt.get_scene(key)), tree, table)
        _, rays, _ = ttt.any_case(key)
        want = _spec_moved(("any", key)) if refit else wt.occluded(s.vertex_indices, s.vertex_data, rays)
        h = r.trace(rays, shadow=True)
        occ = h["t"] > 0
        assert np.array_equal(occ, want), "any/%s [%s]: %d of %d occlusion flags differ from the specification" % (key, tree, (occ != want).sum(), len(rays))
        bits = r.trace_shadow_bits(rays)
        i = np.arange(len(rays))
        assert np.array_equal(((bits[i >> 5] >> (i & 31)) & 1).astype(bool), want), "any/%s [%s]: trace_shadow_bits differs from the specification" % (key, tree)
        r.close()
    print("far300 slips [%s]: %s" % (tree, slips))
    over = {k: v for k, v in slips.items() if v > ttt.SLIP_BOUND.get(k, 0)}
    assert not over, "slips over their bounds [%s]: %s" % (tree, over)


@pytest.mark.parametrize("tree", TREES)
def test_no_ray_leaves_a_closed_mesh(tree, table):
    """0 rays without a hit and 0 slips from inside, judged by the fp64 truth: the guarantee of DESIGN.md 9, no allowance.  After the refit the mesh has moved (and
    stayed closed: _moved_welded), the truth is recomputed on the moved vertices, and next to the sets of the unmoved mesh -- whose rays no longer meet edges or
    vertices -- the same sets are cast again at the edges and vertices of the moved mesh, which is where the refitted records have to be watertight"""
    control, moved_slips = {}, {}
    refit = tree.endswith("+refit")
    for key in ("icosphere", "fan_room"):
        r, s = _renderer(ttt.get_scene(key), tree, table, moved=_moved_welded)
        c, _ = _renderer(ttt.get_scene(key), tree, table, fa.INTERSECTOR_MT, moved=_moved_welded)
        for what, aimed_at_moved in [(w, a) for w in ("edges", "vertices") for a in ((False, True) if refit else (False,))]:
            _, rays, T = tws.inside_case(key, what)
            if aimed_at_moved:
                rays = tws.inside_rays(s, tws.INSIDE_COUNT[what], 43, what)
            if refit:
                T = tt.truth(s.vertex_indices, s.vertex_data, rays)
            assert (T["tri"] >= 0).all(), "the mesh is not closed around the origins"
            assert not aimed_at_moved or (~T["robust"]).mean() > 0.5
            label = "%s/inside-%s%s [%s]" % (key, what, " of the moved mesh" if aimed_at_moved else "", tree)
            got = r.trace(rays)
            escaped = int((got["triId"] < 0).sum())
            assert escaped == 0, "%s: %d of %d rays report no hit" % (label, escaped, len(rays))
            slips = ttt.judge_closest(s, rays, T, got, label)
            if aimed_at_moved:
                # silhouette edges of the moved mesh (MOVED_SLIP_BOUND): a farther hit, never none -- no ray leaves, asserted above
                moved_slips["%s/%s" % (key, what)] = slips
                assert slips <= MOVED_SLIP_BOUND["%s/%s" % (key, what)], (label, slips)
            else:
                assert slips == 0, "%s: %d rays slipped past their closest crossing" % (label, slips)
            mt = c.trace(rays)
            tie = (mt["triId"] >= 0) & (np.abs(mt["t"].astype(np.float64) - T["t"]) <= tt.MARGIN * T["terr"])
            control["%s/%s%s" % (key, what, "/moved" if aimed_at_moved else "")] = (int((mt["triId"] < 0).sum()), int((~T["robust"] & (mt["triId"] != T["tri"]) & ~tie & ~((mt["triId"] >= 0) & (mt["t"] < T["t"]))).sum()))
        r.close(); c.close()
    print("control, the default intersector on the same rays [%s], (no hit, slips): %s" % (tree, control))
    if refit:
        print("sets aimed at the moved mesh [%s]: slips to a farther hit at silhouette edges (no ray without a hit): %s" % (tree, moved_slips))


def test_the_intersector_belongs_to_the_tree(table, standin_small, monkeypatch):
    s = standin_small
    rays = ttt.rays_random(s, 600, 21)
    r = fa.Renderer(s, 8, 8, fa.default_options(2), table=table)
    assert r.intersector() == (0, 0)
    mt_hits = r.trace(rays); mt_nodes, mt_recs = r.download_bvh()
    # a request alone touches nothing
    r.set_intersector(fa.INTERSECTOR_WATERTIGHT)
    assert r.intersector() == (1, 0)
    assert r.trace(rays).tobytes() == mt_hits.tobytes() and r.download_bvh()[1].tobytes() == mt_recs.tobytes()
    with pytest.raises(fa.FptError):
        r.set_intersector(2)
    assert r.intersector() == (1, 0)
    # a rebuild: tree and description together; the records hold the vertices, the nodes are the same tree
    r.rebuild_geometry()
    assert r.intersector() == (1, 1)
    nodes, recs = r.download_bvh()
    assert nodes.tobytes() == mt_nodes.tobytes()
    ids = recs[:, 9].view(np.int32)
    vi = s.vertex_indices[ids, :3]; P = s.vertex_data[:, :3]
    assert np.array_equal(recs[:, 0:3], P[vi[:, 0]]) and np.array_equal(recs[:, 3:6], P[vi[:, 1]]) and np.array_equal(recs[:, 6:9], P[vi[:, 2]])
    assert np.array_equal(recs[:, 9:12].view(np.uint32), mt_recs[:, 9:12].view(np.uint32))          # id, mask, delta: the same words
    assert np.array_equal(mt_recs[:, 3:6], P[vi[:, 1]] - P[vi[:, 0]])
    wt_hits = r.trace(rays)
    assert _same_hits(wt_hits, wt.closest(s.vertex_indices, s.vertex_data, rays))
    assert wt_hits.tobytes() != mt_hits.tobytes()          # another rounding of t on nearly every ray
    # a refused build (an index out of range, in every build mode, whichever intersector is requested) leaves the old tree with its old intersector, usable
    bad_idx = r.d_vi.clone(); bad_idx[7, 1] = s.num_vertices + 5
    for mode in (0, 1, 2):
        for req in (0, 1):
            r.set_build_mode(mode); r.set_intersector(req)
            rc = r.L.fpt_rt_create_geometry(r.ctx, C.c_uint32(s.num_triangles), C.c_void_p(bad_idx.data_ptr()), C.c_uint32(s.num_vertices), C.c_void_p(r.d_vd.data_ptr()))
            assert rc != 0 and b"vertex index out of range" in r.L.fpt_last_error(r.ctx)
            assert r.intersector() == (req, 1)
            assert r.download_bvh()[1].tobytes() == recs.tobytes() and r.trace(rays).tobytes() == wt_hits.tobytes(), (mode, req)
    # back to the default: fpt-MT's bytes again
    r.set_build_mode(0); r.set_intersector(fa.INTERSECTOR_MT); r.rebuild_geometry()
    assert r.intersector() == (0, 0)
    assert r.download_bvh()[1].tobytes() == mt_recs.tobytes() and r.trace(rays).tobytes() == mt_hits.tobytes()
    # FPT_INTERSECTOR overrides the request, either way
    monkeypatch.setenv("FPT_INTERSECTOR", "watertight")
    r.rebuild_geometry()
    assert r.intersector() == (0, 1) and r.trace(rays).tobytes() == wt_hits.tobytes()
    monkeypatch.setenv("FPT_INTERSECTOR", "mt")
    r.set_intersector(fa.INTERSECTOR_WATERTIGHT); r.rebuild_geometry()
    assert r.intersector() == (1, 0) and r.trace(rays).tobytes() == mt_hits.tobytes()
    # the counted launch is the tree's too
    monkeypatch.delenv("FPT_INTERSECTOR")
    r.rebuild_geometry()
    counted, cnt = r.trace(rays, counted=True)
    assert counted.tobytes() == wt_hits.tobytes() and cnt.tris_tested > 0 and cnt.rays == len(rays)
    r.close()


# CornellBox-JP, 128 x 128, 16 passes.  |mean(COMPOSITED_C) watertight - default| / default, measured on an MI355X (the renderers are deterministic), asserted at
# twice the measurement and never above 1 %: almost every path is the same path with another rounding of t, far below the Monte-Carlo noise of the mean
MEAN_MEASURED = {"pt": 1.301e-08, "bpt": 6.725e-08, "psfpt": 8.950e-09}          # 15758, 15607 and 14719 of the 16384 pixels differ in some bit; the means agree to eight digits
PASSES, RES = 16, 128


def _make(kind, s, table):
    L = 6
    if kind == "pt":
        return fa.Renderer(s, RES, RES, fa.default_options(L), table=table)
    if kind == "bpt":
        return fa.Renderer(s, RES, RES, fa.default_options(L), table=table, bpt_options=fa.default_bpt_options(L))
    return fa.Renderer(s, RES, RES, fa.default_options(L), table=table, psf_options=fa.default_psf_options())


def _render(kind, r, in_flight):
    one = {"pt": r.render_pass, "bpt": r.bpt_render, "psfpt": r.psf_render}[kind]
    if not in_flight:
        for i in range(PASSES):
            one(i)
    else:
        {"pt": r.set_batch, "bpt": r.bpt_set_batch, "psfpt": r.psf_set_batch}[kind](PASSES // 2)
        batch = {"pt": r.render_batch, "bpt": r.bpt_render_batch, "psfpt": r.psf_render_batch}[kind]
        batch(0, PASSES // 2); batch(PASSES // 2, PASSES // 2)
    return r.framebuffer()


@pytest.mark.parametrize("kind", ["pt", "bpt", "psfpt"])
def test_renderers_on_a_watertight_tree(kind, table, cornell):
    frames = {}
    for intersector, in_flight in ((1, False), (1, True), (0, False)):
        r = _make(kind, cornell, table)
        r.set_intersector(intersector); r.rebuild_geometry()
        assert r.intersector() == (intersector, intersector)
        frames[intersector, in_flight] = _render(kind, r, in_flight)
        r.close()
    seq, bat, ref = frames[1, False], frames[1, True], frames[0, False]
    assert np.isfinite(seq).all() and np.isfinite(bat).all()
    # the channels the existing promise covers (tests/test_gpu_parity.py, test_psfpt.py, test_bpt.py: the BPT's batches leave FILTERED_C and LUMINANCE alone)
    for c in (range(6) if kind == "bpt" else (0, 1, 2, 3, 4, 5, 7)):
        assert np.array_equal(seq[c].view(np.uint32), bat[c].view(np.uint32)), "%s: channel %d of the passes in flight differs from sequential passes" % (kind, c)
    m_wt, m_mt = float(seq[fa.api.FB_COMPOSITED_C][:, :3].astype(np.float64).mean()), float(ref[fa.api.FB_COMPOSITED_C][:, :3].astype(np.float64).mean())
    rel = abs(m_wt - m_mt) / m_mt
    differing = int((seq[fa.api.FB_COMPOSITED_C] != ref[fa.api.FB_COMPOSITED_C]).any(1).sum())
    print("%s: mean COMPOSITED_C watertight %.9g, default %.9g, relative difference %.3e; %d of %d pixels differ" % (kind, m_wt, m_mt, rel, differing, RES * RES))
    assert m_mt > 1e-3
    bound = min(0.01, 2.0 * MEAN_MEASURED[kind])
    assert rel <= bound, (kind, rel, bound)


def test_the_mirror_renders_with_the_watertight_intersector(tmp_path):
    exe = os.path.join(ROOT, "fermat_amd", "bin", "fermat_hip")
    assert os.path.exists(exe), "fermat_amd/bin/fermat_hip missing: run __graft_entry__.build()"
    d = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    common = [exe, "-i", os.path.join(d, "CornellBox-JP.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "64", "48", "-pt", "-bounces", "4", "-passes", "2"]
    env = {k: v for k, v in os.environ.items() if k not in ("FPT_INTERSECTOR", "FPT_BVH_BUILD")}
    a = subprocess.run(common + ["-intersector", "watertight", "-o", str(tmp_path / "wt")], capture_output=True, text=True, timeout=300, env=env)
    assert a.returncode == 0, a.stderr[-2000:]
    assert "intersector: requested 1, tree 1" in a.stderr, a.stderr[-2000:]          # fpt_rt_intersector, read back after the build
    b = subprocess.run(common + ["-o", str(tmp_path / "mt")], capture_output=True, text=True, timeout=300, env=env)
    assert b.returncode == 0 and "intersector:" not in b.stderr, b.stderr[-2000:]
    wt_img, mt_img = scene.load_tga(str(tmp_path / "wt.tga")), scene.load_tga(str(tmp_path / "mt.tga"))
    assert wt_img.shape == mt_img.shape and wt_img[..., :3].mean() > 0.05
    assert np.abs(wt_img[..., :3] - mt_img[..., :3]).mean() < 0.01          # the same picture: a handful of paths differ by a rounding of t
