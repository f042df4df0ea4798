"""Build mode 2 (trbvh): the device radix tree of mode 1, restructured by 7-leaf treelets (Karras & Aila, HPG 2013) before the collapse (fpt_build_lbvh.hip, stage 3b).
The tree must be as valid as the other two, traced hits must not depend on it, and it must be cheaper to walk than mode 1's radix tree."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene
from oracle import binding as ob

import test_trace_truth as ttt
import trace_truth as tt
from test_gpu_parity import _random_rays, bit_equal
from test_wide_bvh import check_tree, check_containment, decode, _soup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_mode_override(monkeypatch):
    """every test here picks its build modes itself: an FPT_BVH_BUILD of the caller's would override them (monkeypatch restores it afterwards)"""
    monkeypatch.delenv("FPT_BVH_BUILD", raising=False)


def _trbvh(s, table, w=48, h=32, L=4):
    r = fa.Renderer(s, w, h, fa.default_options(L), table=table)
    r.set_build_mode(fa.BUILD_TRBVH); r.rebuild_geometry()
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1: a valid tree, the oracle's hits

def test_trbvh_gives_a_valid_tree_and_the_same_hits(table, cornell_glossy, standin_small):
    for s in (cornell_glossy, standin_small):
        r = fa.Renderer(s, 48, 32, fa.default_options(4), table=table)
        r.render_pass(0)
        want_fb = r.framebuffer().copy()
        r.set_build_mode(2); r.rebuild_geometry()
        st = r.bvh_stats()
        assert st["records"] == s.num_triangles and 1 <= st["stack_need"] <= 48 and st["depth"] >= 1, st
        assert sum(st["slot_hist"]) == st["nodes"] and st["inner_children"] == st["nodes"] - 1, st
        nodes, recs = r.download_bvh()
        assert len(recs) == s.num_triangles
        check_tree(s, nodes, recs, st["depth"], table, 300, 3)
        assert check_containment(nodes, recs) >= len(nodes)
        r.rebuild_geometry()
        n2, r2 = r.download_bvh()
        assert np.array_equal(n2, nodes) and np.array_equal(r2.view(np.uint32), recs.view(np.uint32)), "two trbvh builds of one mesh differ"
        o = ob.OraclePT(s, 16, 16, ob.default_options(2), table, scene.DATA_DIR)
        rays = _random_rays(s, 20000, 5)
        hg = r.trace(rays); ho = o.trace(rays)
        assert np.array_equal(hg["triId"], ho["triId"]) and bit_equal(hg["t"], ho["t"]) and bit_equal(hg["u"], ho["u"]) and bit_equal(hg["v"], ho["v"])
        sh = _random_rays(s, 20000, 6); sh["dir"] *= np.float32(3.0); sh["tmax"] = 0.9999
        sh["mask"] = np.where(np.arange(len(sh)) % 2 == 0, 0x2, 0x1).astype(np.uint32)
        assert np.array_equal(r.trace(sh, shadow=True)["t"], o.trace(sh, shadow=True)["t"])
        r.clear_framebuffer(); r.render_pass(0)
        assert bit_equal(r.framebuffer()[5], want_fb[5])
        # a device refit of the restructured tree
        rng = np.random.default_rng(4)
        ext = float(np.max(np.asarray(s.bbox[1]) - np.asarray(s.bbox[0])))
        moved = s.vertex_data.copy(); moved[:, :3] += (rng.standard_normal((len(moved), 3)) * 0.02 * ext).astype(np.float32)
        r.refit_geometry(moved)
        n3, r3 = r.download_bvh()
        assert np.array_equal(n3[:, 4:8], nodes[:, 4:8]) and check_containment(n3, r3) >= len(nodes)
        s2 = copy.copy(s); s2.vertex_data = moved
        o2 = ob.OraclePT(s2, 16, 16, ob.default_options(2), table, scene.DATA_DIR)
        h2 = r.trace(rays); w2 = o2.trace(rays)
        assert np.array_equal(h2["triId"], w2["triId"]) and bit_equal(h2["t"], w2["t"])
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2: the fp64 judge of test_trace_truth on the restructured tree and on a refit of it (the same cases, truths and slip bounds)

@pytest.mark.parametrize("tree", ["trbvh", "trbvh+refit"])
def test_trbvh_hits_against_fp64_truth(tree, table):
    def renderer(s):
        r = _trbvh(s, table, 8, 8, 2)
        if tree.endswith("+refit"):
            s = ttt._with_vertices(s, ttt._moved(s))
            r.refit_geometry(s.vertex_data)
        return r, s
    by_scene = {}
    for name in ttt.GPU_CLOSEST:
        by_scene.setdefault(ttt.CLOSEST[name][0], []).append(name)
    report = {}
    for key, names in sorted(by_scene.items()):
        r, s = renderer(ttt.get_scene(key))
        for name in names:
            _, rays, T = ttt.closest_case(name)
            if s is not ttt.get_scene(key):
                T = tt.truth(s.vertex_indices, s.vertex_data, rays)
            report[name] = ttt.judge_closest(s, rays, T, r.trace(rays), "%s [%s]" % (name, tree))
        r.close()
    for key in sorted(ttt.ANY):
        r, s = renderer(ttt.masked(ttt.get_scene(key)))
        _, rays, T = ttt.any_case(key)
        if tree.endswith("+refit"):
            T = tt.truth(s.vertex_indices, s.vertex_data, rays, shadow=True)
        report["any/" + key] = ttt.judge_any(s, rays, T, r.trace(rays, shadow=True)["t"] > 0, "any/%s [%s]" % (key, tree))
        r.close()
    print("slips [%s]: %s" % (tree, report))
    over = {k: (v, ttt.SLIP_BOUND.get(k, 0)) for k, v in report.items() if v > ttt.SLIP_BOUND.get(k, 0)}
    assert not over, "slips over their bounds [%s]: %s" % (tree, over)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3: degenerate soups (the inputs of test_gpu_parity.test_device_build_on_degenerate_soups)

def test_trbvh_on_degenerate_soups(table, monkeypatch):
    rng = np.random.default_rng(9)
    for n in (2, 3, 17, 3000):
        idx, vtx = _soup(n, rng, spread=1.0, size=0.05)
        if n == 3000:
            vtx[:300, :3] = np.tile(np.float32([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [0.5, 0.6, 0.5]]), (100, 1))
            vtx[300:330, :3] = np.float32([0.25, 0.25, 0.25])
            vtx[330:360, :3] = np.tile(np.float32([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9], [0.5, 0.5, 0.5]]), (10, 1))
        s = copy.copy(scene.cornell_box("CornellBox-JP"))
        s.vertex_indices = idx; s.vertex_data = vtx; s.num_triangles = len(idx); s.num_vertices = len(vtx)
        s.material_indices = (np.arange(len(idx)) % len(s.materials)).astype(np.int32)
        s.texture_indices_comp = None
        s.bbox = (vtx[:, :3].min(0), vtx[:, :3].max(0))
        monkeypatch.setenv("FPT_BVH_BUILD", "trbvh")
        r = fa.Renderer(s, 16, 16, fa.default_options(2), table=table)
        monkeypatch.delenv("FPT_BVH_BUILD")
        st = r.bvh_stats()
        nodes, recs = r.download_bvh()
        assert sorted(recs[:, 9].view(np.int32).tolist()) == list(range(n)) and check_containment(nodes, recs) >= len(nodes)
        assert 1 <= st["stack_need"] <= 48, st
        o = ob.OraclePT(s, 16, 16, ob.default_options(2), table, scene.DATA_DIR)
        rays = _random_rays(s, 4000, 8)
        hg = r.trace(rays); ho = o.trace(rays)
        assert np.array_equal(hg["triId"], ho["triId"]) and bit_equal(hg["t"], ho["t"])
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4: cheaper to walk than mode 1's tree

def wide_sah(nodes):
    """independent of the builders: the collapse's cost recomputed from the downloaded, dequantised boxes -- sum of the wide nodes' areas + 0.6 x sum of the leaf
    slots' areas x their triangles, relative to the root's area (a node's box = the union of its used slots' boxes)"""
    n = len(nodes)
    b = nodes.view(np.uint8).reshape(n, 80)
    p = nodes[:, :3].view(np.float32).astype(np.float64)
    cell = np.ldexp(1.0, b[:, 12:15].astype(np.int64) - 127)
    q = b[:, 32:80].reshape(n, 6, 8).astype(np.float64)
    lo = p[:, None, :] + q[:, 0:3, :].transpose(0, 2, 1) * cell[:, None, :]          # [node, slot, axis]
    hi = p[:, None, :] + q[:, 3:6, :].transpose(0, 2, 1) * cell[:, None, :]
    for i in range(min(n, 64)):          # the same boxes as test_wide_bvh.decode
        _, _, _, _, _, dlo, dhi = decode(nodes[i])
        assert np.array_equal(dlo, lo[i]) and np.array_equal(dhi, hi[i])
    slot = np.arange(8)
    inner = ((nodes[:, 3:4] >> np.uint32(24)) >> slot.astype(np.uint32)) & 1
    valid = nodes[:, 6:7].astype(np.int64)
    tris = ((valid >> (2 * slot)) & 1) + ((valid >> (2 * slot + 1)) & 1)
    used = (inner > 0) | (tris > 0)
    ha = lambda e: e[..., 0] * e[..., 1] + e[..., 2] * (e[..., 0] + e[..., 1])
    big = 1e300
    nlo = np.where(used[..., None], lo, big).min(1); nhi = np.where(used[..., None], hi, -big).max(1)
    node_area = ha(np.maximum(nhi - nlo, 0.0))
    slot_area = ha(np.maximum(hi - lo, 0.0))
    return (node_area.sum() + 0.6 * (slot_area * tris).sum()) / node_area[0]


def _node_steps(r, ray_sets):
    total, per = 0, []
    for rays in ray_sets:
        _, cnt = r.trace(rays, counted=True)
        total += cnt.nodes_visited; per.append(cnt.nodes_visited / max(1, cnt.rays))
    return total / sum(len(x) for x in ray_sets), per


@pytest.mark.parametrize("which", ["bathroom2_standin", "testball_room", "water_caustic_standin", "standin_small"])
def test_trbvh_is_cheaper_than_the_radix_tree(which, table):
    s = scene.bathroom_standin(0.08) if which == "standin_small" else getattr(scene, which)()
    r = fa.Renderer(s, 160, 90, fa.default_options(3), table=table)
    ray_sets = []
    for b in (0, 1):
        r.set_capture(b); r.clear_framebuffer(); r.render_pass(0, sync=True)
        rays = r.captured()["rays"].copy()
        rays["mask"] = np.float32(0.0 if b == 0 else 1e-3).view(np.uint32)
        rays["tmax"] = np.float32(1e34 if b == 0 else 1e8)
        assert len(rays) > 1000
        ray_sets.append(rays)
    r.set_capture(-1)
    ray_sets.append(_random_rays(s, 2000000, 12))
    got = {}
    for mode in (1, 2):
        r.set_build_mode(mode); r.rebuild_geometry()
        nodes, _ = r.download_bvh()
        steps, per = _node_steps(r, ray_sets)
        got[mode] = dict(sah=wide_sah(nodes), steps=steps, per=per, stats=r.bvh_stats())
    r.close()
    print("%s: wide SAH %.3f -> %.3f, node steps / ray %.3f -> %.3f (bounce 0, 1, random: %s -> %s), stats %s"
          % (which, got[1]["sah"], got[2]["sah"], got[1]["steps"], got[2]["steps"], np.round(got[1]["per"], 3).tolist(), np.round(got[2]["per"], 3).tolist(), got[2]["stats"]))
    assert got[2]["sah"] < got[1]["sah"], which
    assert got[2]["steps"] < got[1]["steps"], which
    if which in ("bathroom2_standin", "testball_room"):
        assert got[2]["steps"] <= 0.95 * got[1]["steps"], (which, got[2]["steps"] / got[1]["steps"])
    st = got[2]["stats"]
    assert st["inner_area_after"] < st["inner_area_before"] and st["optimise_iterations"] >= 1 and st["sah_cost_wide"] > 0, st


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5: through the renderers

def test_trbvh_through_the_renderers(tmp_path, table, monkeypatch):
    exe = os.path.join(ROOT, "fermat_amd", "bin", "fermat_hip")
    assert os.path.exists(exe), "fermat_amd/bin/fermat_hip missing: run __graft_entry__.build()"
    d = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    out = str(tmp_path / "img")
    imgs = {}
    for bvh in ("quality", "trbvh"):
        p = subprocess.run([exe, "-i", os.path.join(d, "CornellBox-Glossy.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "64", "48", "-pt",
                            "-bounces", "4", "-passes", "2", "-bvh", bvh, "-o", out + "_" + bvh], capture_output=True, text=True, timeout=300, env=dict(os.environ, FPT_BVH_TIMERS="1"))
        assert p.returncode == 0, p.stderr[-2000:]
        assert ("built on the device" in p.stderr) == (bvh == "trbvh") and ("restructuring" in p.stderr) == (bvh == "trbvh")
        imgs[bvh] = scene.load_tga(out + "_" + bvh + ".tga")
    assert np.array_equal(imgs["trbvh"], imgs["quality"])
    # BPT and PSFPT: the quality tree's frame bit for bit
    s = scene.cornell_box("CornellBox-Glossy")
    frames = {}
    for bvh in ("quality", "trbvh"):
        monkeypatch.setenv("FPT_BVH_BUILD", bvh)
        rb = fa.Renderer(s, 64, 48, fa.default_options(5), table=table, bpt_options=fa.default_bpt_options(5))
        rp = fa.Renderer(s, 64, 48, fa.default_options(5), table=table, psf_options=fa.default_psf_options())
        monkeypatch.delenv("FPT_BVH_BUILD")
        assert (rb.bvh_stats()["optimise_iterations"] == 3) == (bvh == "trbvh")
        rb.clear_gbuffer()
        for i in range(2):
            rb.bpt_render(i, sync=True); rp.psf_render(i, sync=True)
        frames[bvh] = (rb.framebuffer().copy(), rp.framebuffer().copy())
        rb.close(); rp.close()
    for k in range(2):
        assert np.array_equal(frames["trbvh"][k].view(np.uint32), frames["quality"][k].view(np.uint32)), ("bpt", "psfpt")[k]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6: bad input

def test_trbvh_bad_input(table, cornell, monkeypatch):
    r = fa.Renderer(cornell, 16, 16, fa.default_options(2), table=table)
    with pytest.raises(fa.FptError, match="trbvh"):
        r.set_build_mode(3)
    L = fa.lib()
    bad = r.d_vi.clone(); bad[7, 1] = cornell.num_vertices + 5
    for mode in (1, 2):
        r.set_build_mode(mode)
        assert L.fpt_rt_create_geometry(r.ctx, C.c_uint32(cornell.num_triangles), C.c_void_p(bad.data_ptr()), C.c_uint32(cornell.num_vertices), C.c_void_p(r.d_vd.data_ptr())) != 0
        assert b"vertex index out of range" in L.fpt_last_error(r.ctx), mode
    r.set_build_mode(0)
    monkeypatch.setenv("FPT_BVH_BUILD", "trbvh")
    assert L.fpt_rt_create_geometry(r.ctx, C.c_uint32(cornell.num_triangles), C.c_void_p(bad.data_ptr()), C.c_uint32(cornell.num_vertices), C.c_void_p(r.d_vd.data_ptr())) != 0
    assert b"vertex index out of range" in L.fpt_last_error(r.ctx)
    r.close()
