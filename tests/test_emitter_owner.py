"""The emitter tables' one owner (EmitterSet, fpt_host.h) seen through the C-ABI: a refused host build leaves the old tables usable, fpt_mesh_lights_update's shortcut
knows who built the live tables, the tables and the frames do not depend on the route taken to them, and an unlit scene is a valid set on both routes.  "Tables" are
the four arrays and `norm` of Renderer.lights(), compared bitwise; CornellBox-JP at 16x12, three-vertex paths."""
import copy
import ctypes as C

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene
from test_gpu_device_emitters import assert_tables_equal, bit_equal, frames_equal, moved_cornell

pytestmark = pytest.mark.gpu

W, H = 16, 12


class LightsView(C.Structure):          # fpt_mesh_lights_view (include/fermat_pt_hip.h)
    _fields_ = [("d_mesh_cdf", C.c_void_p), ("d_mesh_inv_area", C.c_void_p), ("n_prims", C.c_uint32), ("d_vpls", C.c_void_p), ("d_vpl_cdf", C.c_void_p),
                ("n_vpls", C.c_uint32), ("norm", C.c_float)]


def device_view(r):
    v = LightsView()
    assert r.L.fpt_mesh_lights_device_view(r.ctx, C.byref(v)) == 0, r.L.fpt_last_error(r.ctx)
    return (v.d_mesh_cdf, v.d_mesh_inv_area, v.n_prims, v.d_vpls, v.d_vpl_cdf, v.n_vpls, np.float32(v.norm).tobytes())


def render(r, first, n=2):
    for i in range(first, first + n):
        r.render_pass(i)
    return r.framebuffer()


# 1 ---- a refused host build leaves the old tables usable
def test_refused_host_build_leaves_the_old_tables_usable(table, cornell):
    opts = fa.default_options(3)
    twin = fa.Renderer(cornell, W, H, opts, table=table)
    twin.reinit_emitters(500)
    want_frame = render(twin, 0)
    twin.close()
    r = fa.Renderer(cornell, W, H, opts, table=table)
    r.reinit_emitters(500)
    before = r.lights(); view_before = device_view(r)
    assert len(before["vpls"]) == 500 and view_before[5] == 500
    no_materials = fa.api.MeshView.from_buffer_copy(r.h_mesh); no_materials.material_indices = None
    no_vertices = fa.api.MeshView.from_buffer_copy(r.h_mesh); no_vertices.vertex_data = None
    assert r.h_mesh.material_indices and r.h_mesh.vertex_data, "the renderer's own view is whole"
    rebuilt = C.c_int(-1)
    for what, mesh in (("a NULL mesh", None), ("null material_indices", C.byref(no_materials)), ("null vertex_data", C.byref(no_vertices))):
        calls = (("fpt_mesh_lights_init", lambda: r.L.fpt_mesh_lights_init(r.ctx, C.c_uint32(300), mesh, C.byref(r._h_tex), C.c_uint32(0))),
                 ("fpt_mesh_lights_update", lambda: r.L.fpt_mesh_lights_update(r.ctx, C.c_uint32(300), mesh, C.byref(r._h_tex), C.c_uint32(0), C.byref(rebuilt))))
        for name, call in calls:
            assert call() != 0, "%s accepted %s" % (name, what)
            assert b"fpt_mesh_lights_init" in r.L.fpt_last_error(r.ctx), r.L.fpt_last_error(r.ctx)          # fpt_mesh_lights_update forwards to it
            assert_tables_equal(r.lights(), before, "after %s with %s" % (name, what))
            assert device_view(r) == view_before, "%s with %s moved or resized the tables" % (name, what)
    frames_equal(render(r, 0), want_frame)
    r.close()


# 2 ---- the shortcut knows who built the tables
def test_the_shortcut_knows_who_built_the_tables(table):
    s = scene.cornell_box("CornellBox-JP")          # its vertices are edited in place below: not the session's scene
    n = W * H
    r = fa.Renderer(s, W, H, fa.default_options(3), table=table)
    assert r.update_emitters(n) == 0, "host-built from this mesh, nothing moved"
    r.init_emitters_device(n)
    assert r.update_emitters(n) == 1, "the live tables were built on the device: no fingerprint to compare with"
    assert_tables_equal(r.lights(), fa.api.host_emitter_tables(s, n), "rebuilt on the host after a device build")
    assert r.update_emitters(n) == 0
    assert r.update_emitters(n + 1) == 1
    assert len(r.lights()["vpls"]) == n + 1
    moved, _ = moved_cornell("light")
    s.vertex_data[:] = moved.vertex_data
    r.refit_geometry(s.vertex_data)
    assert r.update_emitters(n + 1) == 1, "an emitting triangle moved"
    assert_tables_equal(r.lights(), fa.api.host_emitter_tables(moved, n + 1), "after the light moved")
    pushed, touched = moved_cornell("box")
    s.vertex_data[touched] = pushed.vertex_data[touched]          # the box alone: the light stays where it was moved to
    r.refit_geometry(s.vertex_data)
    assert r.update_emitters(n + 1) == 0, "only a non-emitter moved"
    r.close()


# 3 ---- the result does not depend on the route taken to it
@pytest.mark.parametrize("nee_type", [1, 0])
def test_the_result_does_not_depend_on_the_route(table, cornell, nee_type):
    opts = fa.default_options(3, nee_type)
    a = fa.Renderer(cornell, W, H, opts, table=table)
    a.init_emitters_device(700)
    a.reinit_emitters(500)
    b = fa.Renderer(cornell, W, H, opts, table=table)
    b.reinit_emitters(500)
    tables_a = a.lights()
    assert len(tables_a["vpls"]) == 500 and device_view(a)[5] == 500
    assert_tables_equal(tables_a, b.lights(), "host, device, host against host, host")
    frames_equal(render(a, 0), render(b, 0))
    b.close()
    # the device builder rebuilds with the parameters of its own last init, whatever the host route built since
    a.update_emitters_device()
    assert_tables_equal(a.lights(), fa.api.host_emitter_tables(cornell, 700), "update_device after a host re-init")
    fb = render(a, 2)
    assert np.isfinite(fb).all() and fb[5][:, :3].max() > 0.5
    a.close()


# 4 ---- an unlit scene is a valid set on both routes
def test_an_unlit_scene_on_both_routes(table, cornell):
    s = copy.copy(cornell)
    s.materials = cornell.materials.copy(); s.materials["emissive"][:] = 0.0
    nt = s.num_triangles
    uniform = (np.arange(1, nt + 1, dtype=np.uint32).astype(np.float32) / np.float32(nt)).astype(np.float32)
    r = fa.Renderer(s, W, H, fa.default_options(3), table=table)          # builds on the host
    for route in ("host", "device"):
        if route == "device":
            r.init_emitters_device()
        got = r.lights()
        assert len(got["vpls"]) == 0 and len(got["vpl_cdf"]) == 0 and got["norm"] == 0.0, route
        assert bit_equal(got["mesh_cdf"], uniform), route
        view = device_view(r)
        assert view[2] == nt and view[5] == 0 and view[3] is None and view[4] is None, route
        # with no VPLs fpt_pt_init falls back to mesh NEE (a VPL draw from an empty set would index it)
        assert r.L.fpt_pt_init(r.ctx, C.byref(r.options), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(r.n_local)) == 0, r.L.fpt_last_error(r.ctx)
        fb = render(r, 0, 1)
        assert np.isfinite(fb).all() and not fb[5][:, :3].any(), route
    r.close()
